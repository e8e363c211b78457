"""The reference formulation of the sub-mesh feature, in numpy: ``torch_geometric.utils.subgraph(subset, edge_index, edge_attr,
relabel_nodes=True, num_nodes=N)`` of torch-geometric 2.6.1 for an index subset, statement by statement
(``index_to_mask``, the edge mask, the boolean selection, the relabel through a scatter of ``arange``), and
``BaseDataset._apply_partition`` of the reference on top of it (graphphysics/dataset/dataset.py:244-302).
torch_geometric is not a dependency of this repository; the tests compare the HIP kernels against this file."""
import numpy as np


def index_to_mask(index, size):
    mask = np.zeros(size, dtype=bool)
    mask[index] = True          # an index outside [0, size) raises IndexError, as the torch statement does
    return mask


def subgraph_reference(subset, edge_index, edge_attr=None, num_nodes=None, return_edge_mask=False):
    """(edge_index' int64 [2, E'], edge_attr' or None[, edge_mask bool [E]])"""
    subset = np.asarray(subset, dtype=np.int64).reshape(-1)
    edge_index = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.size else 0
    if subset.size and (subset.min() < 0 or subset.max() >= num_nodes):
        raise IndexError("subset entry outside [0, num_nodes)")
    node_mask = index_to_mask(subset, num_nodes)
    edge_mask = node_mask[edge_index[0]] & node_mask[edge_index[1]]
    out = edge_index[:, edge_mask]
    attr = None if edge_attr is None else np.asarray(edge_attr)[edge_mask]
    node_idx = np.zeros(num_nodes, dtype=np.int64)
    node_idx[subset] = np.arange(subset.shape[0], dtype=np.int64)
    out = node_idx[out]
    return (out, attr, edge_mask) if return_edge_mask else (out, attr)


def apply_partition_reference(x, y, pos, edge_index, edge_attr, node_ids, traj_index=None):
    """``_apply_partition``: a dict with the fields of the sub-graph (and nothing else: ``face`` is not carried)"""
    node_ids = np.sort(np.asarray(node_ids, dtype=np.int64))
    num_nodes = np.asarray(x).shape[0]
    ei, attr = subgraph_reference(node_ids, edge_index, edge_attr, num_nodes=num_nodes)
    return {"x": np.asarray(x)[node_ids], "y": None if y is None else np.asarray(y)[node_ids],
            "pos": None if pos is None else np.asarray(pos)[node_ids], "edge_index": ei, "edge_attr": attr,
            "num_nodes": int(node_ids.shape[0]), "traj_index": traj_index}
