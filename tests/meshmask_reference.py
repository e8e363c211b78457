"""The reference formulation of the masked-mesh feature, in numpy: ``filter_edges``, ``build_masked_graph`` and
``reconstruct_graph`` of the reference's ``utils/meshmask.py`` statement by statement, the node count of
``utils/torch_graph.get_masked_indexes`` and the row mask of ``utils/loss._prepare_mask_for_loss``.  tests/test_meshmask_host.py
pins this file to arrays minted from the reference itself (tests/golden/meshmask.npz); the GPU tests compare the kernels against it."""
import numpy as np


def masked_count(n, masking_ratio):
    """``int((1 - masking_ratio) * n)`` in Python float arithmetic (torch_graph.py:321-322)"""
    nodes_to_keep = 1 - masking_ratio
    return int(nodes_to_keep * n)


def filter_edges_reference(edge_index, node_index, edge_attr=None, num_nodes=None):
    """(edge_index' int64 [2, E'], edge_attr' or None, mask bool [E])  (meshmask.py:22-37)"""
    edge_index = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    node_index = np.asarray(node_index, dtype=np.int64).reshape(-1)
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.size else 0
    cluster_index = np.arange(node_index.shape[0], dtype=np.int64)
    table = np.full(num_nodes, -1, dtype=np.int64)
    table[node_index] = cluster_index          # an index outside [0, num_nodes) raises IndexError, as the torch statement does
    senders, receivers = table[edge_index[0]], table[edge_index[1]]
    mask = (senders >= 0) & (receivers >= 0)
    attr = None if edge_attr is None else np.asarray(edge_attr)[mask]
    return np.stack([senders[mask], receivers[mask]]), attr, mask


def build_masked_graph_reference(x, pos, edge_index, edge_attr, selected_indexes, num_nodes=None):
    """a dict of the fields ``build_masked_graph`` replaces, and the edge mask (meshmask.py:58-70)"""
    sel = np.asarray(selected_indexes, dtype=np.int64)
    ei, attr, mask = filter_edges_reference(edge_index, sel, edge_attr, num_nodes=num_nodes)
    return {"x": np.asarray(x)[sel], "pos": None if pos is None else np.asarray(pos)[sel], "edge_index": ei, "edge_attr": attr}, mask


def reconstruct_reference(n, latent_x, selected_indexes, node_mask_token, edges_mask=None, encoded_edge_attr=None,
                          latent_edge_attr=None, edge_mask_token=None):
    """(x [n, f], edge_attr or None) of the reconstructed mesh (meshmask.py:104-116); ``encoded_edge_attr`` is the edge encoder's
    output on the full mesh's edge_attr"""
    latent_x = np.asarray(latent_x)
    x = np.zeros((n, latent_x.shape[1]), dtype=latent_x.dtype) + np.asarray(node_mask_token).reshape(1, -1)
    x[np.asarray(selected_indexes, dtype=np.int64)] = latent_x
    attr = None
    if encoded_edge_attr is not None:
        attr = np.asarray(encoded_edge_attr) + np.asarray(edge_mask_token).reshape(1, -1)
        attr[np.asarray(edges_mask, dtype=bool)] = np.asarray(latent_edge_attr)
    return x, attr


def reconstruct_gradients_reference(g_x, selected_indexes, g_e=None, edges_mask=None):
    """gradients of ``reconstruct_reference`` for incoming ``g_x`` / ``g_e``: a dict with d_latent_x, d_node_token and, with edges,
    d_latent_edge_attr, d_encoded_edge_attr, d_edge_token"""
    g_x = np.asarray(g_x)
    sel = np.asarray(selected_indexes, dtype=np.int64)
    masked = np.ones(g_x.shape[0], dtype=bool)
    masked[sel] = False
    out = {"d_latent_x": g_x[sel], "d_node_token": g_x[masked].sum(0)}
    if g_e is not None:
        g_e, m = np.asarray(g_e), np.asarray(edges_mask, dtype=bool)
        d_enc = g_e.copy()
        d_enc[m] = 0
        out.update({"d_latent_edge_attr": g_e[m], "d_encoded_edge_attr": d_enc, "d_edge_token": g_e[~m].sum(0)})
    return out


def loss_row_mask(node_type, masks, selected_indexes=None):
    """rows that take part in a loss's mean (loss.py:19-34): a type of ``masks`` and NOT listed in ``selected_indexes``"""
    node_type = np.asarray(node_type)
    mask = np.isin(node_type, [int(m) for m in masks])
    if selected_indexes is not None:
        mask &= ~np.isin(np.arange(node_type.shape[0]), np.asarray(selected_indexes))
    return mask
