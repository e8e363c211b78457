"""On-device input construction: what the reference's CPU
dataloader does per sample with PyG transforms -- ``T.FaceToEdge`` + ``to_undirected``,
``T.Cartesian(norm=False)``, ``T.Distance(norm=False)`` (graphphysics/dataset/preprocessing.py:
16-23,421-424; torch-geometric==2.6.1) -- as HIP kernels on the MI355X (csrc/mgn_prep.hip).
There is no CPU path here: CPU tensors raise ``RuntimeError``."""
from __future__ import annotations

from typing import Optional

import torch

from . import _capi
from ._launch import call, ptr as _ptr, stream_object, workspace
from .ops import _require_device


def faces_to_edges(face: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """face [K,F] (K = 3 triangles or 4 tetrahedra, PyG ``data.face`` layout) -> edge_index [2,E]
    int64: every pair of corners in both directions, sorted by (src,dst), duplicates and self
    loops removed.  One-time topology prep: synchronises once to read E."""
    _require_device(face)
    if face.dim() != 2 or face.shape[0] not in (3, 4):
        raise ValueError("face must have shape [3, F] or [4, F]")
    L = _capi.lib()
    dev = face.device
    f = face.to(torch.int64).contiguous()
    K, F = int(f.shape[0]), int(f.shape[1])
    cap = F * K * (K - 1)
    out = torch.empty(2, max(cap, 1), dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = workspace(L.mgn_faces_to_edges_workspace_bytes(F, K), dev)
    rc = call("mgn_faces_to_edges", dev, _ptr(f), K, F, int(num_nodes), out[0].data_ptr(), out[1].data_ptr(), _ptr(n),
              _ptr(ws), ws.numel(), accept=(3,))
    if rc == 3:
        raise IndexError(f"face has corners outside [0, {num_nodes})")
    E = int(n.item())
    return out[:, :E].contiguous()


def edge_features(pos: torch.Tensor, edge_index: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """edge_attr [E, D+1] = [pos[src]-pos[dst], ||pos[dst]-pos[src]||_2] (Cartesian then Distance)."""
    _require_device(pos, edge_index)
    D = int(pos.shape[1])
    if D not in (2, 3):
        raise ValueError("pos must be [N,2] or [N,3]")
    p = pos.to(torch.float32).contiguous()
    ei = edge_index.to(torch.int64).contiguous()
    E = int(ei.shape[1])
    if out is None:
        out = torch.empty(E, D + 1, dtype=torch.float32, device=pos.device)
    call("mgn_edge_features", pos.device, _ptr(p), D, ei[0].data_ptr(), ei[1].data_ptr(), E, _ptr(out))
    return out


def add_world_edges(x: torch.Tensor, edge_index: torch.Tensor, world_pos_index_start: int, world_pos_index_end: int,
                    node_type_index: int, radius: float = 0.03, max_world_pairs: Optional[int] = None) -> torch.Tensor:
    """``add_world_edges`` of the reference (preprocessing.py:92-140): OBSTACLE-NORMAL node pairs
    within ``radius`` in world position, both directions, merged with ``edge_index`` and coalesced.
    ``max_world_pairs`` bounds the output buffer (default 16 per node)."""
    _require_device(x, edge_index)
    L = _capi.lib()
    dev = x.device
    xx = x.to(torch.float32).contiguous()
    N, D = int(xx.shape[0]), int(world_pos_index_end - world_pos_index_start)
    if D not in (2, 3):
        raise ValueError("world positions must be 2-D or 3-D")
    ei = edge_index.to(torch.int64).contiguous()
    E = int(ei.shape[1])
    mw = int(max_world_pairs if max_world_pairs is not None else 16 * N)
    out = torch.empty(2, 2 * E + 2 * mw + 1, dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = workspace(L.mgn_world_edges_workspace_bytes(E, mw), dev)
    rc = call("mgn_add_world_edges", dev, _ptr(xx), int(xx.shape[1]), int(world_pos_index_start), D, int(node_type_index), N, float(radius),
              ei[0].data_ptr(), ei[1].data_ptr(), E, mw, out[0].data_ptr(), out[1].data_ptr(), _ptr(n), _ptr(ws), ws.numel(),
              accept=(3, 4))
    if rc == 3:
        raise IndexError(f"edge_index has entries outside [0, {N})")
    if rc == 4:
        raise RuntimeError("more world-edge pairs than max_world_pairs; pass a larger bound")
    return out[:, :int(n.item())].contiguous()


def _khop(edge_index: torch.Tensor, num_nodes: int, num_hops: int):
    """(k-hop edge_index, number of rows that took the bitmap path of csrc/mgn_khop.hip)"""
    import ctypes as C

    L = _capi.lib()
    dev = edge_index.device
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, E]")
    ei = edge_index.to(torch.int64).contiguous()
    N, E = int(num_nodes), int(ei.shape[1])
    nbytes = L.mgn_khop_workspace_bytes(N, E)
    ws = workspace(nbytes, dev)
    n_out, n_ovf = C.c_int64(0), C.c_int64(0)
    rc = call("mgn_khop_count", dev, ei[0].data_ptr(), ei[1].data_ptr(), E, N, int(num_hops), C.byref(n_out), C.byref(n_ovf),
              _ptr(ws), nbytes, accept=(3,))
    if rc == 3:
        raise IndexError(f"edge_index has entries outside [0, {N})")
    out = torch.empty(2, n_out.value, dtype=torch.int64, device=dev)
    if n_out.value > 0:
        call("mgn_khop_fill", dev, _ptr(ws), nbytes, N, int(num_hops), out[0].data_ptr(), out[1].data_ptr(), n_out.value)
    return out, n_ovf.value


def khop_edges(edge_index: torch.Tensor, num_nodes: int, num_hops: int) -> torch.Tensor:
    """``compute_k_hop_edge_index`` of the reference (utils/torch_graph.py:14-105) on the device: the int64 [2, E_k] set of
    ordered pairs (i, j), i != j, such that a directed walk of 1..``num_hops`` edges leads from i (row 0) to j (row 1),
    sorted by (row 0, row 1), each pair once -- the order of the coalesced COO tensor the reference returns.  The input may be
    unsorted, hold duplicates and self loops, be asymmetric and leave nodes isolated.  ``num_hops == 1`` returns the input
    object unchanged (the reference expands only for ``khop > 1``); ``num_hops < 1`` is a ``ValueError``.

    One wavefront searches one row in LDS; a row with more than ``mgn_khop_row_capacity()`` (1024) entries -- a hub node, a
    large k on a 3-D mesh -- goes through a bitmap search in global memory that is exact but slow (about 3 * N/32 words per
    level per such row).  One-time topology prep: synchronises to read E_k."""
    if isinstance(num_hops, bool) or not isinstance(num_hops, int):
        raise ValueError(f"num_hops must be an integer >= 1, got {num_hops!r}")
    if num_hops < 1:
        raise ValueError(f"num_hops must be >= 1, got {num_hops}")
    _require_device(edge_index)
    if num_hops == 1:
        return edge_index
    return _khop(edge_index, num_nodes, num_hops)[0]


def khop_graph(graph, num_hops: int, add_edge_features: bool = True):
    """``compute_k_hop_graph`` of the reference (utils/torch_graph.py): ``graph.edge_index`` becomes its k-hop expansion;
    with ``add_edge_features`` ``graph.edge_attr`` is recomputed on the new edges as mesh-space Cartesian + Distance only
    (earlier extra edge columns are dropped, as the reference does), otherwise it is removed (``_may_remove_edges_attr``)."""
    graph.edge_index = khop_edges(graph.edge_index, int(graph.x.shape[0] if graph.x is not None else graph.pos.shape[0]), num_hops)
    graph.edge_attr = edge_features(graph.pos, graph.edge_index) if add_edge_features else None
    return graph


# ----------------------------------------------------------------------------------------- induced sub-meshes (partitioning)
def _rows_as_words(t: torch.Tensor) -> torch.Tensor:
    """a [R, W] view of ``t`` in 32-bit elements (what mgn_gather_rows_batch copies)"""
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2:
        t = t.reshape(t.shape[0], -1)
    if t.element_size() % 4 != 0:
        raise ValueError(f"row gather: rows of {t.dtype} are not made of 32-bit elements")
    if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t if t.dtype == torch.float32 else t.view(torch.int32)


def gather_rows_batch(sources, indices):
    """``[src[idx] for src, idx in zip(sources, indices)]`` as ONE launch of ``mgn_gather_rows_batch`` (up to 8 tensors; a
    ``None`` source gives ``None``).  Rows of any width made of 32-bit elements, int64 indices; no host synchronisation."""
    live = [(i, s) for i, s in enumerate(sources) if s is not None]
    if len(live) > _capi.MAX_GATHER_JOBS:
        raise ValueError(f"at most {_capi.MAX_GATHER_JOBS} tensors per launch")
    outs = [None] * len(sources)
    if not live:
        return outs
    _require_device(*[s for _, s in live], *[indices[i] for i, _ in live])
    dev = live[0][1].device
    jobs = (_capi.GatherJob * len(live))()
    keep = []
    n = 0
    for i, s in live:
        idx = indices[i]
        if idx.dtype != torch.int64 or not idx.is_contiguous():
            idx = idx.to(torch.int64).contiguous()
        rows = int(idx.numel())
        out = torch.empty((rows,) + tuple(s.shape[1:]), dtype=s.dtype, device=dev)
        outs[i] = out
        if rows == 0 or out.numel() == 0:
            continue
        w_src, w_dst = _rows_as_words(s), _rows_as_words(out)
        j = jobs[n]
        j.src, j.ld_src, j.width, j.idx, j.rows = w_src.data_ptr(), int(w_src.stride(0)) if w_src.shape[0] > 1 else int(w_src.shape[1]), int(w_src.shape[1]), idx.data_ptr(), rows
        j.dst, j.ld_dst, j.src_rows = w_dst.data_ptr(), int(w_dst.shape[1]), int(w_src.shape[0])
        keep += [w_src, w_dst, idx]
        n += 1
    if n:
        call("mgn_gather_rows_batch", dev, n, jobs)
    return outs


def _subgraph_count(subset: torch.Tensor, ei: torch.Tensor, N: int, ws: torch.Tensor) -> int:
    """``mgn_subgraph_count``: the one call of the sub-mesh path that synchronises with the host (tests count its calls)"""
    import ctypes as C

    dev = ei.device
    S, E = int(subset.numel()), int(ei.shape[1])
    n_edges = C.c_int64(0)
    rc = call("mgn_subgraph_count", dev, subset.data_ptr() if S else None, S, N, ei[0].data_ptr() if E else None,
              ei[1].data_ptr() if E else None, E, C.byref(n_edges), _ptr(ws), ws.numel(), accept=(3, 5))
    if rc == 3:
        raise IndexError(f"subset or edge_index has entries outside [0, {N})")
    if rc == 5:
        raise ValueError("subset lists a node twice")
    return n_edges.value


def _subgraph_edges(subset: torch.Tensor, edge_index: torch.Tensor, num_nodes: int, want_mask: bool = False):
    """(edge_index' int64 [2, E'], edge_pos int64 [E'], edge mask bool [E] or None) of csrc/mgn_subgraph.hip"""
    L = _capi.lib()
    dev = edge_index.device
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, E]")
    if subset.dim() != 1 or subset.dtype == torch.bool or subset.is_floating_point():
        raise ValueError("subset must be a 1-D tensor of node indices")
    ei = edge_index if edge_index.dtype == torch.int64 and edge_index.is_contiguous() else edge_index.to(torch.int64).contiguous()
    ids = subset if subset.dtype == torch.int64 and subset.is_contiguous() else subset.to(torch.int64).contiguous()
    N, E = int(num_nodes), int(ei.shape[1])
    nbytes = L.mgn_subgraph_workspace_bytes(N, E)
    if nbytes == 0:
        raise ValueError(f"subgraph: num_nodes = {N} / {E} edges are outside what the kernels index")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    n = _subgraph_count(ids, ei, N, ws)
    out = torch.empty(2, n, dtype=torch.int64, device=dev)
    edge_pos = torch.empty(n, dtype=torch.int64, device=dev)
    mask = torch.empty(E, dtype=torch.uint8, device=dev) if want_mask else None
    call("mgn_subgraph_fill", dev, _ptr(ws), nbytes, E, out[0].data_ptr() if n else None, out[1].data_ptr() if n else None,
         edge_pos.data_ptr() if n else None, mask.data_ptr() if want_mask and E else None, n)
    return out, edge_pos, (mask.view(torch.bool) if want_mask else None)


def subgraph(subset: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None,
             num_nodes: Optional[int] = None, return_edge_mask: bool = False):
    """``torch_geometric.utils.subgraph(subset, edge_index, edge_attr, relabel_nodes=True, num_nodes=...)`` of torch-geometric
    2.6.1 for an INDEX subset, on the device: the edges with both ends in ``subset`` in input order, relabelled to the position
    in ``subset`` (which need not be sorted), their ``edge_attr`` rows; duplicates and self loops of the input are kept.  Returns
    ``(edge_index' int64 [2, E'], edge_attr' or None)`` and with ``return_edge_mask`` also the bool ``[E]`` mask of kept edges.
    ``num_nodes`` defaults to ``edge_index.max() + 1`` as in PyG (one more host synchronisation).  An entry of ``subset`` or
    ``edge_index`` outside ``[0, num_nodes)`` is an ``IndexError``, a node listed twice a ``ValueError`` (PyG relabels such a
    subset to whichever position was scattered last).  Synchronises once to read E'."""
    _require_device(subset, edge_index, edge_attr)
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.numel() else 0
    out, edge_pos, mask = _subgraph_edges(subset, edge_index, num_nodes, want_mask=return_edge_mask)
    attr = gather_rows_batch([edge_attr], [edge_pos])[0]
    return (out, attr, mask) if return_edge_mask else (out, attr)


class PartitionPlan:
    """What every frame of one (trajectory, part) shares: the part's sorted node ids, its relabelled ``edge_index`` and the
    position of each of its edges in the full mesh's edge list."""

    def __init__(self, node_ids: torch.Tensor, edge_index: torch.Tensor, edge_pos: torch.Tensor):
        self.node_ids, self.edge_index, self.edge_pos = node_ids, edge_index, edge_pos


def _graph_num_nodes(graph) -> int:
    if graph.num_nodes is not None:
        return int(graph.num_nodes)
    return int(graph.x.shape[0] if graph.x is not None else graph.pos.shape[0])


def partition_plan(graph, node_ids: torch.Tensor) -> PartitionPlan:
    """The topology half of ``apply_partition``: sort ``node_ids``, cut ``graph.edge_index`` (``mgn_subgraph_count`` +
    ``mgn_subgraph_fill``; synchronises once).  Valid for every frame of the trajectory whose ``edge_index`` is the same."""
    _require_device(node_ids, graph.edge_index)
    ids = torch.sort(node_ids.to(torch.int64))[0]
    ei, edge_pos, _ = _subgraph_edges(ids, graph.edge_index, _graph_num_nodes(graph))
    return PartitionPlan(ids, ei, edge_pos)


def apply_partition(graph, node_ids: Optional[torch.Tensor], plan: Optional[PartitionPlan] = None):
    """``BaseDataset._apply_partition`` of the reference (dataset/dataset.py:244-302): the induced sub-mesh of the sorted
    ``node_ids`` as a NEW ``Graph`` with ``x``, ``y``, ``pos`` (rows of the part's nodes), ``edge_index`` (relabelled),
    ``edge_attr`` (rows of the kept edges), ``num_nodes`` and ``traj_index``.  Nothing else is carried over: ``face`` is
    dropped, as in the reference, and edges that leave the part are dropped -- an approximation of the full-mesh step.
    With the ``plan`` of an earlier call for this part (``partition_plan``) the call is one ``mgn_gather_rows_batch`` launch
    and does not synchronise with the host; ``node_ids`` is then not looked at."""
    from .mesh import Graph

    if plan is None:
        plan = partition_plan(graph, node_ids)
    ids, pos_e = plan.node_ids, plan.edge_pos
    x, y, pos, attr = gather_rows_batch([graph.x, graph.y, graph.pos, graph.edge_attr], [ids, ids, ids, pos_e])
    return Graph(x=x, y=y, pos=pos, edge_index=plan.edge_index, edge_attr=attr, num_nodes=int(ids.numel()),
                 traj_index=graph.traj_index)


def num_partitions_for(num_nodes: int, num_partitions: Optional[int] = None, max_nodes_per_partition: Optional[int] = None) -> int:
    """The number of parts of a trajectory with ``num_nodes`` nodes (``BaseDataset.__init__`` and ``_add_traj_to_index_map``,
    dataset/dataset.py:72-80,135-139): ``num_partitions`` as given, or ``ceil(num_nodes / max_nodes_per_partition)``; naming
    both or neither is a ``ValueError``."""
    import math

    if num_partitions is not None and max_nodes_per_partition is not None:
        raise ValueError("Specify either 'num_partitions' or 'max_nodes_per_partition', not both.")
    if num_partitions is None and max_nodes_per_partition is None:
        raise ValueError("If 'use_partitioning' is True, specify either 'num_partitions' or 'max_nodes_per_partition'.")
    if num_partitions is not None:
        if isinstance(num_partitions, bool) or not isinstance(num_partitions, int) or num_partitions < 1:
            raise ValueError(f"num_partitions must be an integer >= 1, got {num_partitions!r}")
        return num_partitions
    if isinstance(max_nodes_per_partition, bool) or not isinstance(max_nodes_per_partition, int) or max_nodes_per_partition < 1:
        raise ValueError(f"max_nodes_per_partition must be an integer >= 1, got {max_nodes_per_partition!r}")
    return max(1, math.ceil(int(num_nodes) / max_nodes_per_partition))


def partition_sample(local_index: int, num_partitions: int):
    """``(frame_in_traj, part)`` of sample ``local_index`` of a trajectory cut into ``num_partitions`` parts
    (``BaseDataset._get_indices``, dataset/dataset.py:122-123): the parts of one frame are consecutive samples."""
    return int(local_index) // int(num_partitions), int(local_index) % int(num_partitions)


def partition_node_ids(graph, num_partitions: int, method: str = "auto", seed: int = 0):
    """The node ids of each of the ``num_partitions`` parts of ``graph`` as a list of sorted int64 tensors on the graph's
    device (``create_subgraphs`` of the reference, utils/torch_graph.py:108-135).  The parts are those of THIS project's
    partitioner (``partition.partition_nodes``: coordinate bisection + boundary refinement where ``graph.pos`` exists, the
    multilevel scheme otherwise), not METIS' -- the reference reaches METIS through PyG ``ClusterData``, and no two
    partitioners cut a mesh alike.  Host side, once per trajectory.  ``num_partitions == 1`` gives ``[arange(N)]``."""
    import numpy as np

    from .partition import partition_nodes

    if isinstance(num_partitions, bool) or not isinstance(num_partitions, int) or num_partitions < 1:
        raise ValueError(f"num_partitions must be an integer >= 1, got {num_partitions!r}")
    N = _graph_num_nodes(graph)
    dev = graph.edge_index.device
    if num_partitions == 1:
        return [torch.arange(N, dtype=torch.int64, device=dev)]
    pos = graph.pos.detach().cpu().numpy() if graph.pos is not None else None
    part = np.asarray(partition_nodes(pos, graph.edge_index, num_partitions, method=method, seed=seed))
    if part.shape[0] < N:   # without coordinates the partitioner sizes the graph by its largest edge entry
        part = np.concatenate([part, np.zeros(N - part.shape[0], dtype=part.dtype)])
    return [torch.from_numpy(np.nonzero(part == p)[0].astype(np.int64)).to(dev) for p in range(num_partitions)]


# ----------------------------------------------------------------------------------------- random extra edges
RANDEDGE_ROUNDS = 4


def num_random_pairs(num_edges: int, p: float) -> int:
    """K of ``add_random_edges``: ``round(E * p) // 2`` with Python's ``round`` (half to even), as PyG computes it"""
    return round(int(num_edges) * p) // 2


def random_edges_sparse(num_nodes: int, num_edges: int, num_pairs: int) -> bool:
    """the regime predicate of ``add_random_edges``: ``4 (E + K) <= N (N - 1) / 2`` (every real mesh) -> the kernels"""
    return 4 * (int(num_edges) + int(num_pairs)) <= int(num_nodes) * (int(num_nodes) - 1) // 2


def random_edges_candidates(num_nodes: int, num_edges: int, num_pairs: int) -> int:
    """M, the candidates drawn per round in the sparse regime: ``int(1.1 K / (1 - E / P)) + 64``"""
    P = int(num_nodes) * (int(num_nodes) - 1) // 2
    return int(1.1 * int(num_pairs) / (1 - int(num_edges) / P)) + 64


_randedge_state: dict = {}   # per device index: {"flags": device int32[4], "pending": [(event, pinned host copy), ...]}


def _randedge_raise(st, bits: int):
    """the sticky device flag has been seen: clear it (one queued memset), forget older copies of it, raise"""
    st["flags"].zero_()
    stream_object(st["flags"].device).synchronize()   # the error path may wait: later copies must not carry the bit again
    st["pending"].clear()
    if bits & 1:
        raise IndexError("add_random_edges: edge_index has entries outside [0, num_nodes)")
    if bits & 4:
        raise RuntimeError("add_random_edges: the pair table of mgn_randedge overflowed")
    raise RuntimeError("add_random_edges: fewer than K free pairs were found in %d rounds of candidates; the missing columns "
                       "of that call's result hold node 0" % RANDEDGE_ROUNDS)


def _randedge_check(st, wait: bool):
    pending = st["pending"]
    bits = 0
    while pending and (wait or pending[0][0].query()):
        ev, host = pending.pop(0)
        if wait:
            ev.synchronize()
        bits |= int(host[0])
    if bits:
        _randedge_raise(st, bits)


def random_edges_check(device=None) -> None:
    """Look at the deferred error flag of earlier ``add_random_edges`` calls WITHOUT waiting: one event query per call whose
    flag has not been read yet.  Raises what ``random_edges_resolve`` raises if a finished call reported an error."""
    for idx, st in list(_randedge_state.items()):
        if device is None or torch.device(device).index in (None, idx):
            _randedge_check(st, wait=False)


def random_edges_resolve(device=None) -> None:
    """Wait for the deferred error flag of every ``add_random_edges`` call queued so far (on ``device``, default: all devices):
    ``IndexError`` if an ``edge_index`` had entries outside ``[0, num_nodes)``, ``RuntimeError`` if a call came up short of K
    pairs.  The flag is cleared when it is raised."""
    for idx, st in list(_randedge_state.items()):
        if device is None or torch.device(device).index in (None, idx):
            _randedge_check(st, wait=True)


def _random_edges_dense(ei: torch.Tensor, N: int, K: int, seed: int, offset: int) -> torch.Tensor:
    """toy graphs (``P <= 6 E``): enumerate the P pairs, drop the occupied ones, pick ``min(K, free)`` without replacement.
    Torch ops on the device, one host synchronisation; not a hot path."""
    dev = ei.device
    if bool(((ei < 0) | (ei >= N)).any()):
        raise IndexError(f"edge_index has entries outside [0, {N})")
    iu = torch.triu_indices(N, N, offset=1, device=dev)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    occupied = (lo * N + hi)[lo != hi]
    free = iu[:, ~torch.isin(iu[0] * N + iu[1], occupied)]
    gen = torch.Generator(device=dev)
    gen.manual_seed(((int(seed) & (2 ** 64 - 1)) * 0x9E3779B97F4A7C15 + (int(offset) & 0xFFFFFFFF) + 0x45444745) % (2 ** 63))
    n_free = int(free.shape[1])
    pick = torch.randperm(n_free, generator=gen, device=dev)[:min(K, n_free)]
    new = free[:, pick]
    return torch.cat([ei, new, new.flip(0)], dim=1)


def add_random_edges(edge_index: torch.Tensor, num_nodes: int, p: float, seed: int = 0, offset: int = 0,
                     candidates_per_round: Optional[int] = None) -> torch.Tensor:
    """``torch_geometric.utils.add_random_edge(edge_index, p, force_undirected=True)`` of torch-geometric 2.6 -- the "random
    jumps" of the reference's ``Dataset._add_random_edges`` (dataset/dataset.py:171-203) -- on the device:
    ``cat([edge_index, [[lo | hi], [hi | lo]]], dim=1)`` as int64, where the ``K = round(E * p) // 2`` new pairs ``lo < hi`` are
    distinct, not yet edges in either direction and come in acceptance order.  ``K == 0`` or ``num_nodes < 2`` returns the input
    object; ``p`` outside ``[0, 1]``, ``num_nodes >= 2^31`` or ``E >= 2^31`` is a ``ValueError``; a CPU tensor the usual
    ``RuntimeError``.  The input may be unsorted and hold duplicates and self loops.

    Deviation from PyG: a pair counts as occupied when EITHER direction is in the input (PyG looks at ``row < col`` entries
    only); on the symmetric edge lists this pipeline makes the two rules agree.

    The draw is a counter-based stream keyed by ``(seed, offset)`` (include/mgn_hip.h, ``mgn_randedge``) -- pass the training
    step as ``offset`` -- pinned bit for bit by tests/randedge_reference.py; two calls with the same arguments give equal
    tensors.  In the sparse regime (``random_edges_sparse``: every real mesh) the call is a fixed sequence of launches and does
    NOT synchronise with the host.  What only the device knows -- an entry of ``edge_index`` outside ``[0, num_nodes)``
    (``IndexError``), coming up short of K pairs (``RuntimeError``; probability below 1e-50 with the default number of
    candidates per round) -- is raised by a LATER ``add_random_edges`` / ``random_edges_check`` call once the flag has arrived,
    or by ``random_edges_resolve()``.  Denser toy graphs are sampled by enumeration with torch ops (one synchronisation,
    ``K' = min(K, free pairs)``, errors raised at once; a ``torch.Generator`` seeded from ``(seed, offset)``)."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(f"p must be a number in [0, 1], got {p!r}")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, E]")
    N, E = int(num_nodes), int(edge_index.shape[1])
    if N >= 2 ** 31 or E >= 2 ** 31:
        raise ValueError(f"add_random_edges: num_nodes = {N} / {E} edges are outside what the kernels index (< 2^31)")
    _require_device(edge_index)
    K = num_random_pairs(E, p)
    if K == 0 or N < 2:
        return edge_index
    dev = edge_index.device
    ei = edge_index if edge_index.dtype == torch.int64 and edge_index.is_contiguous() else edge_index.to(torch.int64).contiguous()
    if not random_edges_sparse(N, E, K):
        return _random_edges_dense(ei, N, K, seed, offset)
    L = _capi.lib()
    M = random_edges_candidates(N, E, K) if candidates_per_round is None else int(candidates_per_round)
    nbytes = L.mgn_randedge_workspace_bytes(N, E, K, M)
    if M < 1 or nbytes == 0:
        raise ValueError(f"add_random_edges: {E} edges + {K} pairs + {M} candidates per round are outside what the kernels index")
    with torch.cuda.device(dev):
        idx = torch.cuda.current_device()
        st = _randedge_state.get(idx)
        if st is None:
            st = _randedge_state[idx] = {"flags": torch.zeros(4, dtype=torch.int32, device=dev), "pending": []}
        _randedge_check(st, wait=False)   # an earlier call's flag, if it has arrived
        out = torch.empty(2, E + 2 * K, dtype=torch.int64, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("mgn_randedge", dev, ei[0].data_ptr(), ei[1].data_ptr(), E, N, K, M, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
             out[0].data_ptr(), out[1].data_ptr(), _ptr(st["flags"]), _ptr(ws), nbytes)
        host = torch.empty(4, dtype=torch.int32, pin_memory=True)
        host.copy_(st["flags"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream_object(dev))
        st["pending"].append((ev, host))
    return out


def add_noise(graph, noise_index_start, noise_index_end, noise_scale, node_type_index: int, t: Optional[float] = None,
              seed: int = 0, offset: int = 0):
    """``add_noise`` of the reference (preprocessing.py:177-238), on the device and in place: Gaussian noise
    on the given feature column ranges of the NORMAL nodes of ``graph.x``; with ``t`` the curriculum
    scale ``10 * std * (1 + cos(t * pi))``.  Same argument conventions and errors as the reference.
    The noise stream is counter-based (``mgn_add_noise``: Philox4x32-10 keyed by ``seed``, indexed by
    (row, column, range, ``offset``)) -- pass the training-step counter as ``offset``."""
    import ctypes as C
    import math

    if isinstance(noise_index_start, int):
        noise_index_start = [noise_index_start]
    if isinstance(noise_index_end, int):
        noise_index_end = [noise_index_end]
    if isinstance(noise_scale, (float, int)):
        noise_scale = [float(noise_scale)] * len(noise_index_start)
    if len(noise_index_start) != len(noise_index_end):
        raise ValueError("noise_index_start and noise_index_end must have the same length.")
    if len(noise_scale) != len(noise_index_start):
        raise ValueError("noise_scale must have the same length as noise_index_start and noise_index_end.")
    x = graph.x
    _require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("graph.x must be a contiguous float32 tensor (noise is added in place)")
    n = len(noise_index_start)
    scales = [(10 * s * (1 + math.cos(t * math.pi)) if t is not None else s) for s in noise_scale]
    st, en, sc = (C.c_int * n)(*noise_index_start), (C.c_int * n)(*noise_index_end), (C.c_float * n)(*scales)
    call("mgn_add_noise", x.device, _ptr(x), int(x.shape[1]), int(x.shape[0]), n, st, en, sc, int(node_type_index),
         int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF)
    return graph


def add_obstacles_next_pos(graph, world_pos_index_start: int, world_pos_index_end: int, node_type_index: int):
    """``add_obstacles_next_pos`` (preprocessing.py:44-89): the obstacle's displacement to its next position
    becomes 3 extra node features (non-obstacle nodes get the obstacles' mean displacement).  A handful of
    elementwise device ops -- plumbing, no kernel of its own."""
    from .nodetype import NodeType

    _require_device(graph.x, graph.y)
    world_pos = graph.x[:, world_pos_index_start:world_pos_index_end]
    other = graph.x[:, world_pos_index_end:]
    disp = graph.y[:, world_pos_index_start:world_pos_index_end] - world_pos
    node_type = graph.x[:, node_type_index - 3]  # the index is the one AFTER the 3 columns are inserted (:78-80)
    is_obs = (node_type == int(NodeType.OBSTACLE)).unsqueeze(1)
    mean_obs = (disp * is_obs).sum(dim=0) / is_obs.sum().clamp_min(1)
    disp = torch.where(is_obs, disp, mean_obs.unsqueeze(0).expand_as(disp))
    graph.x = torch.cat([world_pos, disp, other], dim=1).contiguous()
    return graph


def add_world_pos_features(graph, world_pos_index_start: int, world_pos_index_end: int):
    """``add_world_pos_features`` (preprocessing.py:143-176): relative WORLD position and its norm appended to
    the edge features (the same kernel as the mesh-space edge features)."""
    wp = graph.x[:, world_pos_index_start:world_pos_index_end].contiguous()
    extra = edge_features(wp, graph.edge_index)
    graph.edge_attr = extra if graph.edge_attr is None else torch.cat([graph.edge_attr, extra], dim=1)
    return graph


def build_preprocessing(noise_parameters=None, world_pos_parameters=None, add_edges_features: bool = True,
                        extra_node_features=None, extra_edge_features=None, seed: int = 0, khop: int = 1,
                        khop_cache: Optional[dict] = None, partitioning: Optional[dict] = None, new_edges_ratio: float = 0.0,
                        masking_ratio: Optional[float] = None):
    """Device-side ``build_preprocessing`` (preprocessing.py:380-444): the same transform ORDER as the
    reference -- extra node features, [obstacle next pos,] faces -> edges, [world edges,] edge features,
    noise inserted at position 1, extra edge features -- as one callable
    ``f(graph, step=0) -> graph`` over device tensors (``graph.face`` [K,F], ``graph.pos``, ``graph.x``,
    ``graph.y``).  Topology-only results (edge_index) can be cached by the caller across a trajectory.

    ``khop > 1`` appends the k-hop expansion (``khop_graph``) as the LAST step: the reference applies it after the whole
    preprocessing callable (dataset/h5_dataset.py:184-185).  With a dict as ``khop_cache`` and a graph that carries
    ``traj_index``, the k-hop ``edge_index`` (and, with edge features, ``edge_attr``) is kept per trajectory as device tensors
    and reused, as dataset/dataset.py:216-241 does on the host.  This mirrors a quirk of the reference: the cached
    ``edge_attr`` is that of the FIRST frame seen of a trajectory, also where later frames move the mesh.  ``khop == 1``
    leaves the callable as it is without the argument.

    ``partitioning`` (a dict with ``num_partitions`` or ``max_nodes_per_partition``, optionally ``method`` / ``seed`` for
    ``partition_node_ids``) makes every sample ONE part of the mesh (``apply_partition``), as ``--use_partitioning`` does in
    the reference: the callable becomes ``f(graph, step=0, part=None)``, ``part`` defaulting to ``step % P``.  The cut is the
    very last step, after k-hop (dataset/h5_dataset.py:232-233).  Node ids and per-part plans are kept per ``graph.traj_index``
    in ``f.partition_cache``, computed from the first processed frame seen of a trajectory, as the reference's cache is;
    later frames of a cached part cost one gather launch.  A trajectory of one part comes back untouched.  The parts carry no
    ``face`` and no cut edges (see ``apply_partition``).  ``None`` leaves the callable as it is without the argument.

    ``new_edges_ratio`` in ``(0, 1]`` appends the reference's random extra edges (``add_random_edges``; ``Dataset.
    _add_random_edges``) after k-hop and before the partition cut, the reference's order (dataset/h5_dataset.py:184-187,
    232-233): every sample gets ``round(E * ratio) // 2`` new node pairs in both directions, drawn with ``seed`` = this
    callable's ``seed`` and ``offset = step``, so a ``(seed, step)`` names its draw and consecutive steps differ.  With
    ``add_edges_features`` ``edge_attr`` is then recomputed on ALL edges as mesh-space Cartesian + Distance (earlier extra
    edge columns are dropped, as the reference's ``edge_attr = None`` -> Compose does); without, it is ``None``.  The k-hop
    cache keeps the un-augmented tensors.  The step does not synchronise with the host; at its start the deferred error flag
    of the previous step is looked at with one event query (``random_edges_check``).  With ``partitioning`` the node ids stay
    cached per trajectory but the per-part plans cannot be (they hold the cut edge list, and the edges now change every
    step): every sample is cut with ``subgraph`` as the reference does and PAYS ITS ONE HOST SYNCHRONISATION per sample;
    ``partition_cache[traj]["plans"]`` stays empty.  The default 0.0 leaves the callable as it is without the argument.

    ``masking_ratio`` in ``[0, 1]`` is the reference's ``get_dataset(..., masking_ratio=...)`` (dataset/h5_dataset.py:188,
    235-236): every sample becomes the pair ``(graph, selected_indices)``, the indices of the nodes that stay visible
    (``meshmask.get_masked_indexes``), drawn with ``seed`` = this callable's ``seed`` and ``offset = step`` AFTER k-hop and the
    random edges, the reference's order (h5_dataset.py:184-188).  The graph itself is not cut: ``meshmask.build_masked_graph``
    does that in the model.  The reference freezes a frame's draw while the frame sits in its LRU frame cache; the engine has no
    Dataset class and draws per ``(seed, step)``.  Together with ``partitioning`` it is a ``ValueError`` (the reference marks the
    combination "not working", h5_dataset.py:231).  ``None`` leaves the callable and its return value as they are without the
    argument."""
    if masking_ratio is not None:
        from .meshmask import check_masking_ratio

        check_masking_ratio(masking_ratio)
        if partitioning is not None:
            raise ValueError("masking_ratio and partitioning cannot be combined (masking a partitioned sample is not supported, as in "
                             "the reference)")
    if isinstance(new_edges_ratio, bool) or not isinstance(new_edges_ratio, (int, float)) or not 0.0 <= new_edges_ratio <= 1.0:
        raise ValueError(f"new_edges_ratio must be a number in [0, 1], got {new_edges_ratio!r}")
    if partitioning is not None:
        partitioning = dict(partitioning)
        unknown = set(partitioning) - {"num_partitions", "max_nodes_per_partition", "method", "seed"}
        if unknown:
            raise ValueError(f"partitioning: unknown keys {sorted(unknown)}")
        num_partitions_for(1, partitioning.get("num_partitions"), partitioning.get("max_nodes_per_partition"))   # validates
    if isinstance(khop, bool) or not isinstance(khop, int) or khop < 1:
        raise ValueError(f"khop must be an integer >= 1, got {khop!r}")
    steps = []
    if extra_node_features is not None:
        steps += list(extra_node_features) if isinstance(extra_node_features, (list, tuple)) else [extra_node_features]

    def face_to_edge(g, step):
        if g.edge_index is None:
            g.edge_index = faces_to_edges(g.face, g.x.shape[0])
        return g

    def feats(g, step):
        g.edge_attr = edge_features(g.pos, g.edge_index)
        return g

    if world_pos_parameters is not None:
        w = world_pos_parameters
        steps.append(lambda g, step: add_obstacles_next_pos(g, w["world_pos_index_start"], w["world_pos_index_end"], w["node_type_index"]))
        steps.append(face_to_edge)

        def world(g, step):
            g.edge_index = add_world_edges(g.x, g.edge_index, w["world_pos_index_start"], w["world_pos_index_end"], w["node_type_index"],
                                           radius=w.get("radius", 0.03))
            return g
        steps.append(world)
        steps.append(feats)   # (the reference's pipeline stops here: add_world_pos_features stays a stand-alone transform, :401-420)
    else:
        steps.append(face_to_edge)
        if add_edges_features:
            steps.append(feats)
    if noise_parameters is not None:
        p = noise_parameters
        steps.insert(1, lambda g, step: add_noise(g, p["noise_index_start"], p["noise_index_end"], p["noise_scale"], p["node_type_index"],
                                                  seed=seed, offset=step))
    if extra_edge_features is not None:
        steps += list(extra_edge_features) if isinstance(extra_edge_features, (list, tuple)) else [extra_edge_features]
    if khop > 1:
        def k_hop(g, step):
            traj = g.traj_index if khop_cache is not None else None
            if traj is not None:
                traj = int(traj)
                if traj in khop_cache:
                    g.edge_index, attr = khop_cache[traj]
                    if add_edges_features:
                        g.edge_attr = attr
                    return g
            g = khop_graph(g, khop, add_edge_features=add_edges_features)
            if traj is not None:
                khop_cache[traj] = (g.edge_index, g.edge_attr)
            return g
        steps.append(k_hop)
    if new_edges_ratio > 0:
        def random_edges(g, step):
            random_edges_check(g.edge_index.device)
            g.edge_index = add_random_edges(g.edge_index, _graph_num_nodes(g), new_edges_ratio, seed=seed, offset=step)
            g.edge_attr = edge_features(g.pos, g.edge_index) if add_edges_features else None
            return g
        steps.append(random_edges)

    def run(graph, step: int = 0):
        import inspect
        for f in steps:
            graph = f(graph, step) if len(inspect.signature(f).parameters) >= 2 else f(graph)
        return graph

    if masking_ratio is not None:
        def run_masked(graph, step: int = 0):
            from .meshmask import get_masked_indexes

            graph = run(graph, step)
            return graph, get_masked_indexes(graph, masking_ratio, seed=seed, offset=step)

        run_masked.masking_ratio = masking_ratio
        return run_masked
    if partitioning is None:
        return run

    cache: dict = {}

    def run_part(graph, step: int = 0, part: Optional[int] = None):
        graph = run(graph, step)
        P = num_partitions_for(_graph_num_nodes(graph), partitioning.get("num_partitions"), partitioning.get("max_nodes_per_partition"))
        if P == 1:
            return graph
        p = int(step) % P if part is None else int(part)
        if not 0 <= p < P:
            raise ValueError(f"part must be in [0, {P}), got {p}")
        traj = graph.traj_index
        entry = cache.get(int(traj)) if traj is not None else None
        if entry is None:
            entry = {"node_ids": partition_node_ids(graph, P, method=partitioning.get("method", "auto"), seed=partitioning.get("seed", 0)),
                     "plans": {}}
            if traj is not None:
                cache[int(traj)] = entry
        if new_edges_ratio > 0:   # the edges are this sample's own: nothing of the cut can be kept
            return apply_partition(graph, entry["node_ids"][p])
        plan = entry["plans"].get(p)
        if plan is None:
            plan = entry["plans"][p] = partition_plan(graph, entry["node_ids"][p])
        return apply_partition(graph, None, plan=plan)

    run_part.partition_cache = cache
    run_part.partitioning = partitioning
    return run_part


# ------------------------------------------------------------------------------------------------ k nearest neighbours
def _host_ptr(ptr, n: int, what: str):
    """segment offsets given on the host (list / tuple / CPU tensor) as a checked list of ints"""
    p = [int(v) for v in (ptr.tolist() if torch.is_tensor(ptr) else ptr)]
    if len(p) < 2 or p[0] != 0 or p[-1] != n or any(b < a for a, b in zip(p, p[1:])):
        raise ValueError(f"{what} must be non-decreasing offsets from 0 to the number of points ({n}), got {p[:8]}{'...' if len(p) > 8 else ''}")
    return p


def _knn_segments(nx: int, ny: int, batch_x, batch_y, ptr_x, ptr_y, dev):
    """(ptr_x, ptr_y, nseg, host_x, host_y): the two offset vectors as device int64 [nseg + 1]; host_* are the same offsets as
    lists where the host knows them (given as ``ptr_*``, or a side without ``batch`` and ``ptr``: all of it is segment 0), else
    None.  Synchronises once -- to read the number of segments -- only when no ``ptr_*`` is given and a ``batch_*`` is."""
    sides = []
    for n, batch, ptr, what in ((nx, batch_x, ptr_x, "ptr_x"), (ny, batch_y, ptr_y, "ptr_y")):
        if ptr is not None and torch.is_tensor(ptr) and ptr.is_cuda:
            sides.append(("dev", ptr.to(torch.int64).contiguous()))
        elif ptr is not None:
            sides.append(("host", _host_ptr(ptr, n, what)))
        elif batch is not None and n > 0:
            sides.append(("batch", batch))
        else:
            sides.append(("none", n))
    lens = {(s[1].numel() if s[0] == "dev" else len(s[1])) - 1 for s in sides if s[0] in ("dev", "host")}
    if len(lens) > 1:
        raise ValueError("ptr_x and ptr_y must describe the same number of segments")
    if lens:
        nseg = lens.pop()
    elif any(s[0] == "batch" for s in sides):
        nseg = int(torch.stack([s[1][-1] for s in sides if s[0] == "batch"]).max()) + 1   # the one synchronisation
    else:
        nseg = 1
    if nseg < 1:
        raise ValueError("at least one segment is needed")
    dev_ptr, host = [], []
    for kind, v in sides:
        if kind == "none":
            kind, v = "host", [0] + [v] * nseg
        if kind == "host":
            dev_ptr.append(torch.tensor(v, dtype=torch.int64, device=dev))
            host.append(v)
        elif kind == "dev":
            dev_ptr.append(v)
            host.append(None)
        else:
            b = v.to(torch.int64).contiguous()
            dev_ptr.append(torch.searchsorted(b, torch.arange(nseg + 1, dtype=torch.int64, device=dev)))
            host.append(None)
    return dev_ptr[0], dev_ptr[1], nseg, host[0], host[1]


def _knn_search(pos_x: torch.Tensor, pos_y: torch.Tensor, k: int, ptr_x: torch.Tensor, ptr_y: torch.Tensor, nseg: int,
                exclude_self: bool = False):
    """(idx [ny, k] int64, d2 [ny, k] fp32) of ``mgn_knn_search`` (include/mgn_hip.h): nearest first by (d2, index), ``-1`` /
    ``+inf`` where the segment runs out of references.  ``ptr_*`` are device offsets.  Never synchronises."""
    _require_device(pos_x, pos_y, ptr_x, ptr_y)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    L = _capi.lib()
    if k > L.mgn_knn_max_k():
        raise ValueError(f"k must not exceed {L.mgn_knn_max_k()}, got {k}")
    if pos_x.dim() != 2 or pos_y.dim() != 2 or pos_x.shape[1] != pos_y.shape[1] or pos_x.shape[1] not in (2, 3):
        raise ValueError("positions must be [n, 2] or [n, 3], the same width on both sides")
    dev = pos_y.device
    x, y = pos_x.detach().to(torch.float32).contiguous(), pos_y.detach().to(torch.float32).contiguous()
    nx, ny, D = int(x.shape[0]), int(y.shape[0]), int(x.shape[1])
    idx = torch.empty(ny, k, dtype=torch.int64, device=dev)
    d2 = torch.empty(ny, k, dtype=torch.float32, device=dev)
    call("mgn_knn_search", dev, _ptr(x), nx, _ptr(y), ny, D, k, _ptr(ptr_x), _ptr(ptr_y), nseg, 1 if exclude_self else 0, _ptr(idx), _ptr(d2))
    return idx, d2


def _always_k(host_x, host_y, k: int, exclude_self: bool) -> bool:
    """True where the host can tell that no slot stays empty: every segment with a query holds k admissible references"""
    if host_x is None or host_y is None:
        return False
    need = k + (1 if exclude_self else 0)
    return all(host_x[s + 1] - host_x[s] >= need for s in range(len(host_y) - 1) if host_y[s + 1] > host_y[s])


def knn(pos_x: torch.Tensor, pos_y: torch.Tensor, k: int, batch_x: Optional[torch.Tensor] = None, batch_y: Optional[torch.Tensor] = None,
        ptr_x=None, ptr_y=None) -> torch.Tensor:
    """``torch_cluster.knn``: for every point of ``pos_y`` its ``k`` nearest points of ``pos_x`` within the same graph of the
    batch, as ``assign_index [2, M]`` int64 with rows (query, reference), grouped by query, nearest first; ties in the squared
    fp32 distance go to the lower reference index.  A graph with fewer than ``k`` references gives fewer entries.  Exact
    brute force on the device (csrc/mgn_knn.hip), 2-D or 3-D, ``k <= 32``; ``batch_*`` must be sorted.

    Synchronisation: with ``ptr_x`` / ``ptr_y`` (``nseg + 1`` offsets as a list or a CPU tensor) or with no batch at all the
    search never synchronises, and the result is returned without one where the offsets show that every graph holds ``k``
    references.  With only ``batch_*`` the number of graphs is read once from the device (one synchronisation), and dropping
    the empty slots sizes the result on the device (torch's boolean mask: it synchronises)."""
    _require_device(pos_x, pos_y, batch_x, batch_y)
    dev = pos_y.device
    px, py, nseg, hx, hy = _knn_segments(int(pos_x.shape[0]), int(pos_y.shape[0]), batch_x, batch_y, ptr_x, ptr_y, dev)
    idx, _ = _knn_search(pos_x, pos_y, k, px, py, nseg)
    q = torch.arange(idx.shape[0], dtype=torch.int64, device=dev).repeat_interleave(k)
    r = idx.reshape(-1)
    if not _always_k(hx, hy, k, False):
        keep = r >= 0
        q, r = q[keep], r[keep]
    return torch.stack([q, r])


def knn_graph(pos: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None, loop: bool = False, flow: str = "source_to_target",
              force_undirected: bool = False, ptr=None) -> torch.Tensor:
    """``torch_cluster.knn_graph`` / PyG ``KNNGraph``: edges from every node's ``k`` nearest nodes of its graph to the node,
    ``[2, E]`` int64 with rows (neighbour, centre) (``flow="target_to_source"``: (centre, neighbour)), grouped by centre,
    nearest first.  Without ``loop`` a node is never its own neighbour: the search leaves out the node ITSELF (by index), so
    coincident nodes are neighbours of each other and cost no real neighbour -- upstream searches ``k + 1`` and drops whichever
    entry is the node.  ``force_undirected`` (``KNNGraph(k, force_undirected=True)``): both directions of every edge, each pair
    once, sorted by (row 0, row 1).  ``ptr`` (host offsets) instead of ``batch`` avoids the synchronisation that reads the
    number of graphs; ``force_undirected`` and graphs smaller than ``k`` size their result on the device and synchronise."""
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"flow must be 'source_to_target' or 'target_to_source', got {flow!r}")
    _require_device(pos, batch)
    dev = pos.device
    N = int(pos.shape[0])
    px, py, nseg, hx, hy = _knn_segments(N, N, batch, batch, ptr, ptr, dev)
    idx, _ = _knn_search(pos, pos, k, px, py, nseg, exclude_self=not loop)
    ctr = torch.arange(N, dtype=torch.int64, device=dev).repeat_interleave(k)
    nbr = idx.reshape(-1)
    if not _always_k(hx, hy, k, not loop):
        keep = nbr >= 0
        ctr, nbr = ctr[keep], nbr[keep]
    row, col = (nbr, ctr) if flow == "source_to_target" else (ctr, nbr)
    if force_undirected:   # to_undirected: both directions, coalesced
        key = torch.unique(torch.cat([row * N + col, col * N + row]))   # sorted
        return torch.stack([torch.div(key, N, rounding_mode="floor"), key % N]) if N > 0 else torch.stack([row, col])
    return torch.stack([row, col])


def min_distance_to_type(graph, target_type, node_types: torch.Tensor) -> torch.Tensor:
    """``compute_min_distance_to_type`` of the reference (dataset/preprocessing.py:241-274): for every node the distance to the
    nearest node whose entry of ``node_types`` equals ``target_type``, ``[N]`` fp32, over the whole graph (``batch`` is
    ignored, as upstream).  The square root of the ``k = 1`` search: no ``[N, M, 3]`` intermediate.  A type without a node is a
    ``ValueError``.  Selecting the nodes of the type sizes a tensor on the device: one synchronisation."""
    pos = graph.pos
    _require_device(pos, node_types)
    target = pos[node_types.reshape(-1) == int(target_type)]
    if target.shape[0] == 0:
        raise ValueError(f"no node of type {target_type!r} in the graph")
    dev = pos.device
    px = torch.tensor([0, int(target.shape[0])], dtype=torch.int64, device=dev)
    py = torch.tensor([0, int(pos.shape[0])], dtype=torch.int64, device=dev)
    _, d2 = _knn_search(target, pos, 1, px, py, 1)
    return torch.sqrt(d2[:, 0])
