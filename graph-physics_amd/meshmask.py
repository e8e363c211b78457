"""Masked-mesh training (graphphysics/utils/meshmask.py:9-118 and ``get_masked_indexes`` of utils/torch_graph.py:310-327): cut a
sample down to its visible nodes, run the encoder on that, and rebuild the full latent mesh with trained ``[MASK]`` tokens.
Names, argument order and return values are the reference's.

On device tensors the work runs on the engine's kernels (csrc/mgn_subgraph.hip):

  * ``filter_edges`` is ``preprocess.subgraph``: the relabel table, the edge flags and the ordered compaction; one host
    synchronisation, for the number of kept edges;
  * ``build_masked_graph`` adds the row gathers of ``x``, ``pos`` and ``edge_attr`` as ONE ``mgn_gather_rows_batch`` launch;
  * ``reconstruct_graph`` is one autograd node whose forward is ONE ``mgn_gather_rows_batch`` launch: a row of ``dst`` whose index
    is outside the source is left as it is, so two jobs with one ``dst`` and complementary indices merge two sources row by row --
    the latent rows by the inverse of ``selected_indexes`` (-1 where masked), the ``[MASK]`` rows from a one-row source (the node
    token) or a full-height one (the edge encoder's output plus the edge token).  Its backward is one launch of the same kernel
    for the row gradients; the node token's gradient is a masked column sum in torch ops.

CPU tensors take the reference's torch statements."""
from __future__ import annotations

from typing import Optional

import torch

from . import _capi
from ._launch import call

_MASK64 = 2 ** 64 - 1


def masked_count(num_nodes: int, masking_ratio: float) -> int:
    """number of nodes that stay visible: the reference's ``int((1 - masking_ratio) * n)``, in Python float arithmetic"""
    nodes_to_keep = 1 - masking_ratio
    return int(nodes_to_keep * num_nodes)


def check_masking_ratio(masking_ratio, what: str = "masking_ratio") -> float:
    if isinstance(masking_ratio, bool) or not isinstance(masking_ratio, (int, float)) or not 0.0 <= masking_ratio <= 1.0:
        raise ValueError(f"{what} must be a number in [0, 1], got {masking_ratio!r}")
    return masking_ratio


def mask_seed(seed: int, offset: int) -> int:
    """the generator seed of the draw ``(seed, offset)``: ``(seed * 0x9E3779B97F4A7C15 + offset + 0x4D41534B) mod 2^63`` with
    ``seed`` taken mod 2^64 and ``offset`` mod 2^32 ("MASK" in ASCII keeps the stream apart from the random-edge sampler's)"""
    return ((int(seed) & _MASK64) * 0x9E3779B97F4A7C15 + (int(offset) & 0xFFFFFFFF) + 0x4D41534B) % (2 ** 63)


def get_masked_indexes(graph, masking_ratio: float = 0.15, seed: int = 0, offset: int = 0) -> torch.Tensor:
    """``get_masked_indexes`` of the reference (utils/torch_graph.py:310-327): the indices of the nodes to KEEP, int64 ``[k]`` on
    ``graph.x``'s device, ``k = int((1 - masking_ratio) * n)``: the first ``k`` entries of a uniformly random permutation of
    ``0..n-1``, in permutation order (not sorted).  The reference draws from torch's global CPU generator; here the draw is
    ``torch.randperm`` on the tensor's device with a generator seeded by ``mask_seed(seed, offset)`` -- pass the training step as
    ``offset`` -- so the same ``(seed, offset)`` gives the same draw on the same software stack and consecutive offsets differ.
    No host synchronisation."""
    check_masking_ratio(masking_ratio)
    n = int(graph.x.shape[0])
    dev = graph.x.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(mask_seed(seed, offset))
    return torch.randperm(n, generator=gen, device=dev)[:masked_count(n, masking_ratio)]


# ----------------------------------------------------------------------------------------- filter_edges / build_masked_graph
def _filter_edges_torch(edge_index, node_index, edge_attr, num_nodes):
    """the reference's statements (meshmask.py:22-37)"""
    cluster_index = torch.arange(node_index.size(0), device=node_index.device)
    mask = node_index.new_full((num_nodes,), -1)
    mask[node_index] = cluster_index
    senders, receivers = mask[edge_index[0]], mask[edge_index[1]]
    mask = (senders >= 0) & (receivers >= 0)
    senders, receivers = senders[mask], receivers[mask]
    if edge_attr is not None:
        edge_attr = edge_attr[mask]
    return torch.stack([senders, receivers], dim=0), edge_attr, mask


def filter_edges(edge_index: torch.Tensor, node_index: torch.Tensor, edge_attr: Optional[torch.Tensor] = None,
                 num_nodes: Optional[int] = None):
    """``filter_edges`` of the reference: ``(edge_index', edge_attr', mask)`` -- the edges with both ends in ``node_index``, in
    input order, their ends relabelled to the position in ``node_index`` (which need not be sorted), their ``edge_attr`` rows, and
    the bool ``[E]`` mask of kept edges.  ``num_nodes=None`` means ``edge_index.max() + 1`` as in the reference (one host
    synchronisation); the keyword is this project's extension, so that a caller who knows ``N`` skips it.  Device tensors go
    through ``preprocess.subgraph`` (one synchronisation for the edge count; an entry outside ``[0, num_nodes)`` is an
    ``IndexError``, a node listed twice a ``ValueError``); CPU tensors take the reference's torch statements."""
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1 if edge_index.numel() else 0
    if not edge_index.is_cuda:
        return _filter_edges_torch(edge_index.long(), node_index.to(edge_index.device).long(), edge_attr, int(num_nodes))
    from .preprocess import subgraph

    return subgraph(node_index.to(edge_index.device), edge_index, edge_attr, num_nodes=int(num_nodes), return_edge_mask=True)


def _no_grad_rows(what: str, *tensors):
    for t in tensors:
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{what}: the row gather of a tensor that requires grad is not differentiable here (masking applies to a "
                             "sample's input tensors)")


def build_masked_graph(masked_graph, selected_indexes: torch.Tensor):
    """``build_masked_graph`` of the reference: ``(masked_graph, edges_mask)``; the argument is changed in place, as the reference
    does -- ``x`` and ``pos`` (where present) become the rows ``selected_indexes``, ``edge_index`` / ``edge_attr`` (where present)
    the filtered edges; ``y`` and everything else stay as they are.  On device tensors the three row gathers are one
    ``mgn_gather_rows_batch`` launch and the node count comes from ``x``, so the call synchronises once (the edge count)."""
    g = masked_graph
    if not g.x.is_cuda:
        ei, attr, mask = _filter_edges_torch(g.edge_index.long(), selected_indexes.long(), g.edge_attr,
                                             int(g.edge_index.max()) + 1 if g.edge_index.numel() else 0)
        g.edge_index = ei
        g.x = g.x[selected_indexes]
        if g.pos is not None:
            g.pos = g.pos[selected_indexes]
        if attr is not None:
            g.edge_attr = attr
        return g, mask
    from .preprocess import _subgraph_edges, gather_rows_batch

    _no_grad_rows("build_masked_graph", g.x, g.pos, g.edge_attr)
    sel = selected_indexes.to(g.x.device)
    ei, edge_pos, mask = _subgraph_edges(sel, g.edge_index, int(g.x.shape[0]), want_mask=True)
    x, pos, attr = gather_rows_batch([g.x, g.pos, g.edge_attr], [sel, sel, edge_pos])
    g.edge_index, g.x = ei, x
    if pos is not None:
        g.pos = pos
    if attr is not None:
        g.edge_attr = attr
    return g, mask


# ----------------------------------------------------------------------------------------- reconstruct_graph
def _launch_row_jobs(dev, jobs):
    """ONE ``mgn_gather_rows_batch`` launch: ``dst[r] = src[idx[r]]`` where ``0 <= idx[r] < src rows`` for every
    ``(src [S, W], idx [R] int64, dst [R, W])`` of contiguous fp32 rows; a source without rows takes no job"""
    live = [(s, i, d) for s, i, d in jobs if d.numel() and s.shape[0]]
    if len(live) > _capi.MAX_GATHER_JOBS:
        raise ValueError(f"at most {_capi.MAX_GATHER_JOBS} jobs per launch")
    if not live:
        return
    arr = (_capi.GatherJob * len(live))()
    for j, (s, i, d) in zip(arr, live):
        w = int(d.shape[1])
        j.src, j.ld_src, j.width, j.idx, j.rows = s.data_ptr(), w, w, i.data_ptr(), int(d.shape[0])
        j.dst, j.ld_dst, j.src_rows = d.data_ptr(), w, int(s.shape[0])
    call("mgn_gather_rows_batch", dev, len(live), arr)


class _Side:
    """index tensors of one side (nodes or edges) of a reconstruction, all int64 on the device and built without a host
    synchronisation: ``inv [R]`` = row of the latent source (-1 on a masked row), ``other [R]`` = row of the [MASK] source on a
    masked row (0 for a one-row source, ``r`` for a full-height one; -1 on a kept row), ``pos [K]`` = the row each latent row goes to"""

    def __init__(self, inv: torch.Tensor, pos: torch.Tensor, full_height: bool):
        rows = int(inv.shape[0])
        masked = inv < 0
        r = torch.arange(rows, device=inv.device) if full_height else torch.zeros(rows, dtype=torch.int64, device=inv.device)
        self.inv, self.pos, self.masked = inv, pos, masked
        self.other = torch.where(masked, r, torch.full_like(r, -1))
        self.kept0 = torch.where(masked, torch.full_like(r, -1), torch.zeros_like(r))   # row 0 of a zero source on the kept rows


class _ReconstructFn(torch.autograd.Function):
    """``(x, edge_attr)`` of the reconstructed mesh from ``(latent x [k, f], node token [1, f], latent edge_attr [k_e, fe] or None,
    encoder output + edge token [E, fe] or None)``"""

    @staticmethod
    def forward(ctx, lat_x, token, lat_e, fill_e, node: _Side, edge: Optional[_Side]):
        dev = lat_x.device
        n, f = int(node.inv.shape[0]), int(lat_x.shape[1])
        x = torch.empty(n, f, dtype=torch.float32, device=dev)
        jobs = [(lat_x, node.inv, x), (token, node.other, x)]
        e = None
        if edge is not None:
            e = torch.empty_like(fill_e)
            jobs += [(lat_e, edge.inv, e), (fill_e, edge.other, e)]
        _launch_row_jobs(dev, jobs)
        ctx.node, ctx.edge = node, edge
        ctx.k, ctx.ke = int(lat_x.shape[0]), int(lat_e.shape[0]) if edge is not None else 0
        if edge is None:
            return x
        return x, e

    @staticmethod
    def backward(ctx, g_x, g_e=None):
        node, edge = ctx.node, ctx.edge
        need = ctx.needs_input_grad
        dev = g_x.device
        g_x = g_x.float().contiguous()
        jobs = []
        d_lat_x = d_token = d_lat_e = d_fill_e = None
        if need[0]:
            d_lat_x = torch.empty(ctx.k, g_x.shape[1], dtype=torch.float32, device=dev)
            jobs.append((g_x, node.pos, d_lat_x))
        if edge is not None and g_e is not None:
            g_e = g_e.float().contiguous()
            if need[2]:
                d_lat_e = torch.empty(ctx.ke, g_e.shape[1], dtype=torch.float32, device=dev)
                jobs.append((g_e, edge.pos, d_lat_e))
            if need[3]:   # the incoming rows where masked, a zero row where kept
                d_fill_e = torch.empty_like(g_e)
                zero = torch.zeros(1, g_e.shape[1], dtype=torch.float32, device=dev)
                jobs += [(g_e, edge.other, d_fill_e), (zero, edge.kept0, d_fill_e)]
        _launch_row_jobs(dev, jobs)
        if need[1]:   # column sum of the incoming gradient over the masked rows (torch ops)
            d_token = torch.where(node.masked.unsqueeze(1), g_x, torch.zeros_like(g_x)).sum(0, keepdim=True)
        return d_lat_x, d_token, d_lat_e, d_fill_e, None, None


def _check_selection(sel: torch.Tensor, n: int):
    """duplicates / entries outside [0, n) in ``selected_indexes``, found on the device by ``mgn_subgraph_count`` (codes 5 / 3) on
    an empty edge list; the one host synchronisation of ``reconstruct_graph``"""
    from .preprocess import _subgraph_count

    nbytes = _capi.lib().mgn_subgraph_workspace_bytes(n, 0)
    if nbytes == 0:
        raise ValueError(f"reconstruct_graph: {n} nodes are outside what the kernels index")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=sel.device)
    empty = torch.empty(2, 0, dtype=torch.int64, device=sel.device)
    try:
        _subgraph_count(sel, empty, n, ws)
    except ValueError as e:
        raise ValueError("reconstruct_graph: selected_indexes lists a node twice") from e


def _f32_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise ValueError(f"reconstruct_graph: {what} must be float32 on the device, got {t.dtype}")
    return t.contiguous()


def reconstruct_graph(graph, latent_masked_graph, selected_indexes: torch.Tensor, node_mask_token: torch.Tensor,
                      edges_mask: torch.Tensor, edge_encoder=None, edge_mask_token: Optional[torch.Tensor] = None):
    """``reconstruct_graph`` of the reference: a clone of ``graph`` with ``x[n] = latent_masked_graph.x[i]`` where
    ``selected_indexes[i] == n`` and ``node_mask_token`` elsewhere, and, when ``graph.edge_attr`` is not None,
    ``edge_attr[e] = latent_masked_graph.edge_attr[rank of e among the kept edges]`` where ``edges_mask[e]`` and
    ``edge_encoder(graph.edge_attr)[e] + edge_mask_token`` elsewhere.  Differentiable in both tokens, both latent tensors and
    the encoder's parameters.  The widths of the token, ``latent_masked_graph.x`` and ``graph.x`` must agree (``ValueError``
    before any launch).  On device tensors a node listed twice in ``selected_indexes`` is a ``ValueError`` and an entry outside
    ``[0, n)`` an ``IndexError`` (one host synchronisation); see the module text for the launches.  CPU tensors take the
    reference's statements."""
    n, f = graph.x.shape
    lat_x = latent_masked_graph.x
    k = int(selected_indexes.shape[0])
    if node_mask_token.numel() != f or lat_x.dim() != 2 or int(lat_x.shape[1]) != f:
        raise ValueError(f"reconstruct_graph: graph.x has {f} columns, latent_masked_graph.x {tuple(lat_x.shape)} and the node token "
                         f"{node_mask_token.numel()} entries: the widths must agree")
    if int(lat_x.shape[0]) != k:
        raise ValueError(f"reconstruct_graph: {k} selected indexes for {int(lat_x.shape[0])} latent rows")
    with_edges = graph.edge_attr is not None
    if with_edges and (edge_encoder is None or edge_mask_token is None):
        raise ValueError("reconstruct_graph: a graph with edge_attr needs edge_encoder and edge_mask_token")
    latent_graph = graph.clone()
    if not graph.x.is_cuda:
        features = torch.zeros(n, f, dtype=lat_x.dtype) + node_mask_token.expand(n, -1)
        features[selected_indexes] = lat_x
        latent_graph.x = features
        if with_edges:
            attr = edge_encoder(latent_graph.edge_attr)
            attr = attr + edge_mask_token.expand(attr.shape[0], -1)
            attr[edges_mask] = latent_masked_graph.edge_attr
            latent_graph.edge_attr = attr
        return latent_graph
    dev = graph.x.device
    n = int(n)
    sel = selected_indexes.to(device=dev, dtype=torch.int64).contiguous()
    fill_e = lat_e = None
    if with_edges:
        fill_e = edge_encoder(graph.edge_attr)
        lat_e = latent_masked_graph.edge_attr
        E, fe = int(fill_e.shape[0]), int(fill_e.shape[1])
        if edge_mask_token.numel() != fe or lat_e.dim() != 2 or int(lat_e.shape[1]) != fe:
            raise ValueError(f"reconstruct_graph: the edge encoder gives {fe} columns, latent_masked_graph.edge_attr {tuple(lat_e.shape)} "
                             f"and the edge token {edge_mask_token.numel()} entries: the widths must agree")
        if edges_mask.dtype != torch.bool or edges_mask.shape != (E,):
            raise ValueError("reconstruct_graph: edges_mask must be a bool tensor of one entry per edge")
        fill_e = _f32_rows(fill_e + edge_mask_token.reshape(1, fe), "the edge encoder's output")
        lat_e = _f32_rows(lat_e, "latent_masked_graph.edge_attr")
    lat_x = _f32_rows(lat_x, "latent_masked_graph.x")
    token = _f32_rows(node_mask_token.reshape(1, int(f)), "node_mask_token")
    _check_selection(sel, n)
    inv = torch.full((n,), -1, dtype=torch.int64, device=dev)
    inv[sel] = torch.arange(k, device=dev)
    node = _Side(inv, sel, full_height=False)
    edge = None
    if with_edges:
        ke = int(lat_e.shape[0])
        mask = edges_mask.to(dev)
        rank = torch.cumsum(mask, 0) - 1
        kept = mask & (rank < ke)   # (a mask of more edges than the latent graph has rows: the surplus counts as masked)
        # position of every kept edge, without nonzero()'s synchronisation: slot ke swallows the masked edges
        pos = torch.zeros(ke + 1, dtype=torch.int64, device=dev)
        pos[torch.where(kept, rank, torch.full_like(rank, ke))] = torch.arange(E, device=dev)
        edge = _Side(torch.where(kept, rank, torch.full_like(rank, -1)), pos[:ke].contiguous(), full_height=True)
        latent_graph.x, latent_graph.edge_attr = _ReconstructFn.apply(lat_x, token, lat_e, fill_e, node, edge)
    else:
        latent_graph.x = _ReconstructFn.apply(lat_x, token, None, None, node, None)
    return latent_graph
