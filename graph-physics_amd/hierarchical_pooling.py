"""Multigrid pooling of the reference (graphphysics/models/hierarchical_pooling.py; README "Pooling"): ``DownSampler`` selects
the highest-scoring ``ceil(ratio * n)`` nodes of every graph and re-meshes them with a symmetrised 6-nearest-neighbour graph,
``UpSampler`` carries coarse features back to the fine nodes by inverse-squared-distance interpolation over the ``k`` nearest
coarse nodes.  Upstream builds both on PyG (``SelectTopK``, ``KNNGraph``, ``knn_interpolate``) and ``torch_cluster.knn``; here
the search and the interpolation are HIP kernels (csrc/mgn_knn.hip), the same names and constructor signatures stay.  CUDA
tensors only: CPU tensors raise ``RuntimeError``."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dense, ops
from ._launch import call, ptr as _ptr
from .mesh import Graph
from .ops import _require_device
from .preprocess import _knn_search, _knn_segments, knn_graph

#: input widths of one ``mgn_linear_fwd`` launch (csrc/mgn_dense.hip).  The backward runs the same launch on dZ [M, d_out], so
#: the output width has to be one of them too.
DENSE_IN_WIDTHS = (16, 32, 48, 64, 96, 128, 192, 256, 384)


def _engine_linear_ok(d_in: int, d_out: int) -> bool:
    return d_in in DENSE_IN_WIDTHS and d_out in DENSE_IN_WIDTHS


def _linear(x: torch.Tensor, lin: nn.Linear) -> torch.Tensor:
    """``lin(x)`` on the engine's fused Linear where its width rules allow (both widths in ``DENSE_IN_WIDTHS``), otherwise
    ``F.linear``"""
    if x.shape[0] > 0 and _engine_linear_ok(lin.in_features, lin.out_features):
        return dense.dense(x, lin.weight, lin.bias)
    return F.linear(x, lin.weight, lin.bias)


class KnnInterpolateFn(torch.autograd.Function):
    """out[y] = sum_j a[y, j] x[idx[y, j]] with the normalised inverse-squared-distance weights of ``mgn_knn_interp_fwd``; the
    backward is the segment sum ``mgn_knn_interp_bwd`` over the CSR of the assignment keyed by coarse node (``ops.csr_build``:
    slots in ascending order, no atomics).  ``idx`` / ``d2`` are constants of the geometry: no gradient."""

    @staticmethod
    def forward(ctx, x, idx, d2):
        _require_device(x, idx, d2)
        x = ops._f32c(x)
        nx, Fw = int(x.shape[0]), int(x.shape[1])
        ny, k = int(idx.shape[0]), int(idx.shape[1])
        if Fw < 1:
            raise ValueError("knn_interpolate: x needs at least one column")
        a = torch.empty(ny, k, dtype=torch.float32, device=x.device)
        out = torch.empty(ny, Fw, dtype=torch.float32, device=x.device)
        call("mgn_knn_interp_fwd", x.device, _ptr(x), nx, Fw, _ptr(idx), _ptr(d2), ny, k, _ptr(a), _ptr(out))
        ctx.save_for_backward(idx, a)
        ctx.shape = (nx, Fw)
        return out

    @staticmethod
    def backward(ctx, dy):
        idx, a = ctx.saved_tensors
        nx, Fw = ctx.shape
        ny, k = int(idx.shape[0]), int(idx.shape[1])
        dy = ops._f32c(dy)
        dev = dy.device
        # empty slots (-1) go to a bucket behind the last coarse node, which the kernel never reads
        key = torch.where(idx < 0, torch.full_like(idx, nx), idx).reshape(-1)
        rowptr, perm = ops.csr_build(key, nx + 1)
        dx = torch.empty(nx, Fw, dtype=torch.float32, device=dev)
        call("mgn_knn_interp_bwd", dev, _ptr(dy), _ptr(a), _ptr(rowptr), _ptr(perm), nx, ny, k, Fw, _ptr(dx))
        return dx, None, None


def knn_interpolate(x: torch.Tensor, pos_x: torch.Tensor, pos_y: torch.Tensor, batch_x: Optional[torch.Tensor] = None,
                    batch_y: Optional[torch.Tensor] = None, k: int = 3, ptr_x=None, ptr_y=None) -> torch.Tensor:
    """``torch_geometric.nn.unpool.knn_interpolate`` (2.6.1): ``y[i] = sum_j w_j x[j] / sum_j w_j`` over the ``k`` nearest points
    ``j`` of ``pos_x`` to ``pos_y[i]`` within the same graph, ``w_j = 1 / max(d2_j, 1e-16)``.  ``[ny, F]`` fp32, any ``F``.
    The gradient reaches ``x`` only: the positions take none (upstream searches under ``no_grad`` too, but lets the weights
    carry a gradient to the positions; here they are constants of the geometry).  The search synchronises once when only
    ``batch_*`` is given (to read the number of graphs) and never with ``ptr_x`` / ``ptr_y`` (host offsets) or without a
    batch; the backward builds its CSR with ``ops.csr_build``, which synchronises once."""
    _require_device(x, pos_x, pos_y, batch_x, batch_y)
    if x.dim() != 2 or x.shape[0] != pos_x.shape[0]:
        raise ValueError("x must be [number of pos_x points, F]")
    with torch.no_grad():
        px, py, nseg, _, _ = _knn_segments(int(pos_x.shape[0]), int(pos_y.shape[0]), batch_x, batch_y, ptr_x, ptr_y, pos_y.device)
        idx, d2 = _knn_search(pos_x, pos_y, k, px, py, nseg)
    return KnnInterpolateFn.apply(x, idx, d2)


class UpSampler(nn.Module):
    """coarse features to the fine nodes: ``lin(knn_interpolate(x_coarse, pos_coarse, pos_fine, ..., k))``"""

    def __init__(self, d_in: int, d_out: int, k: int = 6):
        super().__init__()
        self.k = k
        self.lin = nn.Linear(d_in, d_out)

    def forward(self, x_coarse: torch.Tensor, pos_coarse: torch.Tensor, pos_fine: torch.Tensor,
                batch_coarse: Optional[torch.Tensor] = None, batch_fine: Optional[torch.Tensor] = None) -> torch.Tensor:
        interp = knn_interpolate(x_coarse, pos_coarse, pos_fine, batch_coarse, batch_fine, k=self.k)
        return _linear(interp, self.lin)


class _SelectWeight(nn.Module):
    """the one parameter of PyG's ``SelectTopK``: ``weight [1, d_in]``, uniform in +-1/sqrt(d_in)"""

    def __init__(self, d_in: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(1, d_in))
        bound = 1.0 / math.sqrt(d_in)
        nn.init.uniform_(self.weight, -bound, bound)


def num_selected(ratio: float, num_nodes) -> np.ndarray:
    """nodes kept per graph: ``ceil(ratio * n)`` in fp32, as PyG's ``topk`` computes it (``ratio * n.to(x.dtype)``)"""
    n = np.asarray(num_nodes, dtype=np.int64)
    return np.ceil(np.float32(ratio) * n.astype(np.float32)).astype(np.int64)


def select_topk(score: torch.Tensor, ratio: float, batch: torch.Tensor):
    """(perm, coarse offsets as a list): the ``ceil(ratio * n_g)`` highest scores of every graph g, ordered by graph, then by
    descending score (equal scores: the lower node first) -- PyG ``SelectTopK`` + ``topk``.  Torch sort ops; reads the graph
    offsets back once."""
    dev = score.device
    N = int(score.shape[0])
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), [0, 0]
    b = batch.to(torch.int64).contiguous()
    nseg = int(b[-1]) + 1
    ptr = torch.searchsorted(b, torch.arange(nseg + 1, dtype=torch.int64, device=dev)).cpu().numpy()
    kg = np.minimum(num_selected(ratio, np.diff(ptr)), np.diff(ptr))
    by_score = torch.sort(score.reshape(-1), descending=True, stable=True)[1]
    by_graph = torch.sort(b[by_score], stable=True)[1]          # graphs in order, scores descending inside
    pick = np.concatenate([np.arange(ptr[g], ptr[g] + kg[g]) for g in range(nseg)]) if nseg else np.zeros(0, dtype=np.int64)
    perm = by_score[by_graph[torch.from_numpy(pick.astype(np.int64)).to(dev)]]
    return perm, [0] + np.cumsum(kg).tolist()


class DownSampler(nn.Module):
    """fine graph -> coarse graph.  ``forward(x, pos, batch, attn=None)``: score = (attn or x) . w / ||w|| with
    ``w = select.weight``; per graph the ``ceil(ratio * n)`` highest scores are kept (``perm``: by graph, then by descending
    score; the softmax upstream applies to the score is monotone and changes nothing).  Returns a ``Graph`` with
    ``x = lin(x[perm])``, ``pos[perm]``, ``batch[perm]``, ``edge_index = knn_graph(pos_c, 6, batch_c, force_undirected=True)``,
    ``edge_attr = None`` and, beyond upstream, ``perm``.  As upstream, no gradient reaches ``select.weight``.  ``lin`` runs on
    the engine's fused Linear where ``d_in`` and ``d_out`` are both one of ``DENSE_IN_WIDTHS`` (16, 32, 48, 64, 96, 128, 192,
    256, 384); every other width falls back to ``F.linear``.  The rows are gathered ahead of the launch: its gathered input
    phases belong to a ``Topology`` and have no weight-gradient operand without the norm prologue."""

    def __init__(self, d_in: int, d_out: int, ratio: float = 0.25):
        super().__init__()
        self.ratio = ratio
        self.lin = nn.Linear(d_in, d_out)
        self.select = _SelectWeight(d_in)

    @torch.no_grad()
    def score(self, x: torch.Tensor, attn: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the selection score [N]: (attn or x) . w / ||w||"""
        w = self.select.weight.reshape(-1)
        return ((x if attn is None else attn).float() * w).sum(dim=-1) / w.norm(p=2)

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor, attn: Optional[torch.Tensor] = None) -> Graph:
        _require_device(x, pos, batch, attn)
        with torch.no_grad():
            perm, ptr_c = select_topk(self.score(x, attn), self.ratio, batch)
        pos_c, batch_c = pos[perm], batch[perm]
        x_c = _linear(x.index_select(0, perm), self.lin)
        edge_index = knn_graph(pos_c, 6, ptr=ptr_c, force_undirected=True)
        return Graph(x=x_c, pos=pos_c, batch=batch_c, edge_index=edge_index, edge_attr=None, perm=perm)
