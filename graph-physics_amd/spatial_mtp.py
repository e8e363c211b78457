"""Spatial multi-token prediction over 1-hop stars (graphphysics/models/spatial_mtp_1hop.py; ``training.use_spatial_mtp``).

Each selected centre node forms a "star": its own row of the decoder's input ``H`` first, then its 1-hop neighbours' rows of the
node encoder's output ``H_neigh``.  The rows pass an RMSNorm and ``num_layers`` blocks of ``x + MHA(RMSNorm(x))``,
``x + gated_mlp(RMSNorm(x))`` with full attention inside the star; the model's own decoder is applied to the neighbour rows and an
MSE against their targets is the auxiliary loss.

The reference pads every star to ``1 + max_deg`` rows and masks the padding.  A padded key is masked and a padded query is never
read, so the same mathematics runs here on PACKED rows: star ``b`` owns rows ``[off[b], off[b+1])`` of one ``[R, d]`` matrix.  On the
device every step is an engine launch (include/mgn_hip_mtp.h, csrc/mgn_starattn.inc): offsets, optional neighbour cap, pack + RMSNorm,
per block one in-projection (``dense`` with the norm prologue), the star attention, the out-projection with the residual epilogue and
the gated-MLP half as :class:`transformer.Transformer` runs it, then the loss tail.  CPU tensors take the same packed algorithm as
torch ops (what the host tests pin to the reference).

Same constructor, ``forward`` signature, ``state_dict`` keys and initialisers as the reference module.
"""
from __future__ import annotations

import math
import weakref
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .gated import build_gated_mlp
from .layers import RMSNorm

SUPPORTED_D = (16, 32, 64, 128)
SUPPORTED_HEADS = (1, 2, 4, 8, 16)
REDUCTIONS = {"mean_per_center": 0, "mean": 1}


class _EncoderBlock(nn.Module):
    """parameters of one block under the reference's names; ``attn`` is an ``nn.MultiheadAttention`` for its parameter layout and
    initialisers only -- its forward is never called"""

    def __init__(self, d_model: int, num_heads: int):
        super().__init__()
        self.ln1 = RMSNorm(d_model)
        self.attn = nn.MultiheadAttention(d_model, num_heads, batch_first=True)
        self.ln2 = RMSNorm(d_model)
        self.ffn = build_gated_mlp(in_size=d_model, hidden_size=d_model, out_size=d_model)


class _Encoder(nn.Module):
    def __init__(self, d_model: int, num_heads: int, num_layers: int):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderBlock(d_model, num_heads) for _ in range(num_layers)])


# ---------------------------------------------------------------------------------------------------- device autograd nodes
class _StarPackFn(torch.autograd.Function):
    """X = RMSNorm(rows gathered into stars; scale) on ``mgn_star_pack``.  Backward: ``mgn_rownorm_bwd`` on the gathered rows, then
    one CSR grouping of the rows by node (``mgn_csr_build``) and one segment sum (``mgn_segsum``): centre rows land in dH (a
    repeated centre is summed), neighbour rows in dH_neigh; untouched nodes get exact zeros.  No atomics."""

    @staticmethod
    def forward(ctx, H, Hn, scale, tabs):
        from ._launch import call
        shared = Hn is None
        H = ops._f32c(H)
        Hn = H if shared else ops._f32c(Hn)
        scale = ops._f32c(scale)
        N, d = int(H.shape[0]), int(H.shape[1])
        B, R, dev = tabs["B"], tabs["R"], H.device
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        tabs["row_node"], tabs["row_star"] = torch.empty(R, **i32), torch.empty(R, **i32)
        tabs["row_key"] = torch.empty(R, dtype=torch.int64, device=dev)
        tabs["nb_rows"], tabs["nb_ptr"] = torch.empty(max(R - B, 1), **i32), torch.empty(R + 1, **i32)
        X0, X, inv = torch.empty(R, d, **f32), torch.empty(R, d, **f32), torch.empty(R, **f32)
        call("mgn_star_pack", dev, ops._ptr(tabs["rowptr"]), ops._ptr(tabs["nbr"]), ops._ptr(tabs["centers"]), ops._ptr(tabs["off"]),
             ops._ptr(tabs.get("keep")), ops._ptr(H), ops._ptr(Hn), ops._ptr(scale), N, B, R, d, 0 if shared else N,
             ops._ptr(tabs["row_node"]), ops._ptr(tabs["row_star"]), ops._ptr(tabs["row_key"]), ops._ptr(tabs["nb_rows"]),
             ops._ptr(tabs["nb_ptr"]), ops._ptr(X0), ops._ptr(X), ops._ptr(inv))
        ctx.save_for_backward(X0, scale, inv)
        ctx.aux = (tabs["row_key"], N, shared)
        return X

    @staticmethod
    def backward(ctx, dX):
        from . import _capi
        from ._launch import call, workspace
        X0, scale, inv = ctx.saved_tensors
        row_key, N, shared = ctx.aux
        R, d = X0.shape
        dev = X0.device
        dX = ops._f32c(dX)
        dX0 = torch.empty(R, d, dtype=torch.float32, device=dev)
        dscale = torch.empty(d, dtype=torch.float32, device=dev)
        ws = workspace(_capi.lib().mgn_rownorm_bwd_workspace_bytes(d), dev)
        arr = (_capi.RownormPhase * 1)()
        arr[0].x, arr[0].ldx, arr[0].K, arr[0].idx, arr[0].dx, arr[0].lddx = X0.data_ptr(), d, d, None, dX0.data_ptr(), d
        call("mgn_rownorm_bwd", dev, dX.data_ptr(), arr, 1, inv.data_ptr(), scale.data_ptr(), ops.EPS, R, dscale.data_ptr(), ws.data_ptr(),
             ws.numel())
        groups = N if shared else 2 * N
        rowptr, perm = ops.csr_build(row_key, groups)
        out = ops.segsum(dX0, rowptr, perm)
        if shared:
            return out, None, dscale, None
        return out[N:], out[:N], dscale, None


class _StarAttnFn(torch.autograd.Function):
    """multi-head attention inside each row segment of the packed ``qkv`` [R, 3d] (``mgn_star_attn_fwd`` / ``_bwd``)"""

    @staticmethod
    def forward(ctx, qkv, off, B, heads):
        from ._launch import call
        qkv = ops._f32c(qkv)
        R, d = int(qkv.shape[0]), int(qkv.shape[1]) // 3
        y = torch.empty(R, d, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(R, heads, dtype=torch.float32, device=qkv.device)
        call("mgn_star_attn_fwd", qkv.device, qkv.data_ptr(), off.data_ptr(), R, B, d, heads, y.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(qkv, y, lse, off)
        ctx.aux = (B, heads)
        return y

    @staticmethod
    def backward(ctx, dy):
        from ._launch import call
        qkv, y, lse, off = ctx.saved_tensors
        B, heads = ctx.aux
        R, d = y.shape
        dy = ops._f32c(dy)
        dqkv = torch.empty(R, 3 * d, dtype=torch.float32, device=y.device)
        call("mgn_star_attn_bwd", y.device, dy.data_ptr(), qkv.data_ptr(), y.data_ptr(), lse.data_ptr(), off.data_ptr(), R, B, d, heads,
             dqkv.data_ptr())
        return dqkv, None, None, None


def star_attention(qkv: torch.Tensor, off: torch.Tensor, heads: int) -> torch.Tensor:
    """y [R, d] of the packed ``qkv`` [R, 3d] (``nn.MultiheadAttention``'s in-projection layout) with full attention inside every row
    segment ``[off[b], off[b+1])``; ``off`` int32 [B + 1] on the device"""
    ops._require_device(qkv, off)
    return _StarAttnFn.apply(qkv, off, int(off.numel()) - 1, int(heads))


class _NeighbourRowsFn(torch.autograd.Function):
    """the neighbour rows of the packed matrix (``mgn_gather_rows``); backward: the transposed CSR through ``mgn_segsum`` -- centre rows
    get exact zeros"""

    @staticmethod
    def forward(ctx, Z, nb_rows, nb_ptr, T):
        ctx.nb_ptr = nb_ptr
        return ops.gather_rows(ops._f32c(Z), nb_rows[:T])

    @staticmethod
    def backward(ctx, g):
        return ops.segsum(ops._f32c(g), ctx.nb_ptr, None), None, None, None


class _StarLossFn(torch.autograd.Function):
    """(loss, mean pair loss) of ``mgn_star_loss``; the launch leaves d loss / d yhat behind for the backward"""

    @staticmethod
    def forward(ctx, yhat, target, tabs, reduction):
        from ._launch import call
        yhat, target = ops._f32c(yhat), ops._f32c(target)
        T, O = yhat.shape
        dev = yhat.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        dyhat = torch.empty(T, O, dtype=torch.float32, device=dev)
        call("mgn_star_loss", dev, yhat.data_ptr(), target.data_ptr(), tabs["row_node"].data_ptr(), tabs["off"].data_ptr(), int(target.shape[0]),
             tabs["B"], tabs["R"], O, reduction, out.data_ptr(), dyhat.data_ptr())
        ctx.save_for_backward(dyhat)
        pair = out[1]
        ctx.mark_non_differentiable(pair)
        return out[0], pair

    @staticmethod
    def backward(ctx, g, _g_pair):
        (dyhat,) = ctx.saved_tensors
        return dyhat * g, None, None, None


def star_tables(rowptr: torch.Tensor, nbr: torch.Tensor, centers: torch.Tensor, N: int, max_neighbors: Optional[int] = None, seed: int = 0,
                step: int = 0):
    """The segment table of the stars of ``centers`` over the CSR ``rowptr`` / ``nbr`` (int32, by source): ``(tabs, stats)`` with
    ``tabs = dict(B, R, rowptr, nbr, centers, off[, keep])`` and ``stats`` = device floats {pairs, max_deg}; ``tabs`` is None when no
    centre has a neighbour.  ``mgn_star_offsets`` and, with ``max_neighbors``, ``mgn_star_cap``.  Holds the call's ONE host read: the
    packed row count R (and the bad-centre flag, in the same copy)."""
    from ._launch import call
    dev = rowptr.device
    B = int(centers.numel())
    centers = centers.to(device=dev, dtype=torch.int32).contiguous()
    cap = int(max_neighbors) if max_neighbors is not None else 0
    off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    meta = torch.empty(2, dtype=torch.int32, device=dev)
    stats = torch.empty(2, dtype=torch.float32, device=dev)
    call("mgn_star_offsets", dev, rowptr.data_ptr(), centers.data_ptr(), N, B, cap, off.data_ptr(), meta.data_ptr(), stats.data_ptr())
    R, flags = (int(v) for v in meta.tolist())   # the one host read
    if flags & 1:
        raise IndexError(f"SpatialMTP1Hop: centers has entries outside [0, {N})")
    if flags & 2:
        raise ValueError("SpatialMTP1Hop: more packed rows than the kernels index (INT32_MAX / 384)")
    if R == B:
        return None, stats
    tabs = dict(B=B, R=R, rowptr=rowptr, nbr=nbr, centers=centers, off=off)
    if cap > 0:
        keep = torch.empty(R - B, dtype=torch.int32, device=dev)
        call("mgn_star_cap", dev, rowptr.data_ptr(), centers.data_ptr(), off.data_ptr(), N, B, cap, int(seed) & (2 ** 64 - 1),
             int(step) & 0xFFFFFFFF, keep.data_ptr())
        tabs["keep"] = keep
    return tabs, stats


def pack_stars(H: torch.Tensor, H_neigh: Optional[torch.Tensor], scale: torch.Tensor, tabs: dict) -> torch.Tensor:
    """X [R, d] = RMSNorm(the rows of the stars of ``tabs``; scale): centre rows from ``H``, neighbour rows from ``H_neigh`` (``H``
    when None); fills ``tabs`` with row_node, row_star, row_key, nb_rows and nb_ptr.  Differentiable in H, H_neigh and scale."""
    return _StarPackFn.apply(H, H_neigh, scale, tabs)


def star_loss(yhat: torch.Tensor, target: torch.Tensor, tabs: dict, reduction: str = "mean_per_center"):
    """(loss, mean pair loss) of the decoder's output on the neighbour rows of the packed stars of ``tabs``"""
    return _StarLossFn.apply(yhat, target, tabs, REDUCTIONS[reduction])


# ---------------------------------------------------------------------------------------------------- adjacency
_csr_cache: dict = {}


def _csr_of_edges(edge_index: torch.Tensor, num_nodes: int, assume_undirected: bool):
    """(rowptr int32 [N + 1], nbr int32 [M]) by source, edges kept as they are (duplicates and self loops stay); with
    ``assume_undirected=False`` the reversed edges are appended.  Built once per ``edge_index`` object."""
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), num_nodes, bool(assume_undirected), str(edge_index.device))
    hit = _csr_cache.get(key)
    if hit is not None and hit[0]() is edge_index:
        return hit[1], hit[2]
    e = edge_index.long()
    if not assume_undirected:
        e = torch.cat([e, torch.stack([e[1], e[0]], dim=0)], dim=1)
    if e.is_cuda:
        rowptr, perm = ops.csr_build(e[0], num_nodes)
        nbr = e[1].index_select(0, perm.long()).to(torch.int32)
    else:
        order = torch.argsort(e[0], stable=True)
        nbr = e[1][order]
        rowptr = torch.zeros(num_nodes + 1, dtype=torch.long)
        rowptr[1:] = torch.bincount(e[0], minlength=num_nodes).cumsum(0)
    if len(_csr_cache) > 16:
        _csr_cache.clear()
    _csr_cache[key] = (weakref.ref(edge_index), rowptr, nbr)
    return rowptr, nbr


def _rms(x, scale, eps: float = 1e-8):
    return scale * (x / (x.norm(2, dim=-1, keepdim=True) / math.sqrt(x.shape[-1]) + eps))


class SpatialMTP1Hop(nn.Module):
    """1-hop spatial MTP on packed stars (module docstring).

    ``forward`` takes the reference's arguments plus ``topology`` (an ``ops.Topology`` of ``edge_index`` in the caller's numbering: its
    source-grouped CSR is used and nothing is sorted) and ``step`` (the counter that keys the neighbour cap's random stream; the
    module counts its own calls when it is None).

    Host reads: exactly ONE per call -- the packed row count ``R`` (with the bad-centre flag, in the same copy), which sizes every
    tensor after it.  The returned statistics are device scalars."""

    def __init__(self, d_model: int, num_heads: int = 4, num_layers: int = 1, assume_undirected: bool = True,
                 max_neighbors: Optional[int] = None):
        super().__init__()
        if d_model % num_heads != 0:
            raise ValueError(f"SpatialMTP1Hop: num_heads={num_heads} does not divide d_model={d_model}")
        self.d_model, self.num_heads, self.num_layers = int(d_model), int(num_heads), int(num_layers)
        self.enc = _Encoder(d_model, num_heads, num_layers)
        self.in_ln = RMSNorm(d_model)
        self.assume_undirected = assume_undirected
        self.max_neighbors = max_neighbors
        self.seed = 0           # key of the cap's device stream
        self._calls = 0
        self._generator = None  # the cap's generator on the CPU path

    # ------------------------------------------------------------------ shared pieces
    def _adjacency(self, H, edge_index, row_ptr, dst_sorted, topology):
        N, dev = int(H.shape[0]), H.device
        if row_ptr is not None and dst_sorted is not None:
            rowptr, nbr = row_ptr.to(dev), dst_sorted.to(dev)
        elif topology is not None and H.is_cuda:
            if topology.node_order is not None:
                raise ValueError("SpatialMTP1Hop: `topology` must be in the caller's numbering (this one is renumbered)")
            if not self.assume_undirected:
                raise ValueError("SpatialMTP1Hop: `topology` holds the edges as given; assume_undirected=False needs edge_index")
            rowptr, nbr = topology.rowptr_src, topology.neighbours_by_source()
        else:
            rowptr, nbr = _csr_of_edges(edge_index.to(dev), N, self.assume_undirected)
        if H.is_cuda:
            return rowptr.to(torch.int32).contiguous(), nbr.to(torch.int32).contiguous()
        return rowptr.long(), nbr.long()

    def _act(self, blk) -> str:
        return "silu" if isinstance(blk.ffn[1].activation, nn.SiLU) else "gelu"

    @staticmethod
    def _early(H, B):
        return H.new_tensor(0.0), {"sp_mtp/centers": torch.tensor(float(B), device=H.device) if B else H.new_tensor(0),
                                   "sp_mtp/pairs": H.new_tensor(0)}

    def forward(self, H: torch.Tensor, edge_index: torch.Tensor, centers: torch.Tensor, out_head: nn.Module, target: torch.Tensor,
                reduction: str = "mean_per_center", row_ptr: Optional[torch.Tensor] = None, dst_sorted: Optional[torch.Tensor] = None,
                H_neigh: Optional[torch.Tensor] = None, topology=None, step: Optional[int] = None
                ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        if reduction not in REDUCTIONS:
            reduction = "mean_per_center"   # (the reference treats every other word as its default)
        centers = centers.to(device=H.device)
        if centers.numel() == 0:
            return self._early(H, 0)
        if step is None:
            step = self._calls
        self._calls += 1
        rowptr, nbr = self._adjacency(H, edge_index, row_ptr, dst_sorted, topology)
        if H.is_cuda:
            return self._forward_device(H, rowptr, nbr, centers, out_head, target, reduction, H_neigh, int(step))
        return self._forward_torch(H, rowptr, nbr, centers.long(), out_head, target, reduction, H_neigh)

    # ------------------------------------------------------------------ the engine
    def _forward_device(self, H, rowptr, nbr, centers, out_head, target, reduction, H_neigh, step):
        from .dense import dense, rms_norm
        d = int(H.shape[1])
        if d != self.d_model or d not in SUPPORTED_D or self.num_heads not in SUPPORTED_HEADS:
            raise NotImplementedError(f"SpatialMTP1Hop on the HIP kernels needs d_model in {SUPPORTED_D} and num_heads in {SUPPORTED_HEADS}, "
                                      f"got rows of {d} columns, d_model={self.d_model}, num_heads={self.num_heads}")
        if ops.get_matrix_precision() == "bf16":
            raise NotImplementedError("SpatialMTP1Hop runs in fp32: use_spatial_mtp with enable_vram_optimizations (bf16 matrices) is not built")
        dev = H.device
        B = int(centers.numel())
        tabs, stats = star_tables(rowptr, nbr, centers, int(H.shape[0]), self.max_neighbors, self.seed, step)
        if tabs is None:
            return self._early(H, B)
        R, off = tabs["R"], tabs["off"]
        x = _StarPackFn.apply(H, H_neigh, self.in_ln.scale, tabs)
        for blk in self.enc.layers:
            a = blk.attn
            qkv = dense(x, a.in_proj_weight, a.in_proj_bias, norm_scale=blk.ln1.scale)
            y = _StarAttnFn.apply(qkv, off, B, self.num_heads)
            x = dense(y, a.out_proj.weight, a.out_proj.bias, resid=x)
            gm = blk.ffn
            h = rms_norm(x, blk.ln2.scale)
            p_ = dense(h, gm[1].linear1.weight, gm[1].linear1.bias, W2=gm[1].linear2.weight, b2=gm[1].linear2.bias, norm_scale=gm[0].scale,
                       act=self._act(blk))
            x = dense(p_, gm[2].weight, gm[2].bias, resid=x)
        zf = _NeighbourRowsFn.apply(x, tabs["nb_rows"], tabs["nb_ptr"], R - B)
        yhat = out_head(zf)
        if yhat.dim() != 2 or not 1 <= int(yhat.shape[1]) <= 32 or int(target.shape[1]) != int(yhat.shape[1]):
            raise NotImplementedError("SpatialMTP1Hop: the output head must give 1..32 columns, as many as `target` has")
        loss, pair = _StarLossFn.apply(yhat, target.detach(), tabs, REDUCTIONS[reduction])
        return loss, {"sp_mtp/centers": torch.tensor(float(B), device=dev), "sp_mtp/pairs": stats[0], "sp_mtp/mean_pair_loss": pair.detach(),
                      "sp_mtp/max_deg": stats[1]}

    # ------------------------------------------------------------------ the same packed algorithm as torch ops (CPU tensors)
    def _forward_torch(self, H, rowptr, nbr, centers, out_head, target, reduction, H_neigh):
        N, d = H.shape
        B = int(centers.numel())
        start = rowptr[centers]
        full = rowptr[centers + 1] - start
        kept = full if self.max_neighbors is None else full.clamp(max=int(self.max_neighbors))
        off = torch.zeros(B + 1, dtype=torch.long)
        off[1:] = (kept + 1).cumsum(0)
        R = int(off[-1])   # the one host read
        if R == B:
            return self._early(H, B)
        row_star = torch.repeat_interleave(torch.arange(B), kept + 1)
        t = torch.arange(R) - off[row_star]
        is_c = t == 0
        pos = (t - 1).clamp_min(0)
        if self.max_neighbors is not None:
            if self._generator is None:
                self._generator = torch.Generator().manual_seed(int(self.seed))
            for b in torch.nonzero(full > kept).flatten().tolist():   # uniform without replacement, as the reference draws it
                pos[int(off[b]) + 1:int(off[b + 1])] = torch.randperm(int(full[b]), generator=self._generator)[:int(kept[b])]
        at = (start[row_star] + pos).clamp(max=max(int(nbr.numel()) - 1, 0))
        row_node = torch.where(is_c, centers[row_star], nbr[at] if nbr.numel() else centers[row_star])
        Hn = H if H_neigh is None else H_neigh
        x = _rms(torch.where(is_c.unsqueeze(1), H[row_node], Hn[row_node]), self.in_ln.scale)
        same = row_star.unsqueeze(0) == row_star.unsqueeze(1)
        heads, dh = self.num_heads, d // self.num_heads
        for blk in self.enc.layers:
            a = blk.attn
            qkv = F.linear(_rms(x, blk.ln1.scale), a.in_proj_weight, a.in_proj_bias)
            q, k, v = (m.reshape(R, heads, dh).transpose(0, 1) for m in qkv.split(d, dim=1))
            s = (q @ k.transpose(1, 2)) / math.sqrt(dh)
            p = torch.softmax(s.masked_fill(~same, float("-inf")), dim=-1)
            y = (p @ v).transpose(0, 1).reshape(R, d)
            x = x + F.linear(y, a.out_proj.weight, a.out_proj.bias)
            gm = blk.ffn
            n = _rms(_rms(x, blk.ln2.scale), gm[0].scale)
            act = F.silu if self._act(blk) == "silu" else F.gelu
            p_ = act(F.linear(n, gm[1].linear1.weight, gm[1].linear1.bias)) * F.linear(n, gm[1].linear2.weight, gm[1].linear2.bias)
            x = x + F.linear(p_, gm[2].weight, gm[2].bias)
        nb = ~is_c
        yhat = out_head(x[nb])
        err = (yhat - target[row_node[nb]]).pow(2).mean(dim=-1)
        if reduction == "mean":
            loss = err.mean()
        else:
            per = torch.zeros(B, dtype=err.dtype).index_add(0, row_star[nb], err)
            loss = (per / kept.to(err.dtype).clamp_min(1.0)).mean()
        return loss, {"sp_mtp/centers": torch.tensor(float(B)), "sp_mtp/pairs": torch.tensor(float(R - B)),
                      "sp_mtp/mean_pair_loss": err.mean().detach(), "sp_mtp/max_deg": kept.max().to(torch.float32)}
