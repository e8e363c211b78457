"""Transolver++ processor (graphphysics/models/transolver.py, processors.py:387-461; ``model.type: "transolver"``).

Every block projects the node rows to ``heads x C`` channels, draws a Gumbel-softmax over ``slice_num`` slices per (node, head) row with
a learned per-row temperature, reduces ALL nodes into ``heads x slice_num`` tokens, lets the tokens of a head attend to each other and
broadcasts the result back to the rows.  The reference runs ``Model.forward(x[None], pos[None], None)`` with batch 1 and works on
``[1, H, N, C]`` tensors; here the rows stay ``[N, H * C]`` and a collated batch of meshes is one row set, exactly as there.

On the device the node-sized part -- slice weights, the two reductions, the broadcast and the per-row backward -- is one
``torch.autograd.Function`` around the launches of include/mgn_hip_slice.h (csrc/mgn_slice.inc); every ``nn.Linear`` is a fused
``dense`` launch (narrow widths zero-padded to the widths the launch takes), the temporal block is ``transformer.TemporalAttention``.
Deliberately left as torch ops in this change: ``nn.LayerNorm`` (the engine has RMSNorm kernels only) and the token part between the
reduction and the broadcast (``[H, G, C]`` tensors of a few thousand elements, differentiated by torch autograd).  The slice weights
``w`` are saved for the backward, not recomputed.  fp32 only: there is no bf16 matrix mode.

CPU tensors take the same algorithm as torch ops (what the host tests pin to the reference); ``Model.backend = "torch"`` selects
that path on the device too (tools/kbench_transolver.py).

Noise.  The reference draws ``torch.rand_like`` in every forward, in eval mode too.  Here ``u`` comes from a counter-based stream keyed
by ``(noise_seed, call counter, layer, n, h, g)`` (include/mgn_hip_slice.h).  The call counter is a NON-persistent int64 device buffer
that every forward advances with an op on the stream, and the kernels read it from device memory: a captured graph that is replayed
draws new noise every time.  ``Model.noise_u`` (tests) injects the uniforms per layer instead.

Same constructor signature, module tree, ``state_dict`` keys and shapes, and the same kind of initialisers as the reference.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import build_mlp

SUPPORTED_HIDDEN = (16, 32, 64, 128)
MAX_SLICES = 64     # one lane per slice on a 64-wide wavefront
MAX_CHANNELS = 64   # channels per head
_DENSE_K = (16, 32, 48, 64, 96, 128, 192, 256, 384)   # input widths a dense launch takes (include/mgn_hip.h, "Dense row work")
_TEMPORAL_HEADS = (1, 2, 4, 8, 16)


def _dense_k(k: int, what: str) -> int:
    for v in _DENSE_K:
        if v >= k:
            return v
    raise NotImplementedError(f"Transolver on the HIP dense kernels: {what} has {k} input columns, a launch takes at most {_DENSE_K[-1]}")


def _linear(x, lin: nn.Linear, act: Optional[str] = None, resid=None, hip: bool = True):
    """``[resid +] act(lin(x))``: one fused ``dense`` launch on the device (input columns and output rows of the weight zero-padded to
    widths the launch takes, as ``ops.mlp_apply`` pads its first and last layer), torch ops otherwise"""
    W, b = lin.weight, lin.bias
    if not hip:
        y = F.linear(x, W, b)
        if act == "gelu":
            y = F.gelu(y)
        return y if resid is None else resid + y
    from .dense import dense
    N, K = int(W.shape[0]), int(W.shape[1])
    Kp, Np = _dense_k(K, "a Linear"), ops.pad16(N)
    if Kp != K:
        x, W = F.pad(x, (0, Kp - K)), F.pad(W, (0, Kp - K))
    if Np != N:
        W = F.pad(W, (0, 0, 0, Np - N))
        b = F.pad(b, (0, Np - N)) if b is not None else None
        assert resid is None
    y = dense(x, W, b, act=act, resid=resid)
    return y[:, :N] if Np != N else y


def _temporal_torch(tb, h_prev, h_pred):
    """``TemporalAttention(h_prev, h_pred, None)`` as torch ops for CPU tensors (layers.py:822-887 without an adjacency: attention over
    the head axis of each node, ``[N, d, heads]`` operands scaled by sqrt(d))"""
    N = h_prev.size(0)
    q, k, v = (p(t).reshape(N, tb.d, tb.H) for p, t in ((tb.q_proj, h_pred), (tb.k_proj, h_prev), (tb.v_proj, h_pred)))
    y = torch.softmax((q / math.sqrt(tb.d)) @ k.transpose(-2, -1), dim=-1) @ v
    out = tb.out_proj(y.reshape(N, tb.h))
    if tb.use_gate:
        out = tb.gate(torch.cat([h_pred, h_prev], dim=-1)) * out
    h_corr = h_prev + out
    return h_corr + tb.mixer(torch.cat([h_corr, h_prev], dim=-1))


# ---------------------------------------------------------------------------------------------------- the launches
def slice_uniforms(seed: int, step: torch.Tensor, layer: int, N: int, H: int, G: int) -> torch.Tensor:
    """u [N, H, G] of the noise stream for ``(seed, step, layer)`` (``mgn_slice_uniforms``); ``step``: int64 device tensor of one element"""
    from ._launch import call
    u = torch.empty(N, H, G, dtype=torch.float32, device=step.device)
    call("mgn_slice_uniforms", step.device, int(seed) & (2 ** 64 - 1), step.data_ptr(), int(layer), N, H, G, u.data_ptr())
    return u


def slice_aggregate(w: torch.Tensor, x: torch.Tensor, H: int, G: int, C: int, want_norm: bool = True):
    """(S [H, G, C], norm [H, G] or None) of ``w`` [N, H, G] and the rows ``x`` [N, >= H * C] (``mgn_slice_aggregate``)"""
    from . import _capi
    from ._launch import call, workspace
    N, dev = int(w.shape[0]), w.device
    S = torch.empty(H, G, C, dtype=torch.float32, device=dev)
    norm = torch.empty(H, G, dtype=torch.float32, device=dev) if want_norm else None
    ws = workspace(_capi.lib().mgn_slice_aggregate_workspace_bytes(N, H, G, C), dev)
    call("mgn_slice_aggregate", dev, w.data_ptr(), x.data_ptr(), int(x.stride(0)), N, H, G, C, S.data_ptr(), ops._ptr(norm), ws.data_ptr(),
         ws.numel())
    return S, norm


def slice_expand(w: torch.Tensor, tok: torch.Tensor, H: int, G: int, C: int) -> torch.Tensor:
    """out [N, H * C] = sum_g w[n, h, g] tok[h, g, c] (``mgn_slice_expand``)"""
    from ._launch import call
    N = int(w.shape[0])
    out = torch.empty(N, H * C, dtype=torch.float32, device=w.device)
    call("mgn_slice_expand", w.device, w.data_ptr(), tok.data_ptr(), N, H, G, C, out.data_ptr(), H * C)
    return out


class _SliceAttnFn(torch.autograd.Function):
    """out_x [N, H * C] of the physics attention from x_mid [N, H * C]: launches 2-5 of include/mgn_hip_slice.h, with the token part
    (``token_fn``: torch ops on [H, G, C] tensors) recorded by torch autograd between the reduction and the broadcast and differentiated
    by it in the backward.  ``token_params`` are the parameters ``token_fn`` reads: passed so that their gradients have somewhere to go."""

    @staticmethod
    def forward(ctx, xm, Ws, bs, W1, b1, w2, b2, bias, u, step, meta, token_fn, *token_params):
        from ._launch import call
        seed, layer, H, G, C = meta
        xm = ops._f32c(xm)
        Ws, bs, W1, b1 = ops._f32c(Ws), ops._f32c(bs), ops._f32c(W1), ops._f32c(b1)
        w2, b2, bias = ops._f32c(w2).reshape(-1), ops._f32c(b2).reshape(-1), ops._f32c(bias).reshape(-1)
        N, dev = int(xm.shape[0]), xm.device
        u = ops._f32c(u) if u is not None else None
        w = torch.empty(N, H, G, dtype=torch.float32, device=dev)
        rowsc = torch.empty(max(N * H, 1), 2, dtype=torch.float32, device=dev)
        call("mgn_slice_weights_fwd", dev, xm.data_ptr(), H * C, Ws.data_ptr(), bs.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
             b2.data_ptr(), bias.data_ptr(), ops._ptr(u), seed, step.data_ptr(), layer, N, H, G, C, w.data_ptr(), rowsc.data_ptr())
        S, norm = slice_aggregate(w, xm, H, G, C)
        need = any(ctx.needs_input_grad)
        if need:
            with torch.enable_grad():
                S_, norm_ = S.requires_grad_(True), norm.requires_grad_(True)
                tok = token_fn(S_, norm_)
            ctx.tok_graph = (S_, norm_, tok)
        else:
            tok = token_fn(S, norm)
        tok_d = tok.detach().contiguous()
        out = slice_expand(w, tok_d, H, G, C)
        if need:
            ctx.save_for_backward(xm, w, rowsc, Ws, bs, W1, b1, w2, u, step, tok_d)
            ctx.meta = meta
            ctx.token_params = token_params
        return out

    @staticmethod
    def backward(ctx, dOut):
        from . import _capi
        from ._launch import call, workspace
        xm, w, rowsc, Ws, bs, W1, b1, w2, u, step, tok_d = ctx.saved_tensors
        seed, layer, H, G, C = ctx.meta
        if ctx.tok_graph is None:
            raise RuntimeError("_SliceAttnFn: backward ran twice (the token part's recorded graph is released by the first backward)")
        S_, norm_, tok = ctx.tok_graph
        ctx.tok_graph = None
        N, dev = int(xm.shape[0]), xm.device
        f = dict(dtype=torch.float32, device=dev)
        dOut = ops._f32c(dOut)
        dtok, _ = slice_aggregate(w, dOut, H, G, C, want_norm=False)
        live = [p for p in ctx.token_params if p.requires_grad]
        grads = torch.autograd.grad(tok, [S_, norm_] + live, dtok, allow_unused=True)
        dS = grads[0].contiguous() if grads[0] is not None else torch.zeros(H, G, C, **f)
        dnorm = grads[1].contiguous() if grads[1] is not None else torch.zeros(H, G, **f)
        it = iter(grads[2:])
        dparams = [next(it) if p.requires_grad else None for p in ctx.token_params]
        dx = torch.empty(N, H * C, **f)
        da, dh1, dt2 = torch.empty(N * H, G, **f), torch.empty(N * H, G, **f), torch.empty(max(N * H, 1), **f)
        dw2, db2, dbias = torch.empty(G, **f), torch.empty(1, **f), torch.empty(H, **f)
        ws = workspace(_capi.lib().mgn_slice_rows_bwd_workspace_bytes(N, H, G), dev)
        call("mgn_slice_rows_bwd", dev, dOut.data_ptr(), H * C, tok_d.data_ptr(), dS.data_ptr(), dnorm.data_ptr(), xm.data_ptr(), H * C, w.data_ptr(),
             rowsc.data_ptr(), Ws.data_ptr(), bs.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), ops._ptr(u), seed, step.data_ptr(), layer,
             N, H, G, C, dx.data_ptr(), H * C, da.data_ptr(), dh1.data_ptr(), dt2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), dbias.data_ptr(),
             ws.data_ptr(), ws.numel())
        # the two G x C weight gradients: the same reduction over the N * H (row, head) pairs, one "head"
        rows = xm.view(N * H, C)
        dWs, dbs = slice_aggregate(da.view(N * H, 1, G), rows, 1, G, C)
        dW1, db1 = slice_aggregate(dh1.view(N * H, 1, G), rows, 1, G, C)
        return (dx, dWs.view(G, C), dbs.view(G), dW1.view(G, C), db1.view(G), dw2.view(1, G), db2, dbias.view(1, H, 1, 1), None, None, None, None,
                *dparams)


# ---------------------------------------------------------------------------------------------------- modules
class Physics_Attention_1D_Eidetic(nn.Module):
    """the reference's module of this name (transolver.py:35-165) on ``[N, dim]`` rows; ``forward(x, pos, ctl)`` -- ``ctl`` carries the
    path and the noise source of this call (see :class:`Model`)"""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.0, slice_num=64, use_rope_embeddings: bool = False, rope_pos_dimension: int = 3,
                 rope_base: float = 10000.0, use_gated_attention: bool = False):
        super().__init__()
        if dropout != 0:
            raise NotImplementedError("Transolver: dropout != 0 is not built (the reference's configs train with dropout 0)")
        if not 1 <= slice_num <= MAX_SLICES or not 1 <= dim_head <= MAX_CHANNELS:
            raise NotImplementedError(f"Transolver on the HIP kernels needs slice_num in 1..{MAX_SLICES} and hidden_size / num_heads in "
                                      f"1..{MAX_CHANNELS}, got slice_num={slice_num}, channels per head={dim_head}")
        inner_dim = dim_head * heads
        self.dim_head, self.heads, self.slice_num = dim_head, heads, slice_num
        self.keep_last, self.last = False, None   # (tests: the torch-ops path keeps its intermediates of the last call)
        self.scale = dim_head ** -0.5
        self.softmax = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.bias = nn.Parameter(torch.ones([1, heads, 1, 1]) * 0.5)
        self.proj_temperature = nn.Sequential(nn.Linear(dim_head, slice_num), nn.GELU(), nn.Linear(slice_num, 1), nn.GELU())
        self.use_rope_embeddings, self.rope_pos_dimension, self.rope_base = use_rope_embeddings, rope_pos_dimension, rope_base
        self.use_gated_attention = use_gated_attention
        if self.use_rope_embeddings:
            if rope_pos_dimension <= 0:
                raise ValueError("rope_pos_dimension must be positive when use_rope_embeddings=True.")
            self.rope_projection = nn.Linear(rope_pos_dimension * 2, dim_head)
        else:
            self.rope_projection = None
        self.in_project_x = nn.Linear(dim, inner_dim)
        self.in_project_slice = nn.Linear(dim_head, slice_num)
        torch.nn.init.orthogonal_(self.in_project_slice.weight)
        self.to_q = nn.Linear(dim_head, dim_head, bias=False)
        self.to_k = nn.Linear(dim_head, dim_head, bias=False)
        self.to_v = nn.Linear(dim_head, dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, dim), nn.Dropout(dropout))
        if self.use_gated_attention:
            self.attn_gate = nn.Sequential(nn.Linear(2 * dim_head, dim_head), nn.SiLU(), nn.Linear(dim_head, dim_head), nn.Sigmoid())
        else:
            self.attn_gate = None

    def _rope_features(self, pos: torch.Tensor) -> torch.Tensor:
        r = self.rope_pos_dimension
        if pos.size(-1) < r:
            raise ValueError(f"Expected at least {r} positional dimensions, but received {pos.size(-1)}.")
        log_base = torch.log(torch.tensor(self.rope_base, device=pos.device, dtype=pos.dtype))
        inv_freq = torch.exp(-torch.arange(r, device=pos.device, dtype=pos.dtype) * log_base / max(r, 1))
        angles = pos[..., :r] * inv_freq.view(1, r)
        return torch.cat((torch.sin(angles), torch.cos(angles)), dim=-1)

    def _tokens(self, S: torch.Tensor, norm: torch.Tensor) -> torch.Tensor:
        """out_slice_token [H, G, C] from the reductions S [H, G, C] and norm [H, G]: plain torch ops on either device.  The reference's
        ``F.scaled_dot_product_attention`` takes its default scale C^-0.5 (``self.scale``, ``self.softmax``, ``self.dropout`` are unused there)"""
        token = S / (norm + 1e-5).unsqueeze(-1)
        q, k, v = self.to_q(token), self.to_k(token), self.to_v(token)
        p = torch.softmax(q @ k.transpose(1, 2) * (1.0 / math.sqrt(self.dim_head)), dim=-1)
        out = p @ v
        if self.attn_gate is not None:
            out = self.attn_gate(torch.cat([token, out], dim=-1)) * out
        return out

    def _token_params(self) -> List[torch.Tensor]:
        ps = [self.to_q.weight, self.to_k.weight, self.to_v.weight]
        if self.attn_gate is not None:
            ps += list(self.attn_gate.parameters())
        return ps

    def forward(self, x, pos=None, ctl=None):
        N, H, C, G = int(x.shape[0]), self.heads, self.dim_head, self.slice_num
        hip = ctl["hip"]
        xm = _linear(x, self.in_project_x, hip=hip)
        if self.use_rope_embeddings and pos is not None:
            rope = _linear(self._rope_features(pos).to(xm.dtype), self.rope_projection, hip=hip)
            xm = (xm.view(N, H, C) + rope.unsqueeze(1)).reshape(N, H * C)
        pt, sl = self.proj_temperature, self.in_project_slice
        if hip:
            out_x = _SliceAttnFn.apply(xm, sl.weight, sl.bias, pt[0].weight, pt[0].bias, pt[2].weight, pt[2].bias, self.bias, ctl["u"], ctl["step"],
                                       (ctl["seed"], ctl["layer"], H, G, C), self._tokens, *self._token_params())
        else:
            # head-major [H, N, .] operands and the reference's einsums: the same operations in the same order as there (batch of 1 dropped)
            x3 = xm.view(N, H, C).permute(1, 0, 2).contiguous()
            tpre = pt(x3) + self.bias.view(H, 1, 1)
            t = torch.clamp(tpre, min=0.01)
            u = ctl["u"].permute(1, 0, 2)
            gum = -torch.log(-torch.log(u + 1e-8) + 1e-8)
            # softmax((y - c) / t) is the same function for any per-row c, and its value does not depend on c (sum_g dz_g = 0): with the
            # row maximum as a CONSTANT c the temperature's gradient is -sum_g dz_g (y_g - c) / t^2, the same number from small
            # operands instead of one that cancels at the size of y (the kernels form it the same way)
            y = sl(x3) + gum
            w = torch.softmax((y - y.detach().amax(dim=-1, keepdim=True)) / t, dim=-1)
            self.last_tpre = tpre.detach().squeeze(-1).t()
            tok = self._tokens(torch.einsum("hnc,hng->hgc", x3, w).contiguous(), w.sum(1))
            out_x = torch.einsum("hgc,hng->hnc", tok, w).permute(1, 0, 2).reshape(N, H * C)
            if self.keep_last:   # (tests: this call's x_mid, w [N, H, G] and out_x, still attached to the graph)
                self.last = (xm, w.permute(1, 0, 2), out_x)
        return _linear(out_x, self.to_out[0], hip=hip)


class Transolver_plus_block(nn.Module):
    """transolver.py:168-228: ``fx = Attn(ln_1(fx)) + fx``, ``fx = mlp(ln_2(fx)) + fx`` and, in the last block, ``mlp2(ln_3(fx))``.  The
    reference's ``checkpoint`` calls in training mode do not change the mathematics and are not reproduced."""

    def __init__(self, num_heads: int, hidden_dim: int, dropout: float, act="gelu", mlp_ratio=4, last_layer=False, out_dim=1, slice_num=32,
                 use_rope_embeddings: bool = False, rope_pos_dimension: int = 3, rope_base: float = 10000.0, use_gated_attention: bool = False):
        super().__init__()
        self.last_layer = last_layer
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.Attn = Physics_Attention_1D_Eidetic(hidden_dim, heads=num_heads, dim_head=hidden_dim // num_heads, dropout=dropout, slice_num=slice_num,
                                                 use_rope_embeddings=use_rope_embeddings, rope_pos_dimension=rope_pos_dimension,
                                                 rope_base=rope_base, use_gated_attention=use_gated_attention)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = build_mlp(in_size=hidden_dim, hidden_size=hidden_dim * mlp_ratio, out_size=hidden_dim, nb_of_layers=2, layer_norm=False, act=act)
        if self.last_layer:
            self.ln_3 = nn.LayerNorm(hidden_dim)
            self.mlp2 = nn.Linear(hidden_dim, out_dim)

    def forward(self, fx, pos=None, ctl=None):
        hip = ctl["hip"]
        attn_out = self.Attn(self.ln_1(fx), pos, ctl)
        fx = attn_out + fx
        fx = _linear(_linear(self.ln_2(fx), self.mlp[0], act="gelu", hip=hip), self.mlp[2], resid=fx, hip=hip)
        if self.last_layer:
            return _linear(self.ln_3(fx), self.mlp2, hip=hip)
        return fx


class Model(nn.Module):
    """transolver.py:231-394 on ``[N, C]`` rows (the reference's batch of 1 dropped).

    ``noise_seed`` (default 0; ``Engine(seed=)`` sets it) keys the noise stream; ``noise_u`` (tests): None, or one ``[N, heads, slice_num]``
    tensor of uniforms per block, used instead of the stream; ``backend``: "auto" (the HIP kernels for device tensors, torch ops for CPU
    tensors) or "torch" (the torch-ops path on any device, with the same noise stream on the device)."""

    def __init__(self, space_dim=1, n_layers=5, n_hidden=256, dropout=0, n_head=8, act="gelu", mlp_ratio=1, fun_dim=1, out_dim=1, slice_num=32,
                 ref=8, unified_pos=False, use_rope_embeddings: bool = False, use_gated_attention: bool = False, rope_pos_dimension: int = 3,
                 rope_base: float = 10000.0, use_temporal_block: bool = False):
        super().__init__()
        self.__name__ = "UniPDE_3D"
        self.ref, self.unified_pos = ref, unified_pos
        self.use_rope_embeddings, self.use_gated_attention = use_rope_embeddings, use_gated_attention
        self.rope_pos_dimension, self.rope_base = rope_pos_dimension, rope_base
        self.use_temporal_block = use_temporal_block
        if n_hidden not in SUPPORTED_HIDDEN or n_hidden % n_head != 0:
            raise NotImplementedError(f"Transolver on the HIP dense kernels needs hidden_size in {SUPPORTED_HIDDEN} and num_heads dividing it, "
                                      f"got hidden_size={n_hidden}, num_heads={n_head}")
        in_size = fun_dim + (ref ** 3 if unified_pos else space_dim)
        _dense_k(in_size, "the preprocess MLP" + (" (node features + ref^3 grid distances)" if unified_pos else ""))
        if n_hidden * mlp_ratio not in _DENSE_K:
            raise NotImplementedError(f"Transolver on the HIP dense kernels: hidden_size * mlp_ratio must be one of {_DENSE_K}, got {n_hidden * mlp_ratio}")
        if out_dim > _DENSE_K[-1]:
            raise NotImplementedError(f"Transolver on the HIP dense kernels: output_size at most {_DENSE_K[-1]}, got {out_dim}")
        if use_temporal_block and n_head not in _TEMPORAL_HEADS:
            raise NotImplementedError(f"Transolver with use_temporal_block: the temporal block's kernels take num_heads in {_TEMPORAL_HEADS}, got {n_head}")
        self.preprocess = build_mlp(in_size=in_size, hidden_size=n_hidden * 2, out_size=n_hidden, nb_of_layers=2, layer_norm=False, act=act)
        self.n_hidden, self.space_dim = n_hidden, space_dim
        self.embedding = nn.Linear(3, n_hidden)   # (the condition is always None: never used, never receives a gradient)
        kw = dict(num_heads=n_head, hidden_dim=n_hidden, dropout=dropout, act=act, mlp_ratio=mlp_ratio, out_dim=out_dim, slice_num=slice_num,
                  use_rope_embeddings=use_rope_embeddings, rope_pos_dimension=rope_pos_dimension, rope_base=rope_base,
                  use_gated_attention=use_gated_attention)
        if use_temporal_block:   # no block is "last": output_proj follows the temporal block
            self.blocks = nn.ModuleList([Transolver_plus_block(**kw, last_layer=False) for _ in range(n_layers)])
            self.output_proj = nn.Linear(n_hidden, out_dim)
        else:
            self.blocks = nn.ModuleList([Transolver_plus_block(**kw, last_layer=(i == n_layers - 1)) for i in range(n_layers)])
            self.output_proj = None
        self.placeholder = nn.Parameter((1 / n_hidden) * torch.rand(n_hidden, dtype=torch.float))
        if use_temporal_block:
            from .transformer import TemporalAttention
            self.temporal_block = TemporalAttention(hidden_size=n_hidden, num_heads=n_head, use_gate=use_gated_attention)
        else:
            self.temporal_block = None
        self.n_head, self.slice_num = n_head, slice_num
        self.noise_seed = 0
        self.noise_u: Optional[List[torch.Tensor]] = None
        self.backend = "auto"
        #: the call counter of the noise stream: every forward reads it and advances it ON THE STREAM (a replayed graph keeps counting)
        self.register_buffer("_noise_step", torch.zeros(1, dtype=torch.int64), persistent=False)
        self._cpu_generator = None

    def get_grid(self, pos: torch.Tensor) -> torch.Tensor:
        """distances [N, ref^3] of the 3-D positions to the fixed reference grid (transolver.py:329-359), plain torch ops"""
        if pos.size(-1) != 3:
            raise ValueError(f"unified_pos needs 3-D node positions, got {pos.size(-1)} columns")
        axes = [torch.tensor(np.linspace(a, b, self.ref), dtype=torch.float) for a, b in ((-1.5, 1.5), (0, 2), (-4, 4))]
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(self.ref ** 3, 3).to(pos.device)
        return torch.sqrt(torch.sum((pos[:, None, :] - grid[None, :, :]) ** 2, dim=-1)).contiguous()

    def _uniforms(self, layer: int, N: int, step: torch.Tensor, dev) -> torch.Tensor:
        """the torch-ops path's u: the device stream on the device, a seeded host generator on the CPU"""
        H, G = self.n_head, self.slice_num
        if dev.type == "cuda":
            return slice_uniforms(self.noise_seed, step, layer, N, H, G)
        if self._cpu_generator is None:
            self._cpu_generator = torch.Generator().manual_seed(int(self.noise_seed))
        return torch.rand(N, H, G, generator=self._cpu_generator)

    def forward(self, x, pos, condition=None):
        if condition is not None:
            raise NotImplementedError("Transolver: a global condition vector is not built (TransolverProcessor always passes None)")
        if self.use_rope_embeddings and pos is None:
            raise ValueError("use_rope_embeddings=True requires node positions for Transolver.")
        hip = bool(x.is_cuda) and self.backend == "auto"
        if self.backend not in ("auto", "torch"):
            raise ValueError(f"Model.backend: 'auto' or 'torch', got {self.backend!r}")
        if x.is_cuda and ops.get_matrix_precision() == "bf16":
            raise NotImplementedError("Transolver runs in fp32: the bf16 matrix mode (enable_vram_optimizations) is not built for it")
        N = int(x.shape[0])
        if pos is not None and self.unified_pos:
            x = torch.cat((x, self.get_grid(pos)), dim=-1)
        if self.noise_u is not None and len(self.noise_u) != len(self.blocks):
            raise ValueError(f"Model.noise_u: one tensor per block ({len(self.blocks)}), got {len(self.noise_u)}")
        step = self._noise_step.clone()   # this call's counter value, kept for the backward
        self._noise_step.add_(1)
        fx = _linear(_linear(x, self.preprocess[0], act="gelu", hip=hip), self.preprocess[2], hip=hip)
        fx = fx + self.placeholder[None, :]
        prev_fx = fx
        for i, block in enumerate(self.blocks):
            prev_fx = fx
            u = self.noise_u[i].to(device=x.device, dtype=torch.float32).reshape(N, self.n_head, self.slice_num) if self.noise_u is not None else None
            if u is None and not hip:
                u = self._uniforms(i, N, step, x.device)
            fx = block(fx, pos=pos, ctl=dict(hip=hip, u=u, step=step, seed=int(self.noise_seed) & (2 ** 64 - 1), layer=i))
        if self.temporal_block is not None:
            # (the temporal block has engine launches only: it runs on them for every device tensor, whatever `backend` says)
            fx = self.temporal_block(prev_fx, fx, None) if x.is_cuda else _temporal_torch(self.temporal_block, prev_fx, fx)
            fx = _linear(fx, self.output_proj, hip=bool(x.is_cuda))
        return fx


class TransolverProcessor(nn.Module):
    """processors.py:387-461: ``forward(graph)`` runs :class:`Model` on ``graph.x`` and ``graph.pos`` with no condition and
    ``space_dim = 0``; same constructor signature as the reference.  ``noise_seed``, ``noise_u`` and ``backend`` forward to the model."""

    def __init__(self, message_passing_num: int, node_input_size: int, output_size: int, hidden_size: int = 64, num_heads: int = 2,
                 dropout: float = 0.0, mlp_ratio: int = 1, slice_num: int = 32, ref: int = 8, unified_pos: bool = False,
                 use_rope_embeddings: bool = False, use_gated_attention: bool = False, rope_pos_dimension: int = 3, rope_base: float = 10000.0,
                 use_temporal_block: bool = False):
        super().__init__()
        self.hidden_size = hidden_size
        self.use_rope_embeddings = use_rope_embeddings
        self.model = Model(space_dim=0, n_layers=message_passing_num, n_hidden=hidden_size, dropout=dropout, n_head=num_heads, act="gelu",
                           mlp_ratio=mlp_ratio, fun_dim=node_input_size, out_dim=output_size, slice_num=slice_num, ref=ref, unified_pos=unified_pos,
                           use_rope_embeddings=use_rope_embeddings, use_gated_attention=use_gated_attention, rope_pos_dimension=rope_pos_dimension,
                           rope_base=rope_base, use_temporal_block=use_temporal_block)

    noise_seed = property(lambda self: self.model.noise_seed, lambda self, v: setattr(self.model, "noise_seed", int(v)))
    noise_u = property(lambda self: self.model.noise_u, lambda self, v: setattr(self.model, "noise_u", v))
    backend = property(lambda self: self.model.backend, lambda self, v: setattr(self.model, "backend", v))

    def forward(self, graph) -> torch.Tensor:
        pos = getattr(graph, "pos", None)
        if self.use_rope_embeddings and pos is None:
            raise ValueError("use_rope_embeddings=True requires 'pos' attribute in the input graph.")
        return self.model(graph.x, pos, None)
