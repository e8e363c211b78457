"""The ``"loss"`` section of a training config (graphphysics/utils/loss.py:19-494 on top of
utils/vectorial_operators.py:5-217): three pointwise losses on the normalised network output, five physics losses on the
nodal spatial gradient of the PHYSICAL fields, and ``MultiLoss``, their fixed-weight sum.

The nodal gradient ``G [N, F, D]`` of a field ``U [N, F]`` is a fixed sparse linear operator on ``U``:

  * ``finite_diff``   -- ``G[n] = (sum_{m in nbr(n)} (U[m] - U[n]) (x) c_nm) / (sum_m w_nm + 1e-8)`` over the de-duplicated
    symmetric closure of ``edge_index``, ``w = 1 / (|dx|^2 + 1e-8)``, ``c_nm = dx_nm w_nm / (|dx_nm|^2 + 1e-8)`` (the per-node form
    of the reference's two ``index_add_`` over the unique undirected pairs; a self pair adds ``2 w`` to the weight sum only);
  * ``least_squares`` -- per element of ``graph.face`` the least-squares gradient ``pinv(P[1:] - P[0])`` applied to the corner
    values, averaged onto the nodes with the element measures as weights.

so the geometry part (``LossGeometry``) is computed once per mesh, in fp64, and the per-step part is two gather passes.  On
device tensors the whole section is ONE autograd node on the engine's kernels (``mgn_loss_fwd`` / ``mgn_loss_bwd``: no
``[E, F, D]`` tensor, no float atomics, no host synchronisation); on CPU tensors, and under ``MGN_TORCH_LOSS``, the same formulas
run as plain torch ops -- the restatement the tests pin to the reference."""
from __future__ import annotations

import ctypes as C
import enum
import os
from typing import Optional, Sequence

import torch
from torch.nn.modules.loss import _Loss

from ._launch import call
from .nodetype import PREDICTED

GRADIENT_METHODS = ("finite_diff", "least_squares")
_EPS = 1e-8

# term codes of include/mgn_hip.h (MGN_LOSS_*)
_L2, _COSINE, _L1SMOOTH, _GRADIENT, _CONVECTION, _DIV_L2, _DIV_L1, _DIV_L1SMOOTH = range(8)


def check_gradient_method(method: str) -> str:
    m = str(method).lower()
    if m not in GRADIENT_METHODS:
        raise ValueError(f"gradient_method: unknown method '{method}' (one of {', '.join(GRADIENT_METHODS)})")
    return m


def _use_kernels(t: torch.Tensor) -> bool:
    return t.is_cuda and os.environ.get("MGN_TORCH_LOSS") is None


# ================================================================================ geometry
class LossGeometry:
    """What the nodal-gradient operator of one mesh needs, computed once: for ``finite_diff`` the de-duplicated symmetric
    neighbour CSR (``rowptr`` int64, ``col`` int32, ``row`` for the torch path), ``coef [nnz, D]`` and ``inv [N]``; for
    ``least_squares`` the elements ``[M, K]``, ``cv [M, K, D]`` (= columns of ``pinv(A)`` times the element measure; corner 0
    carries minus the sum), the node -> (element, corner) inverted index and ``inv [N] = 1 / clamp(sum of measures, 1e-12)``.
    Coefficients are computed in fp64 and stored as fp32, without ever forming ``A A^T``.

    The object is pinned on the graph as ``graph.mgn_loss_geometry`` (``for_graph``) and found there, never by a data pointer:
    it is a snapshot of ``graph.pos`` and the topology at build time.  WRITING NEW POSITIONS INTO THE SAME GRAPH OBJECT DOES NOT
    UPDATE IT -- a deformed mesh needs ``LossGeometry(graph, method)`` again (or a new graph object, which gets a fresh build).
    Building synchronises with the host (index validation, ``unique``), so it happens in eager code, never inside a capture."""

    #: number of geometry builds so far (tests assert "built once" on it)
    builds = 0

    def __init__(self, graph, method: str):
        self.method = check_gradient_method(method)
        pos = graph.pos
        if pos is None:
            raise ValueError("the physics losses need graph.pos")
        if pos.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LossGeometry cannot be built inside a graph capture: build it in an eager step first")
        self.device = pos.device
        self.N, self.D = int(pos.shape[0]), int(pos.shape[1])
        if not 1 <= self.D <= 3:
            raise ValueError("graph.pos must have 1..3 columns")
        self.pos = pos.detach().to(torch.float32).contiguous().clone()
        kernels = _use_kernels(self.pos)
        if self.method == "finite_diff":
            self._build_finite_diff(graph, kernels)
        else:
            self._build_least_squares(graph, kernels)
        LossGeometry.builds += 1

    @staticmethod
    def for_graph(graph, method: str) -> "LossGeometry":
        """the geometry pinned on ``graph`` (built and pinned on first use)"""
        method = check_gradient_method(method)
        g = graph.__dict__.get("mgn_loss_geometry") if hasattr(graph, "__dict__") else None
        if isinstance(g, LossGeometry) and g.method == method and g.N == int(graph.pos.shape[0]):
            return g
        g = LossGeometry(graph, method)
        graph.mgn_loss_geometry = g
        return g

    # ---------------------------------------------------------------- finite differences
    def _build_finite_diff(self, graph, kernels: bool):
        ei, N, dev = graph.edge_index, self.N, self.device
        if ei is None:
            raise ValueError("gradient_method 'finite_diff' needs graph.edge_index")
        ei = ei.to(dev).long()
        if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= N):
            raise ValueError("edge_index holds a node outside [0, N)")
        lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
        key = torch.unique(lo * N + hi)   # the unique undirected pairs (vectorial_operators.py:97)
        lo, hi = key // N, key % N
        is_self = lo == hi
        self.self_loop = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.self_loop[lo[is_self]] = 1
        lo, hi = lo[~is_self], hi[~is_self]
        rows, cols = torch.cat([lo, hi]), torch.cat([hi, lo])
        order = torch.argsort(rows * N + cols)   # distinct keys: one possible order
        rows, cols = rows[order], cols[order]
        self.row = rows
        self.col = cols.to(torch.int32).contiguous()
        self.rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
        nnz = int(rows.numel())
        if kernels:
            self.coef = torch.empty(nnz, self.D, dtype=torch.float32, device=dev)
            self.inv = torch.empty(N, dtype=torch.float32, device=dev)
            call("mgn_loss_fd_geometry", dev, self.rowptr.data_ptr(), self.col.data_ptr(), self.self_loop.data_ptr(),
                 self.pos.data_ptr(), self.D, N, self.coef.data_ptr(), self.inv.data_ptr())
        else:
            p = self.pos.double()
            dx = p[cols] - p[rows]
            w = 1.0 / ((dx * dx).sum(1) + _EPS)
            wsum = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, rows, w) + self.self_loop.double() * (2.0 / _EPS)
            self.coef = (dx * (w * w)[:, None]).float().contiguous()
            self.inv = (1.0 / (wsum + _EPS)).float()

    # ---------------------------------------------------------------- least squares
    def _build_least_squares(self, graph, kernels: bool):
        face, N, D, dev = graph.face, self.N, self.D, self.device
        if face is None:
            raise ValueError("gradient_method 'least_squares' needs graph.face (the mesh's triangles or tetrahedra)")
        elems = face.to(dev).long().T.contiguous()   # [M, K]
        M, K = int(elems.shape[0]), int(elems.shape[1])
        if not ((K == 3 and D in (2, 3)) or (K == 4 and D == 3)):
            raise ValueError(f"least_squares: elements of {K} corners in {D}-D are not supported (triangles in 2-D / 3-D, tetrahedra in 3-D)")
        if M and (int(elems.min()) < 0 or int(elems.max()) >= N):
            raise ValueError("face holds a node outside [0, N)")
        if M * K >= 2 ** 31:
            raise ValueError("least_squares: too many element corners for 32-bit entries")
        flat = elems.reshape(-1)
        order = torch.sort(flat, stable=True)[1]
        self.M, self.K = M, K
        self.elems = elems.to(torch.int32).contiguous()
        self.nent = order.to(torch.int32).contiguous()   # entry e * K + k
        self.nptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        self.nptr[1:] = torch.cumsum(torch.bincount(flat, minlength=N), 0)
        self.corner_node = flat   # torch path: node of every (e, k)
        if kernels:
            self.cv = torch.empty(M, K, D, dtype=torch.float32, device=dev)
            self.inv = torch.empty(N, dtype=torch.float32, device=dev)
            vol = torch.empty(max(M, 1), dtype=torch.float64, device=dev)
            call("mgn_loss_ls_geometry", dev, self.elems.data_ptr(), M, K, self.pos.data_ptr(), D, N, self.nptr.data_ptr(),
                 self.nent.data_ptr(), self.cv.data_ptr(), vol.data_ptr(), self.inv.data_ptr())
        else:
            P = self.pos.double()[elems]               # [M, K, D]
            A = P[:, 1:, :] - P[:, :1, :]              # [M, S, D]
            if K == 4:
                vol = torch.linalg.det(A).abs() / 6.0
            elif D == 2:
                vol = 0.5 * (A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]).abs()
            else:
                vol = 0.5 * torch.linalg.cross(A[:, 0], A[:, 1], dim=1).norm(dim=1)
            Cm = torch.linalg.pinv(A) if M else A.new_zeros(0, D, K - 1)   # [M, D, S], fp64 SVD
            Cm = torch.where((vol > 0)[:, None, None], Cm, torch.zeros_like(Cm))
            cv = torch.empty(M, K, D, dtype=torch.float64, device=dev)
            cv[:, 1:, :] = Cm.transpose(1, 2) * vol[:, None, None]
            cv[:, 0, :] = -cv[:, 1:, :].sum(1)
            self.cv = cv.float().contiguous()
            vs = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, flat, vol.repeat_interleave(K))
            self.inv = (1.0 / vs.clamp(min=1e-12)).float()

    # ---------------------------------------------------------------- torch statement of the operator
    def gradient(self, field: torch.Tensor) -> torch.Tensor:
        """``G [N, F, D]`` of ``field [N, F]`` as plain torch ops (differentiable)"""
        if field.dim() == 1:
            field = field.unsqueeze(1)
        N, F, D = self.N, int(field.shape[1]), self.D
        dt = field.dtype
        if self.method == "finite_diff":
            du = field[self.col.long()] - field[self.row]
            contrib = du.unsqueeze(2) * self.coef.to(dt).unsqueeze(1)
            g = torch.zeros(N, F, D, dtype=dt, device=field.device).index_add_(0, self.row, contrib)
        else:
            ue = field[self.elems.long()]                               # [M, K, F]
            # grad_e * vol_e from the differences to corner 0 (cv[:, 0] is minus the sum of the others): exact differences first
            ge = torch.einsum("mkf,mkd->mfd", ue[:, 1:] - ue[:, :1], self.cv[:, 1:].to(dt))
            g = torch.zeros(N, F, D, dtype=dt, device=field.device).index_add_(0, self.corner_node, ge.repeat_interleave(self.K, dim=0))
        return g * self.inv.to(dt).view(-1, 1, 1)


def compute_gradient(graph, field: torch.Tensor, method: str = "least_squares", device=None) -> torch.Tensor:
    """nodal spatial gradient ``[N, F, D]`` of ``field`` (vectorial_operators.py:131-154); the geometry is cached on ``graph``"""
    geom = LossGeometry.for_graph(graph, method)
    if field.dim() == 1:
        field = field.unsqueeze(1)
    if _use_kernels(field) and field.shape[1] <= 4 and not (torch.is_grad_enabled() and field.requires_grad):
        u = field.detach().float().contiguous()
        N = int(u.shape[0])
        nt = torch.zeros(N, dtype=torch.float32, device=u.device)
        g_out = torch.empty(N, u.shape[1], geom.D, dtype=torch.float32, device=u.device)
        _launch_fwd(u, u, nt, u, u, geom, (_GRADIENT,), (1.0,), (0,), g_out=g_out)
        return g_out
    return geom.gradient(field)


# ================================================================================ the torch formulas
def _mask_of(node_type: torch.Tensor, masks: Sequence[int]) -> torch.Tensor:
    mask = node_type == int(masks[0])
    for t in masks[1:]:
        mask = torch.logical_or(mask, node_type == int(t))
    return mask


def _exclude_of(selected_indexes, n: int, device) -> Optional[torch.Tensor]:
    """``[n]`` uint8, 1 on the rows ``selected_indexes`` lists (the reference's ``~isin(arange(n), selected_indexes)``,
    loss.py:19-34: the rows LISTED are LEFT OUT); entries outside ``[0, n)`` and repeated entries change nothing.  ``None`` or an
    empty tensor: ``None``.  Torch ops only, no host synchronisation."""
    if selected_indexes is None:
        return None
    sel = torch.as_tensor(selected_indexes, device=device).reshape(-1).long()
    if sel.numel() == 0:
        return None
    ex = torch.zeros(n + 1, dtype=torch.uint8, device=device)   # slot n swallows what is out of range
    ex[torch.where((sel >= 0) & (sel < n), sel, torch.full_like(sel, n))] = 1
    return ex[:n]


def _masked_mean(err: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """mean over all elements of the selected rows, without a data-dependent shape"""
    e = err.reshape(err.shape[0], -1)
    sel = torch.where(mask.unsqueeze(1), e, torch.zeros_like(e))
    return sel.sum() / (mask.to(e.dtype).sum() * e.shape[1])


def _smooth_l1(d: torch.Tensor, beta: float) -> torch.Tensor:
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)


def _term_torch(kind: int, beta: float, out, tgt, mask, u_out, u_tgt, g_out, g_tgt) -> torch.Tensor:
    if kind == _L2:
        return _masked_mean((out - tgt) ** 2, mask)
    if kind == _COSINE:
        ab, aa, bb = (out * tgt).sum(1), (out * out).sum(1) + 1e-12, (tgt * tgt).sum(1) + 1e-12
        return _masked_mean(1.0 - ab / torch.sqrt(aa * bb), mask)
    if kind == _L1SMOOTH:
        return _masked_mean(_smooth_l1(out - tgt, beta), mask)
    if kind == _GRADIENT:
        return _masked_mean((g_out - g_tgt) ** 2, mask)
    if kind == _CONVECTION:   # einsum "nf,nfd->nf": U[n, f] * sum_d G[n, f, d]
        return _masked_mean((u_out * g_out.sum(2) - u_tgt * g_tgt.sum(2)) ** 2, mask)
    div = g_out.diagonal(dim1=1, dim2=2).sum(-1)
    if kind == _DIV_L2:
        return _masked_mean(div ** 2, mask)
    if kind == _DIV_L1:
        return _masked_mean(div.abs(), mask)
    return _masked_mean(_smooth_l1(div, beta), mask)


# ================================================================================ the fused path
def _launch_fwd(net_out, target, node_type, u_out, u_tgt, geom, kinds, weights, masks, g_out=None, exclude=None):
    """fill an ``mgn_loss_args`` and run ``mgn_loss_fwd``; returns (args, tensors kept alive, terms, total)"""
    from . import _capi
    dev = net_out.device
    N, O = int(net_out.shape[0]), int(net_out.shape[1])
    a = _capi.LossArgs()
    keep = [net_out, target, node_type, u_out, u_tgt, geom]
    a.N, a.O = N, O
    a.net_out, a.ld_out = net_out.data_ptr(), int(net_out.stride(0)) if N else O
    a.target, a.ld_tgt = target.data_ptr(), int(target.stride(0)) if N else O
    a.type, a.ldty = node_type.data_ptr(), int(node_type.stride(0)) if N else 1
    if exclude is not None:
        a.exclude = exclude.data_ptr()
        keep.append(exclude)
    a.ntypes = len(masks)
    for i, t in enumerate(masks):
        a.types[i] = float(int(t))
    a.nterms = len(kinds)
    for i, (k, w) in enumerate(zip(kinds, weights)):
        a.term_type[i], a.term_weight[i] = int(k), float(w)
    L = _capi.lib()
    nf = (L.mgn_loss_workspace_bytes() + 3) // 4
    # one allocation: partial table | terms | total | 1 / count
    ws = torch.empty(nf + len(kinds) + 2, dtype=torch.float32, device=dev)
    terms, total, invc = ws[nf:nf + len(kinds)], ws[nf + len(kinds)], ws[nf + len(kinds) + 1]
    a.part, a.terms, a.total, a.invcount = ws.data_ptr(), terms.data_ptr(), total.data_ptr(), invc.data_ptr()
    b_out = torch.empty(N, O, dtype=torch.float32, device=dev)
    a.b_out = b_out.data_ptr()
    keep += [ws, b_out]
    if u_out is not None:
        F, D = int(u_out.shape[1]), geom.D
        a.F, a.DX = F, D
        a.u_out, a.u_tgt = u_out.data_ptr(), u_tgt.data_ptr()
        a_out, bu_out = torch.empty(N, F, D, dtype=torch.float32, device=dev), torch.empty(N, F, dtype=torch.float32, device=dev)
        a.a_out, a.bu_out, a.inv = a_out.data_ptr(), bu_out.data_ptr(), geom.inv.data_ptr()
        keep += [a_out, bu_out]
        if geom.method == "finite_diff":
            a.method = 0
            a.rowptr, a.col, a.coef = geom.rowptr.data_ptr(), geom.col.data_ptr(), geom.coef.data_ptr()
        else:
            a.method = 1
            a.M, a.K = geom.M, geom.K
            a.elems, a.cv, a.nptr, a.nent = geom.elems.data_ptr(), geom.cv.data_ptr(), geom.nptr.data_ptr(), geom.nent.data_ptr()
            ge = torch.empty(2, max(geom.M, 1), F, D, dtype=torch.float32, device=dev)
            a.ge_out, a.ge_tgt = ge[0].data_ptr(), ge[1].data_ptr()
            keep.append(ge)
        if g_out is not None:
            a.g_out = g_out.data_ptr()
            keep.append(g_out)
    call("mgn_loss_fwd", dev, C.byref(a))
    return a, keep, terms, total


class _FusedLossFn(torch.autograd.Function):
    """the whole ``loss`` section as one autograd node: ``(total, weighted terms)`` from the normalised rows and the physical
    fields; gradients into ``net_out`` (pointwise terms) and ``u_out`` (physics terms)"""

    @staticmethod
    def forward(ctx, net_out, target, node_type, u_out, u_tgt, geom, kinds, weights, masks, exclude=None):
        f32 = lambda t: t if t.dtype == torch.float32 else t.float()   # noqa: E731
        rows = lambda t: t if t.stride(-1) == 1 else t.contiguous()    # noqa: E731
        net_out, target, node_type = rows(f32(net_out)), rows(f32(target)), f32(node_type)
        N = int(net_out.shape[0])
        if target.shape != net_out.shape or int(node_type.shape[0]) != N:
            raise ValueError("loss: output, target and node_type must describe the same rows")
        if u_out is not None:
            u_out, u_tgt = f32(u_out).contiguous(), f32(u_tgt).contiguous()
            if u_out.shape != u_tgt.shape or int(u_out.shape[0]) != N or geom.N != N:
                raise ValueError("loss: the physical fields and the geometry must describe the same nodes")
            if not 1 <= int(u_out.shape[1]) <= 4:
                raise ValueError("loss: the physics kernels take fields of 1..4 columns")
        if exclude is not None and (exclude.dtype != torch.uint8 or exclude.shape != (N,) or not exclude.is_contiguous()):
            raise ValueError("loss: exclude must be a contiguous uint8 tensor of one entry per row")
        a, keep, terms, total = _launch_fwd(net_out, target, node_type, u_out, u_tgt, geom, kinds, weights, masks, exclude=exclude)
        ctx.args, ctx.keep = a, keep
        ctx.shape = (N, int(net_out.shape[1]), int(u_out.shape[1]) if u_out is not None else 0)
        ctx.geom = geom if u_out is not None else None
        ctx.pointwise = any(k < _GRADIENT for k in kinds)
        ctx.dev = net_out.device
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        N, O, F = ctx.shape
        dev = ctx.dev
        g = g.float().reshape(1).contiguous()
        need_net, need_u = ctx.needs_input_grad[0] and ctx.pointwise, ctx.needs_input_grad[3] and ctx.geom is not None
        d_net = torch.empty(N, O, dtype=torch.float32, device=dev) if need_net else None
        d_u = torch.empty(N, F, dtype=torch.float32, device=dev) if need_u else None
        dge = None
        if need_u and ctx.geom.method == "least_squares":
            dge = torch.empty(max(ctx.geom.M, 1), F, ctx.geom.D, dtype=torch.float32, device=dev)
        if need_net or need_u:
            call("mgn_loss_bwd", dev, C.byref(ctx.args), g.data_ptr(), d_net.data_ptr() if need_net else None,
                 d_u.data_ptr() if need_u else None, dge.data_ptr() if dge is not None else None)
        if ctx.needs_input_grad[0] and d_net is None:
            d_net = torch.zeros(N, O, dtype=torch.float32, device=dev)
        return d_net, None, None, d_u, None, None, None, None, None, None


def evaluate(kinds: Sequence[int], weights: Sequence[float], betas: Sequence[float], *, graph=None, target=None,
             network_output=None, node_type=None, masks=None, network_output_physical=None, target_physical=None,
             gradient_method=None, network_output_gradient=None, target_gradient=None, geometry: Optional[LossGeometry] = None,
             selected_indexes=None):
    """``(sum_t w_t loss_t, [w_t loss_t])`` for the terms ``kinds``.  Device tensors go through the engine's fused kernels (every
    term in one pass); CPU tensors, ``MGN_TORCH_LOSS``, a caller-supplied gradient tensor or a ``beta`` other than 1 take the torch
    formulas.  ``selected_indexes`` has the reference's meaning (loss.py:19-34): the rows it lists are left out of every term's
    mean, while their field values still feed their neighbours' nodal gradients."""
    masks = tuple(int(t) for t in (masks if masks is not None else PREDICTED))
    physics = any(k >= _GRADIENT for k in kinds)
    anchor = network_output if network_output is not None else network_output_physical
    if physics:
        if network_output_physical is None or (target_physical is None and any(k in (_GRADIENT, _CONVECTION) for k in kinds)):
            raise ValueError("a physics loss needs network_output_physical and target_physical")
        if target_physical is None:
            target_physical = network_output_physical.detach()
        if network_output_gradient is None and geometry is None:
            if gradient_method is None:
                raise ValueError("a physics loss needs gradient_method ('finite_diff' or 'least_squares')")
            geometry = LossGeometry.for_graph(graph, gradient_method)
    else:
        network_output_physical = target_physical = None
    if network_output is None:   # a physics loss called alone: nothing pointwise to read, the fields stand in for the row shapes
        network_output, target = network_output_physical, target_physical
    fused = (_use_kernels(anchor) and network_output_gradient is None and target_gradient is None and 1 <= len(masks) <= 4
             and len(kinds) <= 8 and all(float(b) == 1.0 for b in betas) and network_output.dim() == 2 and node_type.dim() == 1
             and (not physics or (network_output_physical.dim() == 2 and network_output_physical.shape[1] <= 4)))
    exclude = _exclude_of(selected_indexes, int(node_type.shape[0]), node_type.device)
    if fused:
        total, terms = _FusedLossFn.apply(network_output, target, node_type, network_output_physical, target_physical,
                                          geometry if physics else None, tuple(kinds), tuple(float(w) for w in weights), masks, exclude)
        return total, list(terms.unbind(0))
    mask = _mask_of(node_type, masks)
    if exclude is not None:
        mask = torch.logical_and(mask, exclude == 0)
    g_out = g_tgt = None
    if physics:
        g_out = network_output_gradient if network_output_gradient is not None else geometry.gradient(network_output_physical)
        if any(k in (_GRADIENT, _CONVECTION) for k in kinds):
            g_tgt = target_gradient if target_gradient is not None else geometry.gradient(target_physical)
    terms = [w * _term_torch(k, b, network_output, target, mask, network_output_physical, target_physical, g_out, g_tgt)
             for k, w, b in zip(kinds, weights, betas)]
    return sum(terms), terms


# ================================================================================ the loss objects
class _Term(_Loss):
    """one loss type; callable with the reference's keyword set"""
    kind = _L2
    _name = ""
    beta = 1.0

    @property
    def __name__(self):
        return self._name

    def forward(self, graph=None, target=None, network_output=None, node_type=None, masks=None, selected_indexes=None,
                network_output_physical=None, target_physical=None, gradient_method=None, network_output_gradient=None,
                target_gradient=None, **kwargs) -> torch.Tensor:
        if selected_indexes is not None and torch.as_tensor(selected_indexes).numel() == 0:
            selected_indexes = None   # nothing listed: the call without the argument
        if self.kind == _L2 and network_output is not None and selected_indexes is None:   # the engine's existing masked-MSE path, unchanged
            from .harness import l2_loss
            return l2_loss(network_output, target, node_type, tuple(masks) if masks is not None else PREDICTED)
        total, _ = evaluate((self.kind,), (1.0,), (self.beta,), graph=graph, target=target, network_output=network_output,
                            node_type=node_type, masks=masks, network_output_physical=network_output_physical,
                            target_physical=target_physical, gradient_method=gradient_method,
                            network_output_gradient=network_output_gradient, target_gradient=target_gradient,
                            selected_indexes=selected_indexes)
        return total


class L2Loss(_Term):
    kind, _name = _L2, "MSE"


class CosineLoss(_Term):
    kind, _name = _COSINE, "Cosine"


class L1SmoothLoss(_Term):
    kind, _name = _L1SMOOTH, "L1Smooth"

    def __init__(self, beta: float = 1.0, **kwargs):
        super().__init__(**kwargs)
        self.beta = beta


class GradientL2Loss(_Term):
    kind, _name = _GRADIENT, "GradientL2Loss"


class ConvectionL2Loss(_Term):
    kind, _name = _CONVECTION, "ConvectionL2Loss"


class DivergenceL2Loss(_Term):
    kind, _name = _DIV_L2, "DivergenceL2Loss"


class DivergenceL1Loss(_Term):
    kind, _name = _DIV_L1, "DivergenceL1Loss"


class DivergenceL1SmoothLoss(_Term):
    kind, _name = _DIV_L1SMOOTH, "DivergenceL1Smooth"

    def __init__(self, beta: float = 1.0, **kwargs):
        super().__init__(**kwargs)
        self.beta = beta


class MultiLoss(_Loss):
    """``sum_i w_i loss_i`` (loss.py:429-482); with ``return_all_losses`` also the list of the WEIGHTED terms.  Both nodal
    gradients are formed once for all terms -- on device tensors inside the one fused pass."""

    def __init__(self, losses: Sequence[_Term], weights: Sequence[float], **kwargs):
        super().__init__(**kwargs)
        losses, weights = list(losses), list(weights)
        if len(weights) != len(losses):
            raise ValueError(f"loss.weights: {len(weights)} weights for {len(losses)} loss types")
        if not 1 <= len(losses) <= 8:
            raise ValueError("loss.type: 1..8 loss types")
        for l in losses:
            if not isinstance(l, _Term):
                raise ValueError("loss.type: MultiLoss takes the loss objects of this module")
        self.losses = losses
        self.weights = weights

    @property
    def __name__(self):
        return "MultiLoss"

    @property
    def needs_physical_fields(self) -> bool:
        return any(l.kind >= _GRADIENT for l in self.losses)

    def forward(self, graph=None, network_output_physical=None, target_physical=None, gradient_method=None,
                return_all_losses: bool = False, geometry: Optional[LossGeometry] = None, **kwargs):
        total, terms = evaluate([l.kind for l in self.losses], self.weights, [l.beta for l in self.losses], graph=graph,
                                target=kwargs.get("target"), network_output=kwargs.get("network_output"),
                                node_type=kwargs.get("node_type"), masks=kwargs.get("masks"),
                                network_output_physical=network_output_physical, target_physical=target_physical,
                                gradient_method=gradient_method, geometry=geometry, selected_indexes=kwargs.get("selected_indexes"))
        return (total, terms) if return_all_losses else total


class LossType(enum.Enum):
    L2LOSS = L2Loss
    COSINEL2LOSS = CosineLoss
    L1SMOOTHLOSS = L1SmoothLoss
    GRADIENTL2LOSS = GradientL2Loss
    CONVECTIONL2LOSS = ConvectionL2Loss
    DIVERGENCEL2LOSS = DivergenceL2Loss
    DIVERGENCEL1LOSS = DivergenceL1Loss
    DIVERGENCEL1SMOOTHLOSS = DivergenceL1SmoothLoss


#: loss types that read the physical fields and their nodal gradient
PHYSICS_LOSSES = (LossType.GRADIENTL2LOSS, LossType.CONVECTIONL2LOSS, LossType.DIVERGENCEL2LOSS, LossType.DIVERGENCEL1LOSS,
                  LossType.DIVERGENCEL1SMOOTHLOSS)
