"""Training-step and rollout loops that reproduce the semantics of the reference's
LightningModule for the MeshGraphNet path without Lightning (not installed on the
GPU box):

  * training step  (training/lightning_module.py:270-320): Simulator forward,
    masked L2 on NORMAL|OUTFLOW nodes (utils/loss.py:37-75, default masks
    lightning_module.py:48), backward, clip-grad-norm 1.0 (train.py:288),
    AdamW(lr, betas=(0.9,0.95), weight_decay=1e-4) + cosine warm-up
    (lightning_module.py:494-511, utils/scheduler.py:51-67);
  * rollout  (lightning_module.py:375-409): autoregressive feedback of the last
    prediction (with ``use_previous_data`` also of ``prediction - current output``),
    ground truth re-imposed on the non NORMAL/OUTFLOW nodes;
  * validation  (lightning_module.py:411-492): ``Engine.validate``, the rollout plus
    ``val_loss`` / ``val_all_rollout_rmse`` / ``val_1step_rmse`` from sums kept on the device.

These are what ``bench.py`` times ("training steps/sec", "rollout nodes*steps/sec").
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence

import torch

from .mesh import Graph
from .processors import EncodeProcessDecode
from .nodetype import NodeType
from .parse_parameters import (get_gradient_method, get_loss, get_model, get_simulator, get_spatial_mtp, get_transolver,
                               matrix_precision_from_config)
from .losses import L2Loss, LossGeometry, MultiLoss
from . import ops as _ops
from ._launch import call, stream_object


def lr_factor(last_epoch: int, warmup: int, max_iters: int, min_lr_factor: float = 0.001) -> float:
    epoch = last_epoch + 1
    f = 0.5 * (1 + math.cos(math.pi * epoch / max_iters))
    if epoch <= warmup:
        f *= epoch * 1.0 / warmup
    return max(f, min_lr_factor)


class _MaskedMseFn(torch.autograd.Function):
    """the loss below as two engine launches forward and one backward (``mgn_masked_mse_fwd`` / ``_bwd``) instead of torch's ~20
    elementwise / reduction launches -- 1-2 % of the batch-16 step, 4 % of the one-mesh step"""

    @staticmethod
    def forward(ctx, out, tgt, node_type, types):
        import ctypes as C
        out = out.float() if out.dtype != torch.float32 else out
        tgt = tgt.float() if tgt.dtype != torch.float32 else tgt
        node_type = node_type.float() if node_type.dtype != torch.float32 else node_type
        if out.stride(-1) != 1:
            out = out.contiguous()
        if tgt.stride(-1) != 1:
            tgt = tgt.contiguous()
        N, O = int(out.shape[0]), int(out.shape[1])
        if tgt.shape != out.shape or int(node_type.shape[0]) != N:
            raise ValueError("l2_loss: output, target and node_type must describe the same rows")
        dev = out.device
        scratch = torch.empty(514, dtype=torch.float32, device=dev)   # 512 partials | unused | 1 / (rows x O) for the backward
        loss, inv = torch.empty((), dtype=torch.float32, device=dev), scratch[513]
        tarr = (C.c_float * len(types))(*[float(t) for t in types])
        ldty = int(node_type.stride(0)) if N > 0 else 1
        call("mgn_masked_mse_fwd", dev, out.data_ptr(), int(out.stride(0)), tgt.data_ptr(), int(tgt.stride(0)), node_type.data_ptr(), ldty,
             N, O, tarr, len(types), scratch.data_ptr(), loss.data_ptr(), inv.data_ptr())
        ctx.save_for_backward(out, tgt, node_type, scratch)
        ctx.types = tuple(float(t) for t in types)
        return loss

    @staticmethod
    def backward(ctx, g):
        import ctypes as C
        out, tgt, node_type, scratch = ctx.saved_tensors
        N, O = int(out.shape[0]), int(out.shape[1])
        dev = out.device
        g = g.float().reshape(1).contiguous()
        d_out = torch.empty(N, O, dtype=torch.float32, device=dev)
        tarr = (C.c_float * len(ctx.types))(*ctx.types)
        ldty = int(node_type.stride(0)) if N > 0 else 1
        call("mgn_masked_mse_bwd", dev, out.data_ptr(), int(out.stride(0)), tgt.data_ptr(), int(tgt.stride(0)), node_type.data_ptr(), ldty,
             N, O, tarr, len(ctx.types), scratch[513].data_ptr(), g.data_ptr(), d_out.data_ptr())
        return d_out, None, None, None


def l2_loss(network_output: torch.Tensor, target: torch.Tensor, node_type: torch.Tensor,
            masks: Sequence[int] = (NodeType.NORMAL, NodeType.OUTFLOW)) -> torch.Tensor:
    """mean squared error over the rows whose node type is in ``masks`` (graphphysics/training/loss.py:70-75 with the masks of
    lightning_module.py:27-35); on the device one fused engine call, on the CPU (host-logic tests) the plain torch formula"""
    import os as _os
    if network_output.is_cuda and network_output.dim() == 2 and node_type.dim() == 1 and 1 <= len(masks) <= 4 and \
            _os.environ.get("MGN_TORCH_LOSS") is None:
        return _MaskedMseFn.apply(network_output, target, node_type, tuple(int(t) for t in masks))
    mask = node_type == int(masks[0])
    for t in masks[1:]:
        mask = torch.logical_or(mask, node_type == int(t))
    # mean over the selected rows' elements, without a data-dependent shape (no host sync)
    w = mask.to(network_output.dtype).unsqueeze(1)
    err = (network_output - target) ** 2 * w
    return err.sum() / (w.sum() * network_output.shape[1])


def build_mask(node_type: torch.Tensor) -> torch.Tensor:
    keep = torch.logical_or(node_type == int(NodeType.NORMAL), node_type == int(NodeType.OUTFLOW))
    return torch.logical_not(keep)


class FusedClipAdamW:
    """clip_grad_norm_(max_norm) + AdamW(lr, betas, eps, weight_decay) of the reference's training
    step (train.py:288, lightning_module.py:494-511) as ONE engine call (``mgn_clip_adamw``: two
    launches per 96 tensors instead of ~25 multi-tensor launches).  ``lr`` and the step counter are
    device scalars, so the same object works under hipGraph replay.  After ``step()`` the ``.grad``
    tensors hold the clipped gradients, as after ``clip_grad_norm_``."""

    def __init__(self, params, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-4,
                 max_norm: float = 1.0):
        from . import _capi
        self._capi = _capi
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        self.device = dev
        self.betas, self.eps, self.weight_decay, self.max_norm = betas, eps, weight_decay, max_norm
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.step_t = torch.zeros((), dtype=torch.float32, device=dev)
        self.lr_t = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        self.norm_t = torch.zeros((), dtype=torch.float32, device=dev)
        self.param_groups = [{"lr": float(lr)}]
        self._ws = None
        self._table, self._table_key = None, None   # device table of the tensors' fixed fields (mgn_clip_adamw_table)

    def set_lr(self, lr: float):
        self.param_groups[0]["lr"] = float(lr)
        self.lr_t.fill_(float(lr))

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        C = self._capi
        live = [(p, m, v) for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq) if p.grad is not None]
        arr = (C.OptTensor * len(live))()
        for i, (p, m, v) in enumerate(live):
            if not p.grad.is_contiguous():  # e.g. the un-padded slice of an encoder's first-layer gradient
                p.grad = p.grad.contiguous()
            if not p.data.is_contiguous():
                raise RuntimeError("FusedClipAdamW needs contiguous parameters")
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        L = C.lib()
        need = L.mgn_clip_adamw_workspace_bytes(len(live), arr)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        # two launches whatever the number of tensors: parameter / moment pointers and lengths sit in a device table built once per
        # parameter set (a blocking copy: the first, eager step builds it -- before any capture), the gradient pointers travel as
        # kernel arguments (MGN_OPT_NO_TABLE: the 96-tensors-per-launch form, for A/B; same bits)
        import os as _os
        key = tuple((arr[i].p, arr[i].m, arr[i].v, arr[i].n) for i in range(len(live)))
        tb = L.mgn_clip_adamw_table_bytes(len(live), arr) if _os.environ.get("MGN_OPT_NO_TABLE") is None else 0
        if tb > 0:
            if self._table_key != key:
                with torch.cuda.device(self.device):
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("FusedClipAdamW: the parameter table must be built by an eager step before the capture")
                    self._table = torch.empty(tb, dtype=torch.uint8, device=self.device)
                    C.check(L.mgn_clip_adamw_table(len(live), arr, self._table.data_ptr(), tb), "mgn_clip_adamw_table")
                self._table_key = key
            call("mgn_clip_adamw_t", self.device, len(live), arr, self._table.data_ptr(), float(self.max_norm), self.lr_t.data_ptr(),
                 self.step_t.data_ptr(), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                 float(self.weight_decay), self.norm_t.data_ptr(), self._ws.data_ptr(), self._ws.numel())
        else:
            call("mgn_clip_adamw", self.device, len(live), arr, float(self.max_norm), self.lr_t.data_ptr(), self.step_t.data_ptr(),
                 float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                 self.norm_t.data_ptr(), self._ws.data_ptr(), self._ws.numel())


class Engine:
    """Model + simulator + optimiser for one device."""

    def __init__(self, param: Dict[str, Any], device: torch.device, learning_rate: float = 1e-4,
                 num_steps: int = 1000, warmup: int = 100, grad_clip: float = 1.0, loss_masks: Optional[Sequence[int]] = None,
                 use_previous_data: bool = False, previous_data_start: Optional[int] = None,
                 previous_data_end: Optional[int] = None, seed: int = 0):
        """``loss_masks`` (the LightningModule's ``masks``), ``use_previous_data``, ``previous_data_start`` and
        ``previous_data_end`` are the LightningModule's arguments of the same names (lightning_module.py:48-51).  ``seed`` keys the
        Engine's own random draws (the centres of ``training.use_spatial_mtp``)."""
        self.param, self.device = param, device
        self.mtp = get_spatial_mtp(param)   # the spatial-MTP settings, None when training.use_spatial_mtp is off (validated here)
        if self.mtp is not None and matrix_precision_from_config(param) == "bf16":
            raise NotImplementedError("training.use_spatial_mtp with training.enable_vram_optimizations: the spatial-MTP branch runs in "
                                      "fp32 only (the bf16 matrix mode is not built for it)")
        #: model.type "transolver": built by its own factory (get_model still refuses the type, see get_transolver)
        self.is_transolver = (param.get("model", {}) or {}).get("type", "") == "transolver"
        if self.is_transolver:
            if matrix_precision_from_config(param) == "bf16":
                raise NotImplementedError("model.type 'transolver' with training.enable_vram_optimizations: the slice attention runs in fp32 "
                                          "only (the bf16 matrix mode is not built for it)")
            if self.mtp is not None:
                raise NotImplementedError("model.type 'transolver' with training.use_spatial_mtp: the Transolver processor has no "
                                          "nodes_encoder / decode_module for the branch to hook")
        _ops.set_matrix_precision(matrix_precision_from_config(param))  # bf16-mixed <=> enable_vram_optimizations
        self.model = get_transolver(param) if self.is_transolver else get_model(param)
        if self.is_transolver:
            self.model.noise_seed = int(seed)   # keys the Gumbel noise stream of the slice attention
        self.sim = get_simulator(param, self.model, device)
        # the config's "loss" section (lightning_module.py:86-96); without one: the masked L2, on the code path it always took
        self.loss, self.loss_name = get_loss(param)
        self.gradient_method = get_gradient_method(param)
        self.loss_masks = tuple(loss_masks) if loss_masks is not None else (NodeType.NORMAL, NodeType.OUTFLOW)
        #: autoregressive feedback of ``prediction - current output`` into x[:, previous_data_start:previous_data_end]
        #: (lightning_module.py:383-386,400-401)
        self.use_previous_data = bool(use_previous_data)
        self.previous_data_start, self.previous_data_end = previous_data_start, previous_data_end
        if self.use_previous_data:
            self._check_previous_data()
        self._tail_part = None   # scratch of mgn_rollout_tail
        self._v_table = None     # (metrics [cap, 4] fp64, slot int32 [1], cap) of validate()
        self._f_steps = {}       # captured frame steps with the fused tail: "rollout" (previous data), "validate"
        #: per-term device scalars of the last step of a MultiLoss config, in the order of ``loss_name`` (what the reference logs as
        #: ``train_<name>``: the WEIGHTED terms); None for a single loss
        self.last_losses = None
        self.learning_rate, self.num_steps, self.warmup, self.grad_clip = learning_rate, num_steps, warmup, grad_clip
        #: the auxiliary branch of training.use_spatial_mtp (lightning_module.py:133-268), None when the key is off
        self.spatial_mtp = None
        self.last_mtp_stats = None   # device scalars of the last step: the module's stats plus sp_mtp/aux_loss
        self._mtp_hooks, self._mtp_H, self._mtp_H_neigh = (), None, None
        if self.mtp is not None:
            self._setup_spatial_mtp(seed)
        self.opt = self._make_optimizer(learning_rate, capturable=False)
        self.step_count = 0
        self.grad_sync = None  # set by distributed.DataParallel: callable(params) all-reducing .grad
        self._graph = None     # hipGraph of one training step (capture_train_step)

    def _make_optimizer(self, lr, capturable: bool):
        """AdamW(lr, betas=(0.9,0.95), weight_decay=1e-4) as the reference configures it
        (lightning_module.py:494-511); the fused multi-tensor implementation when the device
        supports it (one kernel instead of ~15 foreach launches over 296 tensors)."""
        kw = dict(lr=lr, weight_decay=0.0001, betas=(0.9, 0.95))
        params = self._train_params()
        import os as _os
        if params and params[0].is_cuda and all(p.dtype == torch.float32 for p in params) and _os.environ.get("MGN_TORCH_ADAMW") is None:
            if getattr(self, "opt", None) is not None and isinstance(self.opt, FusedClipAdamW):
                return self.opt  # already device-resident state: nothing to rebuild for graph capture
            return FusedClipAdamW(params, float(lr) if not torch.is_tensor(lr) else float(lr.item()), betas=kw["betas"],
                                  weight_decay=kw["weight_decay"], max_norm=self.grad_clip)
        if params and params[0].is_cuda:
            try:
                return torch.optim.AdamW(params, fused=True, capturable=capturable, **kw)
            except (RuntimeError, ValueError, TypeError):
                pass
        return torch.optim.AdamW(params, capturable=capturable, **kw) if capturable else torch.optim.AdamW(params, **kw)

    def _train_params(self) -> List[torch.nn.Parameter]:
        """what the optimiser steps and the clip takes ONE norm over: the simulator's parameters, then the spatial-MTP module's
        (the reference registers it as a submodule of the LightningModule: clipped and stepped together)"""
        params = list(self.sim.parameters())
        if self.spatial_mtp is not None:
            params += list(self.spatial_mtp.parameters())
        return params

    # ---------------------------------------------------------------- training.use_spatial_mtp (lightning_module.py:133-268)
    def _setup_spatial_mtp(self, seed: int):
        """``LightningModule._setup_spatial_mtp``: the module sized by the decoder's first Linear, a forward pre-hook on the decoder
        (its input = H) and a forward hook on the node encoder (its output = H_neigh)"""
        from .spatial_mtp import SpatialMTP1Hop
        out_head, node_encoder = getattr(self.model, "decode_module", None), getattr(self.model, "nodes_encoder", None)
        if not isinstance(out_head, torch.nn.Module):
            raise ValueError("Spatial MTP requires a processor with an output head nn.Module (expected 'decode_module').")
        if not isinstance(node_encoder, torch.nn.Module):
            raise ValueError("Spatial MTP requires a processor with an encoder nn.Module (expected 'nodes_encoder').")
        first = next((m for m in out_head.modules() if isinstance(m, torch.nn.Linear)), None)
        if first is None:
            raise ValueError("Unable to infer hidden size for Spatial MTP (no Linear layer in decode module).")
        cfg = self.mtp
        self.spatial_mtp = SpatialMTP1Hop(d_model=first.in_features, num_heads=cfg["spatial_mtp_num_heads"],
                                          num_layers=cfg["spatial_mtp_num_layers"], assume_undirected=cfg["spatial_mtp_assume_undirected"],
                                          max_neighbors=cfg["spatial_mtp_max_neighbors"]).to(self.device)
        self.spatial_mtp.seed = int(seed)
        self._mtp_head = out_head
        self._mtp_generator = torch.Generator(device=self.device)
        self._mtp_generator.manual_seed(int(seed))

        def capture_head_input(module, inputs):
            hidden = inputs[0]
            self._mtp_H = hidden.reshape(-1, hidden.size(-1)) if hidden.dim() > 2 else hidden

        def capture_nodeenc_output(module, inputs, outputs):
            self._mtp_H_neigh = outputs.reshape(-1, outputs.size(-1)) if outputs.dim() > 2 else outputs

        self._mtp_hooks = (out_head.register_forward_pre_hook(capture_head_input), node_encoder.register_forward_hook(capture_nodeenc_output))

    def remove_spatial_mtp_hooks(self):
        for h in self._mtp_hooks:
            h.remove()
        self._mtp_hooks = ()

    def _mtp_loss(self, batch: Graph, target: torch.Tensor, centers: Optional[torch.Tensor]):
        """``_compute_spatial_mtp_loss`` (lightning_module.py:240-268): (aux loss, stats) or (None, {}).  A model that renumbers the
        mesh for locality hands its encoder and decoder rows in ITS numbering, and each model has its own rule for when
        (``ops.get_topology`` for EncodeProcessDecode, ``transformer.get_attn_topology`` for EncodeTransformDecode; the temporal
        block of the former brings the rows back before the decoder).  So every forward records the rank its two hooked modules
        saw (``model.last_node_rank``), and the captured tensors are brought back to the caller's numbering with exactly those:
        centres, adjacency and target then all speak the batch's numbering."""
        H, Hn = self._mtp_H, self._mtp_H_neigh
        edge_index = getattr(batch, "edge_index", None)
        if H is None or edge_index is None or target is None or H.size(0) == 0:
            return None, {}
        N = int(H.size(0))
        ranks = getattr(self.model, "last_node_rank", None) or {}
        if ranks.get("decode_module") is not None:
            H = H.index_select(0, ranks["decode_module"])
        if Hn is not None and ranks.get("nodes_encoder") is not None:
            Hn = Hn.index_select(0, ranks["nodes_encoder"])
        topo = None
        if H.is_cuda and isinstance(self.model, EncodeProcessDecode) and self.spatial_mtp.assume_undirected:
            # the edge topology the model's forward just used (cached per edge_index) already holds the source-grouped CSR; a
            # renumbered one is in the engine's numbering, and other models build no such topology: the module then groups the
            # caller's edge_index itself, once per edge_index
            topo = getattr(batch, "mgn_topology", None)
            if topo is None:
                topo = _ops.get_topology(edge_index, N, pos=getattr(batch, "pos", None), renumber=True)
            if topo.node_order is not None:
                topo = None
        if centers is None:
            B = min(N, self.mtp["spatial_mtp_centers_per_step"])
            centers = torch.randperm(N, device=H.device, generator=self._mtp_generator)[:B]
        return self.spatial_mtp(H=H, edge_index=edge_index, centers=centers, out_head=self._mtp_head, target=target, H_neigh=Hn,
                                topology=topo, step=self.step_count)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """the simulator's weights under their own keys plus, with training.use_spatial_mtp, the module's under ``spatial_mtp.`` --
        where a checkpoint of the reference's LightningModule keeps them"""
        sd = dict(self.sim.state_dict())
        if self.spatial_mtp is not None:
            sd.update({"spatial_mtp." + k: v for k, v in self.spatial_mtp.state_dict().items()})
        return sd

    def load_state_dict(self, state: Dict[str, torch.Tensor], strict: bool = True):
        mtp = {k[len("spatial_mtp."):]: v for k, v in state.items() if k.startswith("spatial_mtp.")}
        rest = {k: v for k, v in state.items() if not k.startswith("spatial_mtp.")}
        if self.spatial_mtp is not None:
            self.spatial_mtp.load_state_dict(mtp, strict=strict)
        elif mtp and strict:
            raise RuntimeError("load_state_dict: the state holds spatial_mtp.* weights, this Engine was built without training.use_spatial_mtp")
        return self.sim.load_state_dict(rest, strict=strict)

    def _loss(self, batch: Graph, net_out: torch.Tensor, target: torch.Tensor, node_type: torch.Tensor) -> torch.Tensor:
        """the training step's loss (lightning_module.py:278-312)"""
        if isinstance(self.loss, L2Loss):
            return l2_loss(net_out, target, node_type, self.loss_masks)
        if not isinstance(self.loss, MultiLoss):
            return self.loss(graph=batch, target=target, network_output=net_out, node_type=node_type, masks=self.loss_masks,
                             gradient_method=self.gradient_method)
        u_out = u_tgt = geom = None
        if self.loss.needs_physical_fields:
            # the geometry of this batch object: pinned on it by the first step that sees it (never built inside a capture)
            geom = LossGeometry.for_graph(batch, self.gradient_method)
            # Simulator.build_outputs of the output and of the normalised target (lightning_module.py:279-280), after this step's
            # normaliser accumulation; the statistics are formed once for both
            nz = self.sim._output_normalizer
            with torch.no_grad():
                std, mean = nz._std_with_epsilon(), nz._mean()
                pre = self.sim._get_pre_target(batch)
                u_tgt = pre + (target * std + mean)
            u_out = pre + (net_out * std + mean)
        total, terms = self.loss(graph=batch, target=target, network_output=net_out, node_type=node_type, masks=self.loss_masks,
                                 network_output_physical=u_out, target_physical=u_tgt, gradient_method=self.gradient_method,
                                 return_all_losses=True, geometry=geom)
        self.last_losses = [t.detach() for t in terms]
        return total

    def train_step(self, batch: Graph, mtp_centers: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one optimiser step; ``mtp_centers`` (tests): the centre nodes of the spatial-MTP branch, in the batch's numbering, instead
        of the Engine's own draw"""
        self.sim.train()
        lr_now = self.learning_rate * lr_factor(self.step_count, self.warmup, self.num_steps)
        fused = isinstance(self.opt, FusedClipAdamW)
        if fused:
            self.opt.set_lr(lr_now)
        else:
            for g in self.opt.param_groups:
                g["lr"] = lr_now
        node_type = batch.x[:, self.sim.node_type_index]
        if self.spatial_mtp is not None:
            self._mtp_H = self._mtp_H_neigh = None
        net_out, target, _ = self.sim(batch)
        loss = self._loss(batch, net_out, target, node_type)
        if self.spatial_mtp is not None:   # lightning_module.py:321-340
            aux, stats = self._mtp_loss(batch, target, mtp_centers)
            if aux is not None:
                loss = loss + self.mtp["spatial_mtp_alpha"] * aux
                self.last_mtp_stats = {"sp_mtp/aux_loss": aux.detach(), **{k: v.detach() for k, v in stats.items()}}
            self._mtp_H = self._mtp_H_neigh = None
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync(self._train_params())
        if fused:  # clip + AdamW in one engine call
            self.opt.step()
            self.last_grad_norm = self.opt.norm_t
        else:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self._train_params(), self.grad_clip)
            self.opt.step()
        self.step_count += 1
        return loss.detach()

    # ---------------------------------------------------------------- hipGraph replay
    def capture_train_step(self, batch: Graph, warmup: int = 3):
        """Capture one whole training step (forward, loss, backward, clip, AdamW) in a hipGraph.

        A step is ~450 dependent launches; driven from Python that is ~10 ms of host time --
        launch-bound for a 2k-node mesh.  The engine's kernels are launched on torch's current
        stream, allocate nothing and never synchronise, so the step captures as is; replay costs
        ~1 us per node.  The mesh topology and tensor shapes are frozen in the graph: capture
        once per mesh/batch shape, feed new data through ``train_step_graphed`` (copied into the
        static input tensors).  The learning rate lives in a device tensor updated before replay.
        With a physics loss the mesh GEOMETRY (``losses.LossGeometry``) is frozen too: it is built by the
        eager warm-up steps and pinned on the static batch; ``last_losses`` then holds the captured step's
        per-term scalars, refreshed by every replay.
        """
        dev = self.device
        if self.is_transolver:
            raise NotImplementedError("capture_train_step with model.type 'transolver' is not verified (the token part between the slice "
                                      "launches is differentiated by torch autograd inside the backward); use train_step")
        if self.spatial_mtp is not None:
            raise NotImplementedError("capture_train_step with training.use_spatial_mtp: the centres, and with them the packed row count, "
                                      "change every step, so the step has no fixed shape to capture; use train_step")
        assert self.grad_sync is None, "graph capture of the multi-GPU step is not supported yet"
        # >= 1 eager step first: the optimiser creates its state lazily, and state created under
        # capture would be re-zeroed by every replay
        warmup = max(1, warmup)
        self.sim.train()
        from .layers import Normalizer
        for mod in self.sim.modules():  # host mirrors of the accumulation counters: no .item() under capture
            if isinstance(mod, Normalizer) and mod._host_num_acc is None:
                mod._host_num_acc = int(mod._num_accumulations.item())
        if isinstance(self.opt, FusedClipAdamW):
            self._lr_t = self.opt.lr_t  # lr and step already live on the device
        else:
            self._lr_t = torch.tensor(self.learning_rate, dtype=torch.float32, device=dev)
            self.opt = self._make_optimizer(self._lr_t, capturable=True)
        self._static = batch.clone()
        if getattr(batch, "mgn_topology", None) is not None:
            self._static.mgn_topology = batch.mgn_topology
        else:
            from . import ops
            self._static.mgn_topology = ops.Topology(self._static.edge_index, self._static.x.shape[0])

        def body():
            node_type = self._static.x[:, self.sim.node_type_index]
            net_out, target, _ = self.sim(self._static)
            loss = self._loss(self._static, net_out, target, node_type)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            if isinstance(self.opt, FusedClipAdamW):
                self.opt.step()
                gn = self.opt.norm_t
            else:
                gn = torch.nn.utils.clip_grad_norm_(self.sim.parameters(), self.grad_clip)
                self.opt.step()
            return loss.detach(), gn

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(stream_object(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._lr_t.fill_(self.learning_rate * lr_factor(self.step_count, self.warmup, self.num_steps))
                body()
                self.step_count += 1
        stream_object(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._g_loss, self._g_gn = body()
        self._graph = g
        return g

    def train_step_graphed(self, batch: Optional[Graph] = None) -> torch.Tensor:
        """Replay the captured step; ``batch`` (same shapes / topology) is copied into the static inputs."""
        if batch is not None and batch is not self._static:
            self._static.x.copy_(batch.x, non_blocking=True)
            self._static.y.copy_(batch.y, non_blocking=True)
            if self._static.edge_attr is not None:   # (a Transformer config has no edge features)
                self._static.edge_attr.copy_(batch.edge_attr, non_blocking=True)
        self._lr_t.fill_(self.learning_rate * lr_factor(self.step_count, self.warmup, self.num_steps))
        self._graph.replay()
        self.step_count += 1
        self.last_grad_norm = self._g_gn
        return self._g_loss

    @torch.no_grad()
    def predict_step(self, batch: Graph, last_prediction: Optional[torch.Tensor]) -> torch.Tensor:
        self.sim.eval()
        batch = batch.clone()
        i0, i1 = self.sim.output_index_start, self.sim.output_index_end
        if last_prediction is not None:
            batch.x[:, i0:i1] = last_prediction
        graph, _ = self.sim._build_input_graph(batch, False)
        return self.sim.predict(batch, self.sim.model(graph), mask_truth=True)

    # ---------------------------------------------------------------- hipGraph rollout
    @torch.no_grad()
    def capture_rollout_step(self, frame: Graph, warmup: int = 2):
        """Capture one autoregressive rollout step (lightning_module.py:375-409: feed the last
        prediction back, Simulator forward in eval mode, re-impose the ground truth on the non
        NORMAL/OUTFLOW nodes) in a hipGraph.  A step is ~60 launches of 5-250 us; driven from
        Python the gaps between them cost ~25 % of the step.  Topology and shapes are frozen;
        ``rollout_graphed`` copies each frame's x / y / edge_attr into the static tensors."""
        dev = self.device
        self.sim.eval()
        st = frame.clone()
        if getattr(frame, "mgn_topology", None) is not None:
            st.mgn_topology = frame.mgn_topology
        else:
            from . import ops
            st.mgn_topology = ops.Topology(st.edge_index, st.x.shape[0])
        i0, i1 = self.sim.output_index_start, self.sim.output_index_end
        last = st.x[:, i0:i1].clone()

        def body():
            b = Graph(x=st.x.clone(), y=st.y, pos=st.pos, edge_attr=st.edge_attr, edge_index=st.edge_index)
            b.mgn_topology = st.mgn_topology
            b.x[:, i0:i1] = last
            graph, _ = self.sim._build_input_graph(b, False)
            pred = self.sim.predict(b, self.sim.model(graph), mask_truth=True)
            last.copy_(pred)
            return pred

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(stream_object(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                body()
        stream_object(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._r_pred = body()
        self._r_graph, self._r_static, self._r_last = g, st, last
        self._r_seen = {}
        return g

    @staticmethod
    def _put_frame(st: Graph, fr: Graph, seen: dict):
        """copy a frame's fields into the static tensors ``st`` of a captured step; ``seen``: name -> (tensor, version) copied last"""
        def put(name, dst, src, may_skip):
            # (the skip is for the MESH's fields only -- edge features, positions: tensors nobody refills in place; x / y are copied
            # every frame: the engine's own kernels write through raw pointers without bumping _version)
            last = seen.get(name)
            if src is dst or (may_skip and last is not None and last[0] is src and last[1] == src._version):
                return
            dst.copy_(src, non_blocking=True)
            seen[name] = (src, src._version)

        if fr is not st:
            put("x", st.x, fr.x, False)
            put("y", st.y, fr.y, False)
            put("edge_attr", st.edge_attr, fr.edge_attr, True)
            # a deforming mesh: positions are per frame (relative RoPE reads them inside the captured step)
            if st.pos is not None and getattr(fr, "pos", None) is not None:
                put("pos", st.pos, fr.pos, True)

    @torch.no_grad()
    def rollout_graphed(self, frames: Sequence[Graph]) -> List[torch.Tensor]:
        """``rollout`` through the captured step (same shapes / topology for every frame)."""
        st, i0, i1 = self._r_static, self.sim.output_index_start, self.sim.output_index_end
        out = []
        # a field whose source is the very tensor OBJECT copied last, at the same version, is not copied again: the mesh's edge
        # features -- and, for a repeated frame, everything -- stay in place (3 launches of ~5 us each per step otherwise).  The
        # object is kept referenced: an address alone may be recycled by the allocator for another frame's data.
        seen = getattr(self, "_r_seen", None)
        if seen is None:
            seen = self._r_seen = {}
        for k, fr in enumerate(frames):
            self._put_frame(st, fr, seen)
            if k == 0:
                self._r_last.copy_(fr.x[:, i0:i1])
            self._r_graph.replay()
            out.append(self._r_pred.clone())
        self._r_seen = {}   # (no frame tensor stays referenced by the engine after the call)
        return out

    #: ``rollout(..., graph="auto")`` replays a captured step when the trajectory has at least this many frames on ONE mesh of at
    #: most AUTO_GRAPH_MAX_EDGES edges (small meshes are launch-bound driven from Python: the shipped cylinder.json, 5 rounds of
    #: latent 32 on a 16-mesh batch, runs 0.88 ms per step eager and 0.45 ms replayed; large meshes gain nothing and a capture holds a
    #: private copy of the step's activations)
    AUTO_GRAPH_MIN_FRAMES = 4
    AUTO_GRAPH_MAX_EDGES = 1_000_000

    def _rollout_graph_key(self, frames: Sequence[Graph]):
        f0 = frames[0]
        ei = f0.edge_index
        if not (torch.is_tensor(ei) and ei.is_cuda):
            return None
        for fr in frames:
            if fr.edge_index is not ei and (fr.edge_index.data_ptr() != ei.data_ptr() or fr.edge_index.shape != ei.shape):
                return None
            if fr.x.shape != f0.x.shape or fr.edge_attr.shape != f0.edge_attr.shape or fr.y.shape != f0.y.shape:
                return None
        from . import ops
        has_pos = getattr(f0, "pos", None) is not None
        for fr in frames:   # positions present for all frames or for none (the captured step is built for one of the two)
            if (getattr(fr, "pos", None) is not None) != has_pos:
                return None
        return (ei.data_ptr(), ei._version, tuple(ei.shape), tuple(f0.x.shape), tuple(f0.edge_attr.shape), tuple(f0.y.shape), has_pos,
                ops.get_matrix_precision())

    @torch.no_grad()
    def rollout(self, frames: Sequence[Graph], graph: str = "auto") -> List[torch.Tensor]:
        """Autoregressive rollout over ``frames`` (lightning_module.py:375-409).  ``graph``: "off" -- every step driven from Python;
        "on" -- one step captured in a hipGraph and replayed (the frames must share one mesh and one shape); "auto" (default) --
        replay when they do, the trajectory is long enough to pay for the capture and the mesh is small enough to be
        launch-bound; same results either way (tests/test_hip_parity.py: graphed == eager)."""
        key = self._replay_key(frames, graph)
        if self.use_previous_data:
            return self._rollout_previous_data(frames, key)
        if key is not None:
            # the keyed edge_index is kept REFERENCED and compared by identity: an address alone may be recycled by the allocator
            # for another trajectory's topology of the same size
            if (getattr(self, "_r_key", None) != key or getattr(self, "_r_graph", None) is None
                    or getattr(self, "_r_ei", None) is not frames[0].edge_index):
                self.capture_rollout_step(frames[0])
                self._r_key = key
                self._r_ei = frames[0].edge_index
            return self.rollout_graphed(frames)
        last, out = None, []
        for fr in frames:
            last = self.predict_step(fr, last)
            out.append(last)
        return out

    def _replay_key(self, frames: Sequence[Graph], graph: str):
        """the capture key of ``frames`` (``_rollout_graph_key``) when ``rollout`` / ``validate`` are to replay a captured step
        under the mode ``graph``, None when every step is driven from Python"""
        if graph not in ("auto", "on", "off"):
            raise ValueError("graph must be 'auto', 'on' or 'off'")
        import torch.distributed as _dist
        # (a live RCCL process group's watchdog thread polls events, which is not allowed while another thread captures)
        rccl = _dist.is_available() and _dist.is_initialized() and _dist.get_backend() == "nccl"
        if graph != "off" and len(frames) > 0 and self.grad_sync is None and not (rccl and graph == "auto"):
            key = self._rollout_graph_key(frames)
            small = key is not None and len(frames) >= self.AUTO_GRAPH_MIN_FRAMES and key[2][1] <= self.AUTO_GRAPH_MAX_EDGES
            if graph == "on" and key is None:
                raise ValueError("rollout(graph='on') needs frames of one shape on one edge_index tensor")
            if key is not None and (graph == "on" or small):
                return key
        return None

    # ------------------------------------------------- previous data and validation (lightning_module.py:375-492)
    def _check_previous_data(self):
        s, p0, p1 = self.sim, self.previous_data_start, self.previous_data_end
        if p0 is None or p1 is None:
            raise ValueError("use_previous_data needs previous_data_start and previous_data_end")
        p0, p1 = int(p0), int(p1)
        if p0 < 0 or p1 <= p0:
            raise ValueError(f"previous-data columns [{p0}, {p1}) are no column range of x")
        if p1 - p0 != s.output_size:
            raise ValueError(f"previous-data columns [{p0}, {p1}) hold {p1 - p0} columns, the simulator's output has {s.output_size}")
        if p0 < s.output_index_end and s.output_index_start < p1:
            raise ValueError(f"previous-data columns [{p0}, {p1}) overlap the output columns "
                             f"[{s.output_index_start}, {s.output_index_end})")
        if p0 <= s.node_type_index < p1:
            raise ValueError(f"previous-data columns [{p0}, {p1}) contain the node-type column {s.node_type_index}")
        self.previous_data_start, self.previous_data_end = p0, p1

    def _tail(self, b: Graph, net_out: torch.Tensor, table):
        """What follows the model in a rollout frame (lightning_module.py:387-401,439-455): ``(pred, prev)`` with ``pred`` =
        build_outputs with the ground truth re-imposed and ``prev = pred - x[:, output columns]`` (None unless
        ``use_previous_data``); with ``table = (metrics [cap, 4] fp64, slot int32 [1], cap)`` the frame's row {S_all, S_loss,
        n_loss, N} goes to ``metrics[slot]`` and ``slot`` advances, without a host synchronisation.  One engine call
        (``mgn_rollout_tail``) on the device; the same formulas as torch statements for CPU tensors and outputs wider than 32."""
        sim = self.sim
        O, i0 = sim.output_size, sim.output_index_start
        y = getattr(b, "y", None)
        if y is None:
            raise ValueError("a rollout frame needs y: the ground truth is re-imposed on the boundary nodes")
        N = int(b.x.shape[0])
        if sim._can_fuse(b) and net_out.is_cuda and (table is None or 1 <= len(self.loss_masks) <= 4):
            import ctypes as C
            from . import _capi
            dev = b.x.device
            x, y = b.x.contiguous(), y.contiguous()
            sim._check_widths(x, y, None)
            no = net_out.detach().to(torch.float32).contiguous()
            pred = torch.empty(N, O, dtype=torch.float32, device=dev)
            prev = torch.empty(N, O, dtype=torch.float32, device=dev) if self.use_previous_data else None
            if self._tail_part is None or self._tail_part.device != dev:
                self._tail_part = torch.empty(_capi.lib().mgn_rollout_tail_scratch_floats(), dtype=torch.float32, device=dev)
            types = (C.c_float * len(self.loss_masks))(*[float(int(t)) for t in self.loss_masks])
            m, slot, cap = table if table is not None else (None, None, 0)
            nz = sim._output_normalizer
            call("mgn_rollout_tail", dev, x.data_ptr(), x.shape[1], i0, sim.node_type_index, y.data_ptr(), y.shape[1], no.data_ptr(), O,
                 nz._acc_sum.data_ptr(), nz._acc_sum_squared.data_ptr(), nz._acc_count.data_ptr(), float(nz._std_epsilon_value),
                 types, len(types), N, pred.data_ptr(), (prev.data_ptr() if prev is not None else None), self._tail_part.data_ptr(),
                 (m.data_ptr() if m is not None else None), (slot.data_ptr() if slot is not None else None), cap)
            return pred, prev
        pred = sim.predict(b, net_out, mask_truth=True)
        prev = pred - b.x[:, i0:i0 + O] if self.use_previous_data else None
        if table is not None:
            m, slot, cap = table
            t = b.x[:, sim.node_type_index]
            w = torch.zeros_like(t, dtype=torch.bool)
            for code in self.loss_masks:
                w = torch.logical_or(w, t == int(code))
            d2 = (pred - y[:, :O]).double() ** 2
            row = torch.stack([d2.sum(), (d2 * w.unsqueeze(1)).sum(), w.double().sum(),
                               torch.full((), float(N), dtype=torch.float64, device=pred.device)])
            at = slot.long().clamp(max=cap - 1)   # a device index: no synchronisation; a full table keeps its last row
            m.index_copy_(0, at, torch.where(slot < cap, row, m.index_select(0, at)[0]).unsqueeze(0))
            slot += 1
        return pred, prev

    def _frame(self, batch: Graph, last_prediction, last_previous_data, table):
        self.sim.eval()
        batch = batch.clone()
        i0, i1 = self.sim.output_index_start, self.sim.output_index_end
        if self.use_previous_data and self.previous_data_end > batch.x.shape[1]:
            raise ValueError(f"previous-data columns [{self.previous_data_start}, {self.previous_data_end}) are outside x "
                             f"(width {batch.x.shape[1]})")
        if last_prediction is not None:
            batch.x[:, i0:i1] = last_prediction
            if self.use_previous_data:
                batch.x[:, self.previous_data_start:self.previous_data_end] = last_previous_data
        graph, _ = self.sim._build_input_graph(batch, False)
        pred, prev = self._tail(batch, self.sim.model(graph), table)
        return batch, pred, batch.y, pred, (prev if self.use_previous_data else last_previous_data)

    @torch.no_grad()
    def make_prediction(self, batch: Graph, last_prediction: Optional[torch.Tensor], last_previous_data: Optional[torch.Tensor]):
        """``LightningModule._make_prediction`` (lightning_module.py:375-409): the frame with the last prediction -- and, with
        ``use_previous_data``, the last ``prediction - current output`` -- fed back, one Simulator forward in eval mode, the
        ground truth re-imposed on the nodes that are not NORMAL / OUTFLOW.  Returns the reference's 5-tuple
        ``(batch, predicted_outputs, target, last_prediction, last_previous_data)``."""
        return self._frame(batch, last_prediction, last_previous_data, None)

    @torch.no_grad()
    def _frame_step(self, mode: str, key, frame: Graph, table, warmup: int = 2):
        """The captured form of ``_frame`` for trajectories of one mesh and shape (``capture_rollout_step`` with the fused
        tail): kept per ``mode`` until ``key`` or the edge_index object changes."""
        S = self._f_steps.get(mode)
        if S is not None and S["key"] == key and S["ei"] is frame.edge_index:
            return S
        dev = self.device
        self.sim.eval()
        st = frame.clone()
        if getattr(frame, "mgn_topology", None) is not None:
            st.mgn_topology = frame.mgn_topology
        else:
            st.mgn_topology = _ops.Topology(st.edge_index, st.x.shape[0])
        i0, i1 = self.sim.output_index_start, self.sim.output_index_end
        p0, p1 = self.previous_data_start, self.previous_data_end
        last = st.x[:, i0:i1].clone()
        plast = st.x[:, p0:p1].clone() if self.use_previous_data else None

        def body():
            b = Graph(x=st.x.clone(), y=st.y, pos=st.pos, edge_attr=st.edge_attr, edge_index=st.edge_index)
            b.mgn_topology = st.mgn_topology
            b.x[:, i0:i1] = last
            if plast is not None:
                b.x[:, p0:p1] = plast
            graph, _ = self.sim._build_input_graph(b, False)
            pred, prev = self._tail(b, self.sim.model(graph), table)
            last.copy_(pred)
            if plast is not None:
                plast.copy_(prev)
            return pred

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(stream_object(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):   # (these advance the metrics slot: validate() sets it after the capture)
                body()
        stream_object(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pred = body()
        S = self._f_steps[mode] = dict(key=key, ei=frame.edge_index, graph=g, st=st, last=last, plast=plast, pred=pred)
        return S

    @torch.no_grad()
    def _frames_graphed(self, S, frames: Sequence[Graph]) -> List[torch.Tensor]:
        """one trajectory through the captured step ``S``: the feedback state restarts from the first frame's own columns"""
        i0, i1 = self.sim.output_index_start, self.sim.output_index_end
        out, seen = [], {}
        for k, fr in enumerate(frames):
            self._put_frame(S["st"], fr, seen)
            if k == 0:
                S["last"].copy_(fr.x[:, i0:i1])
                if S["plast"] is not None:
                    S["plast"].copy_(fr.x[:, self.previous_data_start:self.previous_data_end])
            S["graph"].replay()
            out.append(S["pred"].clone())
        return out

    def _previous_data_key(self):
        return (self.use_previous_data, self.previous_data_start, self.previous_data_end)

    def _rollout_previous_data(self, frames: Sequence[Graph], key) -> List[torch.Tensor]:
        if key is not None:
            return self._frames_graphed(self._frame_step("rollout", key + self._previous_data_key(), frames[0], None), frames)
        last = prev = None
        out = []
        for fr in frames:
            _, pred, _, last, prev = self._frame(fr, last, prev, None)
            out.append(pred)
        return out

    def _metrics_table(self, rows: int, dev: torch.device):
        """the device table validate() fills: kept between calls (its address is part of a captured step), regrown in powers of two"""
        t = self._v_table
        if t is None or t[2] < rows or t[0].device != dev:
            cap = max(1024, 1 << (rows - 1).bit_length())
            t = self._v_table = (torch.zeros(cap, 4, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), cap)
        return t

    @torch.no_grad()
    def validate(self, trajectories: Sequence[Sequence[Graph]], graph: str = "auto") -> Dict[str, Any]:
        """The validation loop (``validation_step`` / ``on_validation_epoch_end``, lightning_module.py:411-492) over
        ``trajectories``, a sequence of frame sequences; the feedback state restarts with every trajectory
        (``_reset_validation_trajectory``).  Returns

          * ``val_loss``: the mean over all frames of the masked L2 of the frame, ``S_loss / (n_loss * O)`` over the rows whose
            type is in ``loss_masks``.  (Lightning's epoch mean weights a step by its batch size; the reference validates one
            graph per batch, so that is the plain mean over the frames.)
          * ``val_all_rollout_rmse = sqrt(sum S_all / (sum N * O))``: the reference's concatenate-then-mean;
          * ``val_1step_rmse``: the mean over the trajectories of ``sqrt(S_all / (N * O))`` of their first frame;
          * ``val_loss_per_step``: the per-frame losses, a CPU double tensor in frame order;
          * ``predictions``: per trajectory the list of predicted outputs (device tensors).

        ``S_all`` is the frame's sum of ``(prediction - y)^2``, ``S_loss`` the same over the loss rows.  On the device every frame
        is one Simulator forward plus one engine call that leaves its four numbers in a device table (``mgn_rollout_tail``): no
        host synchronisation and no device-to-host copy inside the frame loop, table and row counter are read once after the
        last frame.  ``graph`` as in :meth:`rollout`; the eager and the captured step give the same bits."""
        total = sum(len(tr) for tr in trajectories)
        if total == 0:
            raise ValueError("validate needs at least one frame")
        dev = next(tr[0].x.device for tr in trajectories if len(tr) > 0)
        table = self._metrics_table(total, dev)
        m, slot, cap = table
        slot.zero_()
        preds, first, base = [], [], 0
        for frames in trajectories:
            key = self._replay_key(frames, graph)
            if key is not None:
                S = self._frame_step("validate", key + self._previous_data_key() + (m.data_ptr(), cap, self.loss_masks), frames[0], table)
            slot.fill_(base)   # this trajectory's first row, whatever a capture's warm-up steps did
            if key is not None:
                out = self._frames_graphed(S, frames)
            else:
                last = prev = None
                out = []
                for fr in frames:
                    _, pred, _, last, prev = self._frame(fr, last, prev, table)
                    out.append(pred)
            if len(frames) > 0:
                first.append(base)
            base += len(frames)
            preds.append(out)
        host = torch.cat([m[:total].reshape(-1), slot.to(torch.float64)]).cpu()   # the one device-to-host copy
        if int(host[-1]) > cap or int(host[-1]) != total:
            raise RuntimeError(f"validate: the metrics table holds {cap} rows and its counter reads {int(host[-1])} after "
                               f"{total} frames")
        S_all, S_loss, n_loss, rows = host[:-1].reshape(total, 4).unbind(1)
        O = self.sim.output_size
        per_step = S_loss / (n_loss * O)
        return {"val_loss": float(per_step.mean()),
                "val_all_rollout_rmse": float(torch.sqrt(S_all.sum() / (rows.sum() * O))),
                "val_1step_rmse": float(torch.sqrt(S_all[first] / (rows[first] * O)).mean()),
                "val_loss_per_step": per_step, "predictions": preds}
