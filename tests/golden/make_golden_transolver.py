#!/usr/bin/env python3
"""Mint ``transolver.npz`` from the REFERENCE implementation (build container only).

Run:  python tests/golden/make_golden_transolver.py            (needs the reference checkout)

The reference's ``graphphysics/models/processors.py::TransolverProcessor`` (and with it ``models/transolver.py``) is imported unmodified,
with the stand-ins of make_golden.py.  Only arrays and name lists leave this script.

Noise.  ``torch.rand_like`` is patched while a case runs and returns the stored uniforms of the current layer (every ``Attn.forward`` is
wrapped to note its layer; in training mode the checkpoint calls each layer twice and both calls get the same values).  The fp32 run
gets the stored fp32 ``u`` itself.  The fp64 run must see the SAME Gumbel noise: the mathematics under test forms
``g = -log(-log(u + 1e-8) + 1e-8)`` in fp32, where ``u + 1e-8`` rounds away for ``u`` next to 1, and an fp64 evaluation of that line from the
same ``u`` would differ by about 0.16 there.  So the fp64 run's ``rand_like`` returns the fp64 number ``u'`` whose own fp64 evaluation of that
line gives the fp32 ``g`` (``u' = exp(-(exp(-g) - 1e-8)) - 1e-8``): the reference's code stays as it is, and both runs add the same noise.

The models run in ``.train()`` (eval mode's in-place ``fx +=`` cannot be differentiated); ``Tensor.cuda`` is the identity while a case runs
(``get_grid`` calls it).

Cases (``<case>.<name>`` in the file; every case carries its own inputs), all with 2 blocks (``narrow``: 1), 5 input columns and 2 output columns:
  rope_gate   N = 70, hidden 32, 2 heads (C = 16), G = 8, rope on 2 axes, gated attention
  narrow      N = 65, hidden 16, 8 heads (C = 2), G = 64 (the reference's own test shape)
  temporal    N = 40, hidden 32, 4 heads, G = 8, use_temporal_block
  unified     N = 50, hidden 32, 4 heads, G = 8, unified_pos with ref = 2
  clamp       N = 70, hidden 32, 2 heads, G = 8; head 0's ``bias`` of every block lowered to the value at which half of its rows clamp
Per case: ``meta`` = [N, hidden, heads, G, blocks, inputs, outputs, rope axes (0: off), gate, temporal, unified ref (0: off)], ``x``, ``pos``
[N, 3], ``dy`` (the cotangent of the output), ``u`` [blocks, N, heads, G] (with ``u = 0`` and ``u = 1 - 2^-24`` planted in every block),
``tpre`` [blocks, N, heads] (the fp32 run's pre-clamp temperatures), ``keys`` / ``shapes`` (the sorted ``state_dict`` keys and their shapes,
padded with zeros to 4), ``w`` (every weight, ONE flat vector in the order of ``keys``: hundreds of small arrays cost more in archive
headers than in data), ``f32.out`` / ``f64.out`` and ``f32.g.x`` / ``f64.g.x`` (the fp32 run and the same module in ``.double()``), ``gkeys``
(the parameters that receive a gradient), ``f64.g.w`` (their fp64 gradients, one flat vector in the order of ``gkeys``) and, to keep the
file small, of the fp32 run's parameter gradients only their distance to the fp64 run: ``f32err.g.w`` [len(gkeys)] = max |a - b| / max |b|
per tensor (``f32err.out``, ``f32err.g.x`` likewise), which is what the tests' bounds are made of.

Condition (asserted here, and again by the tests from ``tpre``): no row's pre-clamp temperature lies within 1e-3 of the clamp point 0.01,
where the gradient has a kink; the seed of a case is advanced until this holds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

N_IN, N_OUT, BLOCKS = 5, 2, 2
CASES = {
    "rope_gate": dict(N=70, hidden=32, heads=2, G=8, rope=2, gate=True),
    "narrow": dict(N=65, hidden=16, heads=8, G=64, blocks=1),
    "temporal": dict(N=40, hidden=32, heads=4, G=8, temporal=True),
    "unified": dict(N=50, hidden=32, heads=4, G=8, ref=2),
    "clamp": dict(N=70, hidden=32, heads=2, G=8, clamp=True),
}
CLAMP, MARGIN = 0.01, 1e-3


def build(RefProc, c, seed):
    torch.manual_seed(seed)
    mod = RefProc(message_passing_num=c.get("blocks", BLOCKS), node_input_size=N_IN, output_size=N_OUT, hidden_size=c["hidden"], num_heads=c["heads"],
                  slice_num=c["G"], ref=c.get("ref", 8), unified_pos=bool(c.get("ref")), use_rope_embeddings=bool(c.get("rope")),
                  use_gated_attention=c.get("gate", False), rope_pos_dimension=c.get("rope", 3), use_temporal_block=c.get("temporal", False))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():   # off the initialisers' special values (ones, zeros, 0.5): every parameter's gradient path counts
        for p in mod.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    N, H, G = c["N"], c["heads"], c["G"]
    x = torch.randn(N, N_IN, generator=g)
    pos = torch.rand(N, 3, generator=g) * 2 - 1
    dy = torch.randn(N, N_OUT, generator=g)
    u = torch.rand(c.get("blocks", BLOCKS), N, H, G, generator=g)
    u[:, 0, 0, 0] = 0.0
    u[:, 1, 0, 1 % G] = 1.0 - 2.0 ** -24
    return mod.train(), x, pos, dy, u


class Noise:
    """the patched ``torch.rand_like`` and the per-layer wrappers of ``Attn.forward``"""

    def __init__(self, mod, u):
        self.u, self.layer, self.tpre = u, None, {}
        g32 = -torch.log(-torch.log(u + 1e-8) + 1e-8)                      # fp32, as the mathematics under test forms it
        self.u64 = torch.exp(-(torch.exp(-g32.double()) - 1e-8)) - 1e-8    # its fp64 pre-image under the same line
        for i, blk in enumerate(mod.model.blocks):
            blk.Attn.forward = self._wrap(blk.Attn, blk.Attn.forward, i)

    def _wrap(self, attn, inner, i):
        def fwd(x, pos=None):
            self.layer = i
            with torch.no_grad():   # the pre-clamp temperature of this layer (recorded, not part of the run)
                xm = attn.in_project_x(x).reshape(x.shape[0], x.shape[1], attn.heads, attn.dim_head).permute(0, 2, 1, 3)
                if attn.use_rope_embeddings and pos is not None:
                    xm = xm + attn.rope_projection(attn._rope_features(pos).to(xm.dtype)).unsqueeze(1)
                self.tpre[i] = (attn.proj_temperature(xm) + attn.bias)[0, :, :, 0].t().clone()   # [N, H]
            return inner(x, pos)
        return fwd

    def rand_like(self, logits):
        src = self.u if logits.dtype == torch.float32 else self.u64
        return src[self.layer].permute(1, 0, 2).unsqueeze(0).to(logits.dtype)   # [1, H, N, G]


def run(mod, x, pos, dy, noise, dt):
    mod = mod.to(dt)
    for p in mod.parameters():
        p.grad = None
    from torch_geometric.data import Data
    xx = x.to(dt).clone().requires_grad_(True)
    real_rand, real_cuda = torch.rand_like, torch.Tensor.cuda
    torch.rand_like, torch.Tensor.cuda = noise.rand_like, (lambda self, *a, **k: self)
    try:
        out = mod(Data(x=xx, pos=pos.to(dt)))
        out.backward(dy.to(dt))
    finally:
        torch.rand_like, torch.Tensor.cuda = real_rand, real_cuda
    res = {"out": out.detach().numpy().copy(), "g.x": xx.grad.numpy().copy()}
    for k, p in mod.named_parameters():
        if p.grad is not None:
            res["g.w." + k] = p.grad.numpy().copy()
    return res


def margin_ok(noise):
    return all(float((t - CLAMP).abs().min()) > MARGIN for t in noise.tpre.values())


def main():
    if not os.path.isdir(MG.REF):
        sys.exit("reference checkout not present: goldens can only be minted in the build container")
    MG.install_standins()
    torch.set_num_threads(4)
    from graphphysics.models.processors import TransolverProcessor as RefProc

    out = {}
    for ci, (name, c) in enumerate(CASES.items()):
        seed = 5100 + 100 * ci
        while True:
            mod, x, pos, dy, u = build(RefProc, c, seed)
            noise = Noise(mod, u)
            if c.get("clamp"):   # block by block: head 0's bias to where the median row of that head sits at the clamp point
                for i, blk in enumerate(mod.model.blocks):
                    run(mod, x, pos, dy, noise, torch.float32)
                    with torch.no_grad():
                        s = noise.tpre[i][:, 0].sort().values   # (between the two middle rows, not onto one of them)
                        blk.Attn.bias[0, 0, 0, 0] += CLAMP - 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
            f32 = run(mod, x, pos, dy, noise, torch.float32)
            tpre = torch.stack([noise.tpre[i] for i in range(c.get("blocks", BLOCKS))]).clone()
            if margin_ok(noise):
                break
            seed += 1
            assert seed < 5100 + 100 * ci + 50, f"{name}: no seed with every row off the clamp point"
        if c.get("clamp"):
            frac = [(float((tpre[i][:, 0] < CLAMP).float().mean()), float(mod.model.blocks[i].Attn.bias.detach()[0, 0, 0, 0])) for i in range(BLOCKS)]
            print("clamp: (fraction of head 0's rows clamped, its bias) per block:", frac)
            assert all(0.3 < f < 0.7 for f, _ in frac)
        pre = name + "."
        out[pre + "meta"] = np.array([c["N"], c["hidden"], c["heads"], c["G"], c.get("blocks", BLOCKS), N_IN, N_OUT, c.get("rope", 0), int(c.get("gate", False)),
                                      int(c.get("temporal", False)), c.get("ref", 0)], dtype=np.int64)
        out.update({pre + "x": x.numpy(), pre + "pos": pos.numpy(), pre + "dy": dy.numpy(), pre + "u": u.numpy(), pre + "tpre": tpre.numpy()})
        sd = mod.state_dict()
        keys = sorted(sd)
        out[pre + "keys"] = np.array(keys)
        out[pre + "shapes"] = np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys], dtype=np.int64)
        # (hundreds of small arrays cost more in archive headers than in data: per case the weights are ONE flat vector in the order
        # of `keys`, the fp64 parameter gradients one flat vector in the order of `gkeys`, a subset of `keys`)
        out[pre + "w"] = np.concatenate([sd[k].detach().float().reshape(-1).numpy() for k in keys])
        f64 = run(mod, x, pos, dy, noise, torch.float64)
        mod.to(torch.float32)
        assert set(f32) == set(f64)
        gkeys = [k for k in keys if "g.w." + k in f64]
        out[pre + "gkeys"] = np.array(gkeys)
        out[pre + "f64.g.w"] = np.concatenate([f64["g.w." + k].reshape(-1) for k in gkeys])
        err = lambda k: np.float64(np.abs(f32[k] - f64[k]).max() / max(np.abs(f64[k]).max(), 1e-30))   # noqa: E731
        out[pre + "f32err.g.w"] = np.array([err("g.w." + k) for k in gkeys])
        for k in ("out", "g.x"):
            out[pre + "f64." + k], out[pre + "f32." + k], out[pre + "f32err." + k] = f64[k], f32[k], err(k)
        worst = max(float(np.abs(f32[k] - f64[k]).max() / max(np.abs(f64[k]).max(), 1e-30)) for k in f32)
        print(f"{name}: seed {seed}, min |tpre - 0.01| = {float((tpre - CLAMP).abs().min()):.3e}, worst fp32-vs-fp64 {worst:.2e}")
    path = os.path.join(HERE, "transolver.npz")
    np.savez_compressed(path, **out)
    print(f"wrote transolver.npz  ({os.path.getsize(path) / 1024:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
