#!/usr/bin/env python3
"""Measurements of the Transolver processor on the device (graph_physics_amd/transolver.py, csrc/mgn_slice.inc): hidden 128, 8 heads
(C = 16), slice_num G = 32, at 150 000 rows (the size of BASELINE.json configs[4]) and on the 16-mesh cylinder batch.

  (a) one block (a 1-block model) and the whole model (5 blocks): the HIP path against the torch-ops path of the same module on the
      same device, weights and noise stream (``Model.backend``), forward and forward + backward, alternating in one process; median
      and spread (min .. max) of the timed windows.
  (b) every launch of include/mgn_hip_slice.h alone: time per call, the compulsory bytes of the launch from its shapes (every operand
      read or written once, fp32) and the TB/s that gives.

usage: python tools/kbench_transolver.py [--out profiles/kbench_transolver.json] [--windows 12]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import graph_physics_amd as gp
from graph_physics_amd import _capi, transolver as TS
from graph_physics_amd._launch import call, workspace
from graph_physics_amd.mesh import Graph

dev = torch.device("cuda:0")
HIDDEN, HEADS, G = 128, 8, 32
C = HIDDEN // HEADS


def windows(fns, n_windows, iters):
    """ms per call of each fn: the fns take turns, one window = ``iters`` calls between two synchronisations"""
    out = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def bench_model(layers, N, n_windows, what):
    torch.manual_seed(0)
    n_in = 2 + gp.NodeType.SIZE
    m = gp.TransolverProcessor(message_passing_num=layers, node_input_size=n_in, output_size=2, hidden_size=HIDDEN, num_heads=HEADS,
                               slice_num=G).to(dev).train()
    x = torch.randn(N, n_in, device=dev)
    g = Graph(x=x, pos=None, edge_index=None, edge_attr=None, y=None)
    dy = torch.randn(N, 2, device=dev)
    params = list(m.parameters())

    def fwd(backend):
        m.backend = backend
        with torch.no_grad():
            return m(g)

    def fwd_bwd(backend):
        m.backend = backend
        for p in params:
            p.grad = None
        out = m(g)
        out.backward(dy)
        return out

    m.model._noise_step.zero_()
    a = fwd("auto")
    m.model._noise_step.zero_()
    b = fwd("torch")
    agree = float((a - b).abs().max() / b.abs().max())
    fns = {"hip_fwd": lambda: fwd("auto"), "torch_fwd": lambda: fwd("torch"), "hip_fwd_bwd": lambda: fwd_bwd("auto"),
           "torch_fwd_bwd": lambda: fwd_bwd("torch")}
    for f in fns.values():
        f(), f()
    t = windows(fns, n_windows, iters=3)
    rec = {"what": what, "N": N, "blocks": layers, "hidden": HIDDEN, "heads": HEADS, "slice_num": G, "forward_agreement": agree,
           "windows": n_windows, "calls_per_window": 3}
    rec.update({k: stats(v) for k, v in t.items()})
    rec["torch_over_hip_fwd"] = round(rec["torch_fwd"]["median_ms"] / rec["hip_fwd"]["median_ms"], 2)
    rec["torch_over_hip_fwd_bwd"] = round(rec["torch_fwd_bwd"]["median_ms"] / rec["hip_fwd_bwd"]["median_ms"], 2)
    return rec


def bench_launches(N, n_windows):
    H = HEADS
    f = dict(dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, **f)   # noqa: E731
    xm, dOut = r(N, H * C), r(N, H * C)
    Ws, bs, W1, b1, w2, b2, bias = 0.5 * r(G, C), 0.1 * r(G), 0.5 * r(G, C), 0.1 * r(G), 0.5 * r(G), 0.1 * r(1), torch.full((H,), 0.5, **f)
    tok, dS, dnorm = r(H, G, C), r(H, G, C), r(H, G)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    w, rowsc, u = torch.empty(N, H, G, **f), torch.empty(N * H, 2, **f), torch.empty(N, H, G, **f)
    S, norm, out = torch.empty(H, G, C, **f), torch.empty(H, G, **f), torch.empty(N, H * C, **f)
    dx, da, dh1, dt2 = torch.empty(N, H * C, **f), torch.empty(N * H, G, **f), torch.empty(N * H, G, **f), torch.empty(N * H, **f)
    dw2, db2, dbias = torch.empty(G, **f), torch.empty(1, **f), torch.empty(H, **f)
    L = _capi.lib()
    ws_a = workspace(L.mgn_slice_aggregate_workspace_bytes(N, H, G, C), dev)
    ws_b = workspace(L.mgn_slice_rows_bwd_workspace_bytes(N, H, G), dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    NH = N * H
    fns = {
        "mgn_slice_uniforms": (lambda: call("mgn_slice_uniforms", dev, 0, p(step), 0, N, H, G, p(u)), 4 * NH * G),
        "mgn_slice_weights_fwd": (lambda: call("mgn_slice_weights_fwd", dev, p(xm), H * C, p(Ws), p(bs), p(W1), p(b1), p(w2), p(b2), p(bias), None, 0,
                                               p(step), 0, N, H, G, C, p(w), p(rowsc)), 4 * NH * (C + G + 2)),
        "mgn_slice_aggregate": (lambda: call("mgn_slice_aggregate", dev, p(w), p(xm), H * C, N, H, G, C, p(S), p(norm), p(ws_a), ws_a.numel()),
                                4 * NH * (G + C)),
        "mgn_slice_expand": (lambda: call("mgn_slice_expand", dev, p(w), p(tok), N, H, G, C, p(out), H * C), 4 * NH * (G + C)),
        "mgn_slice_rows_bwd": (lambda: call("mgn_slice_rows_bwd", dev, p(dOut), H * C, p(tok), p(dS), p(dnorm), p(xm), H * C, p(w), p(rowsc), p(Ws),
                                            p(bs), p(W1), p(b1), p(w2), None, 0, p(step), 0, N, H, G, C, p(dx), H * C, p(da), p(dh1), p(dt2),
                                            p(dw2), p(db2), p(dbias), p(ws_b), ws_b.numel()), 4 * NH * (2 * C + G + 2 + C + 2 * G + 1)),
    }
    for fn, _ in fns.values():
        fn(), fn()
    t = windows({k: v[0] for k, v in fns.items()}, n_windows, iters=10)
    rec = {"what": "(b) the launches alone", "N": N, "heads": H, "slice_num": G, "C": C, "windows": n_windows, "calls_per_window": 10, "launches": {}}
    for k, (_, nbytes) in fns.items():
        s = stats(t[k])
        s["compulsory_bytes"] = int(nbytes)
        s["TB_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e12, 3)
        rec["launches"][k] = s
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_transolver measures on the GPU only")
    n_cyl = int(gp.cylinder_batch(16).x.shape[0])
    rec = []
    for N in (150000, n_cyl):
        rec.append(bench_launches(N, a.windows))
        rec.append(bench_model(1, N, a.windows, "(a) one block (1-block model)"))
        rec.append(bench_model(5, N, a.windows, "(a) whole model, 5 blocks"))
    for r in rec:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
