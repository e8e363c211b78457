#!/usr/bin/env python3
"""Measurements of the config ``loss`` section on the device (graph_physics_amd/losses.py, csrc/mgn_loss.hip).

  1. fused loss forward + backward against the SAME formulas run as torch ops on the device (``MGN_TORCH_LOSS``: what running the
     reference's loss code on this GPU amounts to), alternating in one process, both gradient methods;
  2. the one-off geometry build;
  3. the two engine calls alone (``mgn_loss_fwd`` / ``mgn_loss_bwd``) replayed from a captured graph, and the rate of their
     algorithmic bytes (computed from shapes below) as a share of the achievable HBM rate;
  4. (``--step``) the c5-shaped training step (Transformer: 10 blocks, hidden 64, 4 heads) with the pinn-aneurysm section against
     the same step with the L2 loss only, alternating.

at the c5 mesh (3-D Delaunay of ``--c5-nodes`` random points, fields of 3 columns) and at the headline batch (16 cylinder meshes,
N = 30 160, fields of 2 columns).   usage: python tools/kbench_loss.py [--sizes c5,batch16] [--c5-nodes N] [--step]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import graph_physics_amd as gp
from graph_physics_amd import _capi, harness, losses as LS
from graph_physics_amd import preprocess as PP

HBM_ACHIEVABLE = 6.3e12   # bytes/s a streaming kernel reaches on this part
PINN = {"type": ["l2loss", "gradientl2loss", "divergencel2loss"], "weights": [0.5, 0.5, 0.5], "gradient_method": "finite_diff"}
dev = torch.device("cuda:0")


def algorithmic_bytes(method, N, F, D, O, nnz, M, K):
    """bytes each call must move: every index / coefficient entry once, every field and output once"""
    node_in = 4 * N * (2 * O + 2 * F + 2) + 8 * (N + 1)          # net, tgt, u_out, u_tgt, node type, inv, row pointers
    node_out = 4 * N * (F * D + F + O)                            # a_out, bu_out, b_out
    bwd_io = 4 * N * (F * D + F + O) + 4 * N * (O + F) + 8 * (N + 1)
    if method == "finite_diff":
        stream = nnz * (4 + 4 * D)                                # col + coef per CSR entry
        return {"fwd": stream + node_in + node_out, "bwd": stream + bwd_io, "entries": nnz}
    elem = M * K * (4 + 4 * D)                                    # corner index + cv per (element, corner)
    ge = 4 * M * F * D
    fwd = elem + 2 * ge + (4 * M * K + 2 * ge) + node_in + node_out   # element pass writes ge (x2 fields), node pass reads it back
    bwd = (4 * M * K + ge) + (4 * M * K + 4 * M * K * D + ge) + bwd_io
    return {"fwd": fwd, "bwd": bwd, "entries": M * K}


def make_c5(n):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(0)
    pts = rng.random((n, 3)).astype(np.float32)
    cells = torch.from_numpy(Delaunay(pts).simplices.T.astype(np.int64)).to(dev)
    ei = PP.faces_to_edges(cells, n)
    nt = torch.from_numpy(rng.choice([0, 0, 0, 4, 5, 6], size=n).astype(np.float32)).to(dev)
    return gp.Graph(pos=torch.from_numpy(pts).to(dev), face=cells, edge_index=ei), nt, 3


def make_batch16():
    gs = [gp.cylinder_mesh(1885, i) for i in range(16)]
    b = gp.collate(gs)
    face = torch.cat([g.face + 1885 * i for i, g in enumerate(gs)], dim=1)
    return gp.Graph(pos=b.pos.to(dev), face=face.to(dev), edge_index=b.edge_index.to(dev)), b.x[:, 2].contiguous().to(dev), 2


def alternate(fns, iters=20, rounds=7, warm=3):
    """ms per call of each fn: the fns take turns, `rounds` windows of `iters` calls each between device events"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return {k: (min(v), float(np.median(v))) for k, v in out.items()}


def bench_size(name, graph, node_type, F, rec):
    N, D = int(graph.pos.shape[0]), int(graph.pos.shape[1])
    torch.manual_seed(0)
    net = torch.randn(N, F, device=dev, requires_grad=True)
    tgt = (net.detach() + torch.randn(N, F, device=dev)).contiguous()
    pre = torch.sin(3.0 * graph.pos[:, :F]).contiguous()
    std, mean = torch.tensor([0.02, 0.03, 0.025][:F], device=dev), torch.tensor([0.01, -0.02, 0.005][:F], device=dev)
    for method in LS.GRADIENT_METHODS:
        # ---- 2. geometry build (host clock around a synchronised build: it validates indices on the host)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            geom = gp.LossGeometry(graph, method)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        graph.mgn_loss_geometry = geom
        nnz = int(geom.col.numel()) if method == "finite_diff" else 0
        M, K = (geom.M, geom.K) if method == "least_squares" else (0, 0)
        loss, _ = gp.get_loss({"loss": dict(PINN, gradient_method=method)})

        def step():
            net.grad = None
            u_out, u_tgt = pre + (net * std + mean), pre + (tgt * std + mean)
            total = loss(graph=graph, target=tgt, network_output=net, node_type=node_type, masks=[0, 5], network_output_physical=u_out,
                         target_physical=u_tgt, gradient_method=method, geometry=geom)
            total.backward()
            return total

        def torch_step():
            os.environ["MGN_TORCH_LOSS"] = "1"
            try:
                return step()
            finally:
                del os.environ["MGN_TORCH_LOSS"]

        a, b = step(), torch_step()
        agree = abs(float(a) - float(b)) / abs(float(b))
        # ---- 1. fused against torch ops, alternating
        t = alternate({"fused": step, "torch": torch_step})
        # ---- 3. the two engine calls alone, 20 per replayed graph
        f32 = net.detach()
        u_out, u_tgt = (pre + (f32 * std + mean)).contiguous(), (pre + (tgt * std + mean)).contiguous()
        kinds, weights = tuple(l.kind for l in loss.losses), tuple(loss.weights)
        args, keep, _, _ = LS._launch_fwd(f32, tgt, node_type, u_out, u_tgt, geom, kinds, weights, (0, 5))
        g1 = torch.ones(1, device=dev)
        d_net, d_u = torch.empty(N, F, device=dev), torch.empty(N, F, device=dev)
        dge = torch.empty(max(M, 1), F, D, device=dev)
        L = _capi.lib()
        side = torch.cuda.Stream(device=dev)
        graphs = {}
        for which in ("fwd", "bwd"):
            def call(s):
                if which == "fwd":
                    rc = L.mgn_loss_fwd(C.byref(args), s)
                else:
                    rc = L.mgn_loss_bwd(C.byref(args), g1.data_ptr(), d_net.data_ptr(), d_u.data_ptr(), dge.data_ptr(), s)
                _capi.check(rc, "mgn_loss_" + which, loss=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                call(side.cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(20):
                    call(torch.cuda.current_stream(dev).cuda_stream)
            graphs[which] = g
        tk = alternate({k: g.replay for k, g in graphs.items()}, iters=5)
        by = algorithmic_bytes(method, N, F, D, F, nnz, M, K)
        r = {"size": name, "N": N, "F": F, "D": D, "method": method, "entries": by["entries"],
             "geometry_build_ms": [round(x, 3) for x in ts],
             "fused_fwd_bwd_ms_min_median": [round(x, 4) for x in t["fused"]], "torch_fwd_bwd_ms_min_median": [round(x, 4) for x in t["torch"]],
             "torch_over_fused": round(t["torch"][0] / t["fused"][0], 1), "value_agreement": agree}
        for which in ("fwd", "bwd"):
            us = tk[which][0] / 20 * 1e3
            r[f"mgn_loss_{which}_us"] = round(us, 2)
            r[f"mgn_loss_{which}_algorithmic_MB"] = round(by[which] / 1e6, 2)
            r[f"mgn_loss_{which}_TBps"] = round(by[which] / (us * 1e-6) / 1e12, 3)
            r[f"mgn_loss_{which}_share_of_6.3TBps"] = round(by[which] / (us * 1e-6) / HBM_ACHIEVABLE, 3)
        r["note"] = ("the working set of one call (index + coefficients + fields) is %.1f MB: it stays in the L2 / Infinity Cache between the "
                     "back-to-back replays, so the share is of the HBM rate but is not an HBM measurement" % (by["fwd"] / 1e6))
        print(json.dumps(r), flush=True)
        rec.append(r)
        del keep


def bench_step(n, rec):
    """c5-shaped Engine step with the pinn-aneurysm section against L2 only, alternating windows"""
    graph, nt, _ = make_c5(n)
    rng = np.random.default_rng(1)
    feats = torch.from_numpy(rng.standard_normal((n, 14)).astype(np.float32)).to(dev)
    x = torch.cat([feats, nt[:, None]], dim=1).contiguous()
    y = (feats[:, :3] + 0.05 * torch.randn(n, 3, device=dev)).contiguous()
    batch = gp.Graph(x=x, y=y, pos=graph.pos, edge_index=graph.edge_index, face=graph.face)
    cfg = {"model": {"type": "transformer", "message_passing_num": 10, "hidden_size": 64, "node_input_size": 14, "output_size": 3,
                     "edge_input_size": 0, "num_heads": 4, "use_rope_embeddings": False, "use_gated_attention": False},
           "index": {"feature_index_start": 0, "feature_index_end": 14, "output_index_start": 0, "output_index_end": 3, "node_type_index": 14},
           "training": {"use_temporal_block": False}}
    engines = {}
    for k, c in (("l2", cfg), ("pinn", dict(cfg, loss=PINN))):
        torch.manual_seed(0)
        engines[k] = harness.Engine(c, dev, learning_rate=1e-4, num_steps=1000, warmup=10)
    times = {k: [] for k in engines}
    for k, e in engines.items():
        for _ in range(3):
            e.train_step(batch)
    for _ in range(5):
        for k, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(6):
                e.train_step(batch)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / 6 * 1e3)
    r = {"size": "c5 training step", "N": n, "l2_ms_per_step": [round(v, 3) for v in times["l2"]],
         "pinn_ms_per_step": [round(v, 3) for v in times["pinn"]],
         "added_ms_per_step_min_vs_min": round(min(times["pinn"]) - min(times["l2"]), 3),
         "added_ms_per_step_median": round(float(np.median(times["pinn"]) - np.median(times["l2"])), 3)}
    print(json.dumps(r), flush=True)
    rec.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="batch16,c5")
    ap.add_argument("--c5-nodes", type=int, default=150_000)
    ap.add_argument("--step", action="store_true", help="also time the c5-shaped training step with and without the loss section")
    ap.add_argument("--out", default=None, help="write the records as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_loss measures on the GPU: no device visible")
    rec = []
    for s in args.sizes.split(","):
        if s == "batch16":
            bench_size("headline batch (16 cylinder meshes)", *make_batch16(), rec)
        elif s == "c5":
            bench_size(f"c5 mesh (3-D Delaunay, {args.c5_nodes} nodes)", *make_c5(args.c5_nodes), rec)
    if args.step:
        bench_step(args.c5_nodes, rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
