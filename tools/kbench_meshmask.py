#!/usr/bin/env python3
"""Time of the masked-mesh pieces on the device (graph_physics_amd.meshmask: build_masked_graph, reconstruct_graph forward and
backward, and an L2 loss with ``selected_indexes`` on the fused loss kernels) against the SAME construction written with torch
ops on the same device -- the reference's statements of utils/meshmask.py and utils/loss.py: a scatter of ``arange``, boolean
edge selection, row indexing, ``zeros + token.expand``, indexed assignment, ``isin`` and a boolean-indexed mean.

The sample is the cylinder batch of BASELINE configs[1] (16 meshes of 1885 nodes), masking ratio 0.15, latent width 128 on
nodes and edges, a Linear(3, 128) as the edge encoder.  Two figures per side, each the median of ``--reps`` runs after
``--warmup`` calls, device events around a synchronised region:
  build   build_masked_graph of a fresh copy of the sample (one host synchronisation on both sides: the edge count / ``nonzero``)
  step    reconstruct_graph (nodes and edges) + L2 loss that leaves the visible rows out + a weighted sum of the edge rows,
          forward and backward into both tokens, both latent tensors and the encoder
The results of the two formulations are checked first: copies for equality, the loss within 1e-5 relative.  Each GPU step runs
in a child process of its own under a time limit, and the first step that fails ends the run.
Writes profiles/kbench_meshmask.json.

usage: python tools/kbench_meshmask.py [--batch 16] [--ratio 0.15] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

STEP_LIMIT_S = 240
H = 128


def torch_build(g, sel):
    """build_masked_graph with torch ops (meshmask.py:22-70); changes ``g``"""
    n = g.x.shape[0]
    table = sel.new_full((n,), -1)
    table[sel] = torch.arange(sel.numel(), device=sel.device)
    s, r = table[g.edge_index[0]], table[g.edge_index[1]]
    mask = (s >= 0) & (r >= 0)
    g.edge_index, g.edge_attr = torch.stack([s[mask], r[mask]]), g.edge_attr[mask]   # the boolean selection synchronises
    g.x, g.pos = g.x[sel], g.pos[sel]
    return g, mask


def torch_step(w, kernels):
    """reconstruct + excluded L2 + a weighted sum of the edge rows, forward and backward; ``kernels``: through the package"""
    import graph_physics_amd as gp

    for p in w["leaves"]:
        p.grad = None
    full, sel, mask = w["full"], w["sel"], w["mask"]
    n, E = full.x.shape[0], full.edge_attr.shape[0]
    if kernels:
        rec = gp.reconstruct_graph(full, gp.Graph(x=w["lat_x"], edge_attr=w["lat_e"]), sel, w["tok"], mask, edge_encoder=w["enc"],
                                   edge_mask_token=w["etok"])
        x, e = rec.x, rec.edge_attr
        loss = gp.L2Loss()(target=w["y"], network_output=x[:, :2], node_type=w["type"], masks=[0, 5], selected_indexes=sel)
    else:
        x = torch.zeros(n, H, device=sel.device) + w["tok"].expand(n, -1)
        x[sel] = w["lat_x"]
        e = w["enc"](full.edge_attr)
        e = e + w["etok"].expand(E, -1)
        e[mask] = w["lat_e"]
        keep = ((w["type"] == 0) | (w["type"] == 5)) & ~torch.isin(torch.arange(n, device=sel.device), sel)
        loss = ((x[:, :2] - w["y"]) ** 2)[keep].mean()
    total = loss + 1e-3 * (e * w["we"]).sum()
    total.backward()
    return x, e, loss


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4), [round(t, 4) for t in ts]


def step(name, batch, ratio, reps, warmup):
    """one GPU step in this (child) process: prints one JSON line"""
    import graph_physics_amd as gp

    dev = torch.device("cuda:0")
    g = gp.cylinder_batch(batch).to(dev)
    fresh = lambda: gp.Graph(x=g.x, y=g.y, pos=g.pos, edge_index=g.edge_index, edge_attr=g.edge_attr)  # noqa: E731
    sel = gp.get_masked_indexes(g, ratio, seed=0, offset=0)
    _, mask = gp.build_masked_graph(fresh(), sel)
    k, ke = int(sel.numel()), int(mask.sum())
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    torch.manual_seed(0)
    # the mesh that is reconstructed carries latent-width node rows (the reference sizes the result by graph.x)
    full = gp.Graph(x=rnd(g.x.shape[0], H), pos=g.pos, edge_index=g.edge_index, edge_attr=g.edge_attr)
    w = {"full": full, "sel": sel, "mask": mask, "y": g.y, "type": g.x[:, 2].contiguous(), "we": rnd(g.edge_attr.shape[0], H),
         "lat_x": rnd(k, H).requires_grad_(True), "lat_e": rnd(ke, H).requires_grad_(True),
         "tok": torch.nn.Parameter(rnd(H)), "etok": torch.nn.Parameter(rnd(H)), "enc": torch.nn.Linear(3, H).to(dev)}
    w["leaves"] = [w["lat_x"], w["lat_e"], w["tok"], w["etok"]] + list(w["enc"].parameters())
    rec = {"step": name}
    if name == "check":
        a, ma = gp.build_masked_graph(fresh(), sel)
        b, mb = torch_build(fresh(), sel)
        same = [torch.equal(ma, mb)] + [torch.equal(getattr(a, f), getattr(b, f)) for f in ("x", "pos", "edge_index", "edge_attr")]
        xa, ea, la = torch_step(w, True)
        ga = [p.grad.clone() for p in w["leaves"]]
        xb, eb, lb = torch_step(w, False)
        gb = [p.grad.clone() for p in w["leaves"]]
        same += [torch.equal(xa, xb), torch.equal(ea, eb)]
        rel = lambda p, q: float((p - q).abs().max() / q.abs().max().clamp_min(1e-30))  # noqa: E731
        rec["loss_rel"] = rel(la.detach(), lb.detach())
        rec["worst_grad_rel"] = max(rel(p, q) for p, q in zip(ga, gb))
        rec["equal_to_torch_ops"] = bool(all(same)) and rec["loss_rel"] < 1e-5 and rec["worst_grad_rel"] < 1e-5
        rec.update({"device": torch.cuda.get_device_name(0), "nodes": int(g.x.shape[0]), "edges": int(g.edge_attr.shape[0]),
                    "visible_nodes": k, "kept_edges": ke})
    elif name in ("engine", "torch"):
        kernels = name == "engine"
        build = (lambda: gp.build_masked_graph(fresh(), sel)) if kernels else (lambda: torch_build(fresh(), sel))
        rec["build_ms"], rec["build_ms_runs"] = timed(build, reps, warmup)
        rec["step_ms"], rec["step_ms_runs"] = timed(lambda: torch_step(w, kernels), reps, warmup)
    else:
        raise SystemExit(f"unknown step {name}")
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ratio", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kbench_meshmask.json"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit("kbench_meshmask needs the GPU: a CPU run measures nothing")
        return step(args.step, args.batch, args.ratio, args.reps, args.warmup)
    # this process only starts the steps: it never opens the GPU itself
    out = {"tool": "tools/kbench_meshmask.py", "batch": args.batch, "masking_ratio": args.ratio, "latent_width": H, "reps": args.reps,
           "warmup": args.warmup,
           "timing": "median of device-event times around a synchronised region; every GPU step in a process of its own", "steps": {}}
    for name in ("check", "engine", "torch"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(args.batch), "--ratio", str(args.ratio),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {name} ran past {STEP_LIMIT_S} s: stopping")
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"step {name} failed with status {r.returncode}: stopping")
        rec = json.loads(line[-1][len("RESULT "):])
        print(json.dumps(rec), flush=True)
        out["steps"][name] = rec
        if name == "check" and not rec["equal_to_torch_ops"]:
            raise SystemExit("results differ: not timed")
    e, t = out["steps"]["engine"], out["steps"]["torch"]
    out["torch_over_engine_build"] = round(t["build_ms"] / e["build_ms"], 2)
    out["torch_over_engine_step"] = round(t["step_ms"] / e["step_ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
