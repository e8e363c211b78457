#!/usr/bin/env python3
"""Per-frame time of a validation epoch on the cylinder mesh (graph_physics_amd/harness.py, csrc/mgn_rollout.inc), three ways,
alternating in one process:

  validate   ``Engine.validate(graph="on")``: the captured frame step with the fused tail (``mgn_rollout_tail``), the metrics
             read once after the last frame;
  rollout    ``Engine.rollout(graph="on")`` without previous data: the captured step as it was before ``validate`` existed,
             no metrics at all (the floor);
  torch      that rollout plus the reference's validation statements (lightning_module.py:439-455,467-489) as torch ops on its
             predictions: the node-type mask, the boolean index, the masked mean, the first step's RMSE, and one ``.cpu()`` of
             the prediction and of the target per frame; the epoch-end RMSE over the concatenation.

Each configuration is ``ROUNDSxHIDDENxMESHES`` (5x32x16 is training_config/cylinder.json as shipped on the benchmark's batch of 16
meshes, 15x128x1 the benchmark model on one mesh).  A window is one epoch of ``--frames`` frames between two host clocks that
end in a device synchronise; the windows of the three variants take turns, ``--rounds`` times; min and median are reported.

usage: python tools/kbench_validate.py [--configs 5x32x16,15x128x1] [--frames 200] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import graph_physics_amd as gp
from graph_physics_amd import harness, ops

dev = torch.device("cuda:0")


def torch_validation(eng, frames):
    """the reference's validation_step / on_validation_epoch_end statements around the captured rollout"""
    preds = eng.rollout(frames, graph="on")
    outputs, targets, losses, first = [], [], [], None
    for k, (fr, pred) in enumerate(zip(frames, preds)):
        node_type = fr.x[:, eng.sim.node_type_index]
        outputs.append(pred.cpu())
        targets.append(fr.y.cpu())
        mask = torch.zeros_like(node_type, dtype=torch.bool)
        for t in eng.loss_masks:
            mask = torch.logical_or(mask, node_type == int(t))
        losses.append(torch.mean(((pred - fr.y) ** 2)[mask]))
        if k == 0:
            first = torch.sqrt(((pred - fr.y) ** 2).mean()).detach().cpu()
    p, t = torch.cat(outputs, dim=0), torch.cat(targets, dim=0)
    return {"val_loss": float(torch.stack(losses).mean()), "val_all_rollout_rmse": torch.sqrt(((p - t) ** 2).mean()).item(),
            "val_1step_rmse": float(first)}


def alternate(fns, rounds, frames):
    out = {k: [] for k in fns}
    for fn in fns.values():   # warm-up: captures, allocator, code objects
        fn()
        fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / frames * 1e3)
    return out


def bench(rounds_mp, hidden, meshes, nframes, rounds, rec):
    torch.manual_seed(0)
    eng = harness.Engine(gp.cylinder_config(rounds_mp, hidden), dev)
    b = gp.cylinder_batch(meshes, 1885, 0).to(dev)
    n, e = int(b.x.shape[0]), int(b.edge_index.shape[1])
    b.mgn_topology = ops.Topology(b.edge_index, n)
    eng.sim.train()
    eng.sim._build_input_graph(b, True)   # normaliser statistics of the mesh (a fresh normaliser divides by 1e-8)
    eng.sim.eval()
    rng = np.random.default_rng(0)
    frames = []
    for t in range(nframes):   # one mesh, per-frame fields: x and y are copied into the captured step every frame
        f = gp.Graph(x=b.x.clone(), y=(b.y + 0.05 * torch.from_numpy(rng.standard_normal(tuple(b.y.shape)).astype(np.float32)).to(dev)),
                     pos=b.pos, edge_attr=b.edge_attr, edge_index=b.edge_index)
        f.mgn_topology = b.mgn_topology
        frames.append(f)
    a, c = eng.validate([frames], graph="on"), torch_validation(eng, frames)
    agree = {k: abs(a[k] - c[k]) / abs(c[k]) for k in c}
    t = alternate({"validate": lambda: eng.validate([frames], graph="on"), "rollout": lambda: eng.rollout(frames, graph="on"),
                   "torch": lambda: torch_validation(eng, frames)}, rounds, nframes)
    r = {"config": f"{rounds_mp} rounds, latent {hidden}, {meshes} x 1885-node meshes (N={n}, E={e})", "frames_per_epoch": nframes,
         "windows": rounds}
    for k, v in t.items():
        r[f"{k}_ms_per_frame_min_median"] = [round(min(v), 4), round(float(np.median(v)), 4)]
    r["validate_minus_rollout_us_per_frame"] = round((min(t["validate"]) - min(t["rollout"])) * 1e3, 1)
    r["torch_minus_rollout_us_per_frame"] = round((min(t["torch"]) - min(t["rollout"])) * 1e3, 1)
    r["metric_agreement_validate_vs_torch"] = agree
    print(json.dumps(r), flush=True)
    rec.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="5x32x16,15x128x1", help="ROUNDSxHIDDENxMESHES, comma separated")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the records as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kbench_validate measures on the GPU: no device visible")
    rec = []
    for c in args.configs.split(","):
        mp, hidden, meshes = (int(v) for v in c.split("x"))
        bench(mp, hidden, meshes, args.frames, args.rounds, rec)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
