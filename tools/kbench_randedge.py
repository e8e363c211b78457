#!/usr/bin/env python3
"""Time of the random extra edges of ``dataset.new_edges_ratio`` on the device (graph_physics_amd.preprocess.add_random_edges:
mgn_randedge, csrc/mgn_randedge.hip) against the SAME construction written with torch ops on the same device: ``randint``
candidates, pair codes, ``searchsorted`` against the sorted occupied codes, ``unique`` (first occurrence kept, in candidate
order), boolean select, ``cat``.  The torch side draws M candidates once and synchronises where boolean indexing does; it uses
torch's generator, so the two sides are held to the same PROPERTIES (checked before anything is timed), not to equal values.

Sizes a user would run: the 16-mesh cylinder batch (N = 30 160, E = 180 082) and the 1M-node mesh of BASELINE configs[3], at
p = 0.1 and 0.5.  Times are device events around a synchronised region after warm-up calls, median of ``--reps``; the engine's
call includes its workspace and output allocation, as a user's call does.  ``engine_ms_one_pair`` is the same call with
K = 1 on the same edge list: the table memset, the input pass (copy + insert of every input pair) and the fixed sequence of
launches -- what does not depend on K; the difference to the full call is what the candidates cost.

``--step`` adds the step-time cost at the cylinder batch: one training loop in the shape of bench.py's eager loop (Engine,
15 rounds, hidden 128, the preprocessing callable in front of every step) with ratio 0 and one with ratio 0.5.  The second
loop does MORE message-passing work (E + 2K edges instead of E), so the two are not like for like; the record states both E.

Writes profiles/kbench_randedge.json.
usage: python tools/kbench_randedge.py [--sizes batch16,square1m] [--ratios 0.1,0.5] [--reps 20] [--step] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import graph_physics_amd as gp
from graph_physics_amd import harness
from graph_physics_amd import preprocess as PP

dev = torch.device("cuda:0")


def make(name):
    """(edge_index on the CPU, N)"""
    if name == "batch16":
        g = gp.cylinder_batch(16, 1885, 0)
        return g.edge_index, int(g.x.shape[0])
    if name.startswith("square"):
        n = int(name[6:-1]) * 1_000_000
        return gp.square_mesh(n, seed=0).edge_index, n
    raise SystemExit(f"unknown size {name}")


def torch_random_edges(ei, N, K, M, gen):
    """the construction with torch ops on ei's device; K' <= K pairs (one round of M candidates)"""
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    occ = torch.sort((lo * N + hi)[lo != hi])[0]
    a = torch.randint(N, (M,), generator=gen, device=ei.device)
    b = torch.randint(N, (M,), generator=gen, device=ei.device)
    code = torch.minimum(a, b) * N + torch.maximum(a, b)
    at = torch.searchsorted(occ, code).clamp_(max=occ.numel() - 1)
    code = code[(a != b) & (occ[at] != code)]
    uniq, inv = torch.unique(code, return_inverse=True)
    first = torch.full((uniq.numel(),), code.numel(), dtype=torch.int64, device=ei.device)
    first.scatter_reduce_(0, inv, torch.arange(code.numel(), device=ei.device), reduce="amin")
    keep = torch.zeros(code.numel(), dtype=torch.bool, device=ei.device)
    keep[first] = True
    sel = code[keep][:K]                      # candidate order, never sorted-code order
    new = torch.stack([sel // N, sel % N])
    return torch.cat([ei, new, new.flip(0)], dim=1)


def properties(out, ei, N, K):
    """None if ``out`` is ``ei`` followed by K distinct new pairs lo < hi that ``ei`` holds in neither direction, and the same
    pairs reversed; otherwise what is wrong"""
    E = ei.shape[1]
    if out.dtype != torch.int64 or tuple(out.shape) != (2, E + 2 * K):
        return f"shape {tuple(out.shape)}, expected {(2, E + 2 * K)}"
    if not torch.equal(out[:, :E], ei):
        return "the input columns changed"
    lo, hi = out[0, E:E + K], out[1, E:E + K]
    if not (torch.equal(out[0, E + K:], hi) and torch.equal(out[1, E + K:], lo)):
        return "the third block is not the second reversed"
    if not bool(((lo < hi) & (lo >= 0) & (hi < N)).all()):
        return "a new pair is not lo < hi inside [0, N)"
    code = lo * N + hi
    if torch.unique(code).numel() != K:
        return "new pairs repeat"
    a, b = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    if bool(torch.isin(code, (a * N + b)[a != b]).any()):
        return "a new pair is an edge of the input"
    return None


def time_device(fn, reps, warm=3):
    for _ in range(warm):                     # code objects, allocator
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
    return ts


def step_cost(reps_warm=10, steps=50):
    """eager training loops at the cylinder batch, the preprocessing callable in front of every step"""
    out = {}
    batch = gp.cylinder_batch(16, 1885, 0).to(dev)
    for ratio in (0.0, 0.5):
        cfg = dict(gp.cylinder_config(15, 128), dataset={"new_edges_ratio": ratio})
        prep = gp.get_preprocessing(cfg, dev)
        torch.manual_seed(0)
        eng = harness.Engine(cfg, dev, learning_rate=1e-4, num_steps=10000, warmup=100)
        edges = 0

        def one(step):
            nonlocal edges
            g = prep(gp.Graph(**batch.__dict__), step)
            edges = int(g.edge_index.shape[1])
            return eng.train_step(g)

        for s in range(reps_warm):
            one(s)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s in range(reps_warm, reps_warm + steps):
            loss = one(s)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / steps
        PP.random_edges_resolve()
        out[f"ratio_{ratio}"] = {"edges_per_step": edges, "train_ms_per_step": round(1e3 * dt, 3), "steps": steps, "last_loss": float(loss)}
    a, b = out["ratio_0.0"], out["ratio_0.5"]
    out["note"] = ("eager steps (a new edge_index every step cannot replay a captured graph); ratio 0.5 runs the message passing on "
                   f"{b['edges_per_step']} edges instead of {a['edges_per_step']}: the difference is the sampler PLUS the larger graph")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="batch16,square1m")
    ap.add_argument("--ratios", default="0.1,0.5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kbench_randedge.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_randedge needs the GPU: a CPU run measures nothing")
    records = []
    for name in args.sizes.split(","):
        ei_cpu, N = make(name)
        ei = ei_cpu.to(dev).contiguous()
        E = int(ei.shape[1])
        for p in (float(r) for r in args.ratios.split(",")):
            K = PP.num_random_pairs(E, p)
            M = PP.random_edges_candidates(N, E, K)
            gen = torch.Generator(device=dev)
            gen.manual_seed(1)
            got = PP.add_random_edges(ei, N, p, seed=1, offset=0)
            PP.random_edges_resolve()
            ref = torch_random_edges(ei, N, K, M, gen)
            rec = {"size": name, "N": N, "E": E, "p": p, "K": K, "candidates_per_round": M, "sparse": PP.random_edges_sparse(N, E, K),
                   "engine_properties": properties(got, ei, N, K) or "ok", "torch_ops_properties": properties(ref, ei, N, K) or "ok",
                   "deterministic": bool(torch.equal(got, PP.add_random_edges(ei, N, p, seed=1, offset=0)))}
            del got, ref
            if rec["engine_properties"] != "ok" or rec["torch_ops_properties"] != "ok":
                rec["error"] = "a side misses the properties: not timed"
                records.append(rec)
                print(json.dumps(rec), flush=True)
                continue
            step = [0]

            def engine():
                step[0] += 1
                return PP.add_random_edges(ei, N, p, seed=1, offset=step[0])

            p_one = 2.5 / E                       # round(2.5) // 2 = 1 pair: the part of the call that does not depend on K
            assert PP.num_random_pairs(E, p_one) == 1
            t_eng = time_device(engine, args.reps)
            t_one = time_device(lambda: PP.add_random_edges(ei, N, p_one, seed=1, offset=0), args.reps)
            t_ref = time_device(lambda: torch_random_edges(ei, N, K, M, gen), args.reps)
            PP.random_edges_resolve()
            med = lambda t: round(float(np.median(t)), 4)  # noqa: E731
            rec.update({"engine_ms": [round(t, 4) for t in t_eng], "torch_ops_ms": [round(t, 4) for t in t_ref],
                        "engine_ms_median": med(t_eng), "engine_ms_one_pair_median": med(t_one), "torch_ops_ms_median": med(t_ref),
                        "input_pass_share": round(float(np.median(t_one) / np.median(t_eng)), 2),
                        "torch_over_engine": round(float(np.median(t_ref) / np.median(t_eng)), 2)})
            records.append(rec)
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
    out = {"tool": "tools/kbench_randedge.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "device events around a synchronised region after three warm-up calls, median of reps", "records": records}
    if args.step:
        out["step_cost_cylinder_batch"] = step_cost()
        print(json.dumps(out["step_cost_cylinder_batch"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    if any("error" in r for r in records):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
