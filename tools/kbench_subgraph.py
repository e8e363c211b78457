#!/usr/bin/env python3
"""Time of cutting one part out of a large mesh on the device (graph_physics_amd.preprocess.apply_partition:
mgn_subgraph_count + mgn_subgraph_fill + mgn_gather_rows_batch, csrc/mgn_subgraph.hip) against the SAME construction written
with torch ops on the same device -- node mask, edge mask, ``nonzero``, relabel through a scatter of ``arange``, row indexing:
what running the reference's ``_apply_partition`` on this GPU amounts to.

The mesh is the 1M-node / 6M-edge generator mesh of BASELINE configs[3] cut into 8 parts by ``preprocess.partition_node_ids``;
part 0 is timed.  Three figures, each the median of ``--reps`` runs after ``--warmup`` calls, device events around a
synchronised region:
  first    the first call for a part: sort the ids, count + fill (one host synchronisation), gather x / y / pos / edge_attr
  cached   every later frame of that part: one gather launch from the cached plan (node ids, edge positions)
  torch    the same two written with torch ops (the cached form keeps the node ids and ``nonzero`` of the edge mask)
The results of the two formulations are checked equal before anything is timed.  The mesh is built once on the host; each GPU
step then runs in a child process of its own under a time limit, and the first step that fails ends the run.
Writes profiles/kbench_subgraph.json.

usage: python tools/kbench_subgraph.py [--nodes 1000000] [--parts 8] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

STEP_LIMIT_S = 240


def torch_first(g, ids):
    """_apply_partition with torch ops: (x, y, pos, edge_index', edge_attr', edge positions)"""
    N = g.x.shape[0]
    ids = ids.sort()[0]
    mask = torch.zeros(N, dtype=torch.bool, device=ids.device)
    mask[ids] = True
    em = mask[g.edge_index[0]] & mask[g.edge_index[1]]
    new = torch.zeros(N, dtype=torch.int64, device=ids.device)
    new[ids] = torch.arange(ids.numel(), device=ids.device)
    edge_pos = em.nonzero().view(-1)                      # the boolean selection: synchronises with the host
    return g.x[ids], g.y[ids], g.pos[ids], new[g.edge_index[:, edge_pos]], g.edge_attr[edge_pos], edge_pos


def torch_cached(g, ids, edge_pos):
    return g.x[ids], g.y[ids], g.pos[ids], g.edge_attr[edge_pos]


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


def step(name, mesh_file, reps, warmup):
    """one GPU step in this (child) process: prints one JSON line"""
    import graph_physics_amd as gp
    from graph_physics_amd import preprocess as PP

    dev = torch.device("cuda:0")
    saved = torch.load(mesh_file)
    g = gp.Graph(**{k: v.to(dev) for k, v in saved["graph"].items()})
    ids = saved["ids"].to(dev)
    plan = PP.partition_plan(g, ids)
    rec = {"step": name}
    if name == "check":
        got = PP.apply_partition(g, ids)
        x, y, pos, ei, ea, edge_pos = torch_first(g, ids)
        again = PP.apply_partition(g, None, plan=plan)
        rec["equal_to_torch_ops"] = bool(all(torch.equal(a, b) for a, b in ((got.x, x), (got.y, y), (got.pos, pos), (got.edge_index, ei),
                                                                             (got.edge_attr, ea), (plan.edge_pos, edge_pos),
                                                                             (again.x, x), (again.edge_attr, ea))))
        rec.update({"device": torch.cuda.get_device_name(0), "part_nodes": int(ids.numel()), "part_edges": int(ei.shape[1])})
    elif name == "engine":
        rec["first_ms"], rec["first_ms_runs"] = timed(lambda: PP.apply_partition(g, ids), reps, warmup)
        rec["cached_ms"], rec["cached_ms_runs"] = timed(lambda: PP.apply_partition(g, None, plan=plan), reps, warmup)
        # by construction (csrc/mgn_subgraph.hip): 3 memsets + table set / check + flag + the scan + fill, and the gather;
        # torch.sort of the ids comes on top in the first call
        rec["first_launches"] = "torch.sort + 3 memsets + 4 kernels + rocPRIM scan + fill + 1 gather; 1 result sync + 2 header copies"
        rec["cached_launches"] = 1
    elif name == "torch":
        rec["first_ms"], rec["first_ms_runs"] = timed(lambda: torch_first(g, ids), reps, warmup)
        sorted_ids, edge_pos = plan.node_ids, plan.edge_pos
        rec["cached_ms"], rec["cached_ms_runs"] = timed(lambda: torch_cached(g, sorted_ids, edge_pos), reps, warmup)
        rec["first_launches"] = "sort, 2 fills, 2 scatters, arange, 2 mask gathers, and, nonzero (several kernels + a host sync), 6 index ops"
        rec["cached_launches"] = 4
    else:
        raise SystemExit(f"unknown step {name}")
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kbench_subgraph.json"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--mesh-file", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit("kbench_subgraph needs the GPU: a CPU run measures nothing")
        return step(args.step, args.mesh_file, args.reps, args.warmup)
    # this process only builds the mesh and starts the steps: it never opens the GPU itself

    import graph_physics_amd as gp
    from graph_physics_amd import preprocess as PP

    g = gp.square_mesh(args.nodes, seed=0)                 # host tensors: the partitioner runs on the host
    ids = PP.partition_node_ids(g, args.parts)
    out = {"tool": "tools/kbench_subgraph.py", "N": int(g.x.shape[0]), "E": int(g.edge_index.shape[1]),
           "parts": args.parts, "part_sizes": [int(i.numel()) for i in ids], "reps": args.reps, "warmup": args.warmup,
           "timing": "median of device-event times around a synchronised region; every GPU step in a process of its own", "steps": {}}
    with tempfile.TemporaryDirectory() as tmp:
        mesh_file = os.path.join(tmp, "mesh.pt")
        torch.save({"graph": {k: getattr(g, k) for k in ("x", "y", "pos", "edge_index", "edge_attr")}, "ids": ids[0]}, mesh_file)
        for name in ("check", "engine", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--mesh-file", mesh_file, "--reps", str(args.reps),
                   "--warmup", str(args.warmup)]
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
    out["torch_over_engine_first"] = round(t["first_ms"] / e["first_ms"], 2)
    out["torch_over_engine_cached"] = round(t["cached_ms"] / e["cached_ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
