#!/usr/bin/env python3
"""Time of the k-hop edge construction on the device (graph_physics_amd.preprocess.khop_edges: mgn_khop_count + mgn_khop_fill,
csrc/mgn_khop.hip) against the SAME construction written with torch ops on the same device -- sparse COO product of
M = I + A with itself, coalesce (which sums), drop the diagonal: what running the reference's ``compute_k_hop_edge_index`` on
this GPU amounts to.  If torch's sparse product does not run on the device the torch side runs on the CPU, and the record
says so (``torch_device``).

Sizes a user would run: the 16-mesh cylinder batch (N = 30 160), the 150k-node tetrahedral mesh, the 1M-node mesh of BASELINE
configs[3]; k = 2 and 3.  The two results are checked equal (values and order) before anything is timed.  Times are device
events around a synchronised region after a warm-up call (the torch side on the CPU: a host clock); the engine's call includes
its workspace allocation and its own host synchronisation, as a user's call does.  Writes profiles/kbench_khop.json.

usage: python tools/kbench_khop.py [--sizes batch16,tet150k,square1m] [--hops 2,3] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import graph_physics_amd as gp
from graph_physics_amd import _capi
from graph_physics_amd import preprocess as PP

dev = torch.device("cuda:0")


def make(name):
    """(edge_index on the CPU, N)"""
    if name == "batch16":
        g = gp.cylinder_batch(16, 1885, 0)
        return g.edge_index, int(g.x.shape[0])
    if name.startswith("tet"):
        from scipy.spatial import Delaunay
        n = int(name[3:-1]) * 1000
        pts = np.random.default_rng(0).random((n, 3)).astype(np.float32)
        cells = torch.from_numpy(Delaunay(pts).simplices.T.astype(np.int64)).to(dev)
        return PP.faces_to_edges(cells, n).cpu(), n
    if name.startswith("square"):
        n = int(name[6:-1]) * 1_000_000
        g = gp.square_mesh(n, seed=0)
        return g.edge_index, n
    raise SystemExit(f"unknown size {name}")


def torch_khop(ei, N, k):
    """the same set with torch ops on ei's device: (I + A)^k by sparse products, coalesced, diagonal dropped"""
    d = ei.device
    eye = torch.arange(N, device=d)
    idx = torch.cat([ei, torch.stack([eye, eye])], dim=1)
    M = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], device=d), (N, N)).coalesce()
    M = torch.sparse_coo_tensor(M.indices(), torch.ones_like(M.values()), (N, N)).coalesce()   # entries clamped to 1
    R = M
    for _ in range(k - 1):
        R = torch.sparse.mm(R, M).coalesce()
        R = torch.sparse_coo_tensor(R.indices(), torch.ones_like(R.values()), (N, N)).coalesce()
    out = R.indices()
    return out[:, out[0] != out[1]].contiguous()


def time_device(fn, reps):
    fn()                                  # warm-up: code objects, allocator, rocPRIM configurations
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


def time_host(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="batch16,tet150k,square1m")
    ap.add_argument("--hops", default="2,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kbench_khop.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_khop needs the GPU: a CPU run measures nothing")
    cap = _capi.lib().mgn_khop_row_capacity()
    records = []
    for name in args.sizes.split(","):
        ei_cpu, N = make(name)
        ei = ei_cpu.to(dev)
        for k in (int(h) for h in args.hops.split(",")):
            got, n_ovf = PP._khop(ei, N, k)
            torch_dev, why = "device", None
            try:
                want = torch_khop(ei, N, k)
                torch.cuda.synchronize()
            except Exception as e:  # noqa: BLE001 -- whatever the sparse product raises on this device: compare on the CPU instead
                torch_dev, why = "cpu", f"{type(e).__name__}: {str(e)[:200]}"
                want = torch_khop(ei_cpu, N, k).to(dev)
            equal = bool(got.shape == want.shape and torch.equal(got, want))
            rec = {"size": name, "N": N, "E": int(ei.shape[1]), "hops": k, "E_k": int(got.shape[1]), "edges_per_node": round(got.shape[1] / N, 2),
                   "largest_row": int(torch.bincount(got[0], minlength=N).max()) if got.shape[1] else 0, "row_capacity": cap,
                   "overflow_rows": int(n_ovf), "equal_to_torch_ops": equal, "torch_device": torch_dev}
            if why:
                rec["torch_device_error"] = why
            del want
            if not equal:
                rec["error"] = "results differ: not timed"
                records.append(rec)
                print(json.dumps(rec), flush=True)
                continue
            del got
            t_eng = time_device(lambda: PP.khop_edges(ei, N, k), args.reps)
            t_ref = (time_device(lambda: torch_khop(ei, N, k), args.reps) if torch_dev == "device"
                     else time_host(lambda: torch_khop(ei_cpu, N, k), args.reps))
            rec.update({"engine_ms": [round(t, 3) for t in t_eng], "torch_ops_ms": [round(t, 3) for t in t_ref],
                        "engine_ms_median": round(float(np.median(t_eng)), 3), "torch_ops_ms_median": round(float(np.median(t_ref)), 3),
                        "torch_over_engine": round(float(np.median(t_ref) / np.median(t_eng)), 2)})
            records.append(rec)
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
    out = {"tool": "tools/kbench_khop.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "device events around a synchronised region after one warm-up call; torch side on the CPU: host clock", "records": records}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    if not all(r["equal_to_torch_ops"] for r in records):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
