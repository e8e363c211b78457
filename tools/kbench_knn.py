#!/usr/bin/env python3
"""Time of the k-nearest-neighbour search and of ``knn_interpolate`` forward + backward on the device
(graph_physics_amd.preprocess._knn_search: mgn_knn_search; hierarchical_pooling.KnnInterpolateFn: mgn_knn_interp_fwd / _bwd,
csrc/mgn_knn.hip) against the SAME construction written with torch ops on the same device: row-chunked ``cdist`` + ``topk`` per
graph, then ``index_select`` (forward) and ``index_add_`` (backward).  ``cdist`` runs with
``compute_mode="donot_use_mm_for_euclid_dist"``: its matrix-product form loses the neighbours of a fine mesh to cancellation
(|x|^2 + |y|^2 - 2 x.y at a spacing of 1e-3), so it is not the same construction.

Sizes a user would run, fine nodes against the ``ceil(0.25 n)`` coarse nodes per graph a DownSampler keeps (here: drawn by a seeded
random score), k = 6, 128 features:
  batch16    the 16-mesh cylinder batch, 16 x 1885 nodes against 16 x 472
  cube150k   150 000 uniform points in the unit cube against 37 500 of them (the node count of BASELINE configs[4]; the search
             does not look at the connectivity, so no tetrahedra are built)
  square1m   the 1M points of BASELINE configs[3] (``square_mesh(1_000_000, seed=0)`` draws exactly these) against 250 000

Method of kbench_khop.py: per size a ``check`` process compares the two sides first (sorted squared distances, and the share of
queries with identical neighbour sets -- the torch side has no rule for exact ties; interpolation forward and backward by
max-relative error), then each side is timed in a process of its own: device events around a synchronised region, median of
``--reps`` after ``--warm`` warm-up calls.  Every process runs under its own time limit; after a process that faulted, aborted
or ran out of time nothing more is started.  The engine's interpolation call includes its CSR build (one synchronisation), as a
user's backward does.  Writes profiles/kbench_knn.json.

usage: python tools/kbench_knn.py [--sizes batch16,cube150k,square1m] [--reps 20] [--warm 3] [--torch-reps N] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, FEATURES, RATIO = 6, 128, 0.25
#: sizes at which the torch search is checked and timed on the first rows only: its direct cdist kernel takes about 150 s for
#: the 2.5e11 distances of square1m.  The chunks are independent launches, so its time is linear in the rows; the record holds
#: the measured time of the subset and, named as such, the extrapolation to all rows.
TORCH_ROWS = {"square1m": 65536}


def make(name):
    """(pos [N, dim] fp32, graph sizes) on the host"""
    import numpy as np

    if name == "batch16":
        import graph_physics_amd as gp
        g = gp.cylinder_batch(16, 1885, 0)
        return g.pos.numpy().astype(np.float32), [1885] * 16
    if name.startswith("cube"):
        n = int(name[4:-1]) * 1000
        return np.random.default_rng(0).uniform(0.0, 1.0, size=(n, 3)).astype(np.float32), [n]
    if name.startswith("square"):
        n = int(name[6:-1]) * 1_000_000
        return np.random.default_rng(0).uniform(0.0, 1.0, size=(n, 2)).astype(np.float32), [n]
    raise SystemExit(f"unknown size {name}")


def case(name, dev):
    """fine / coarse positions, offsets, features and an output gradient on the device"""
    import numpy as np
    import torch
    from graph_physics_amd.hierarchical_pooling import num_selected

    pos, sizes = make(name)
    ptr_y = [0] + np.cumsum(sizes).tolist()
    rng = np.random.default_rng(1)
    keep = num_selected(RATIO, sizes)
    perm = np.concatenate([ptr_y[g] + rng.permutation(sizes[g])[:keep[g]] for g in range(len(sizes))])
    ptr_x = [0] + np.cumsum(keep).tolist()
    fine = torch.from_numpy(pos).to(dev)
    coarse = fine[torch.from_numpy(perm).to(dev)].contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    x = torch.randn(coarse.shape[0], FEATURES, device=dev, generator=gen)
    dy = torch.randn(fine.shape[0], FEATURES, device=dev, generator=gen)
    return fine, coarse, ptr_x, ptr_y, x, dy


def torch_knn(coarse, fine, k, ptr_x, ptr_y, chunk_entries=1 << 24, max_rows=None):
    """(idx, d2): row-chunked cdist + topk per graph.  A chunk holds at most 2^24 distances: torch's direct cdist kernel gives
    every distance a workgroup of 256 threads, and on this stack a launch beyond 2^32 threads computes only its first 2^24
    workgroups (measured: with 2^28-entry chunks 6.2 % of the rows came out right at both large sizes, 2^24 / chunk)."""
    import torch

    n = fine.shape[0] if max_rows is None else min(max_rows, fine.shape[0])   # (a row limit: single-graph sizes only)
    idx = torch.empty(n, k, dtype=torch.int64, device=fine.device)
    d2 = torch.empty(n, k, dtype=torch.float32, device=fine.device)
    for s in range(len(ptr_x) - 1):
        x0, x1, y0, y1 = ptr_x[s], ptr_x[s + 1], ptr_y[s], min(ptr_y[s + 1], n)
        rows = max(1, chunk_entries // max(1, x1 - x0))
        for r0 in range(y0, y1, rows):
            r1 = min(y1, r0 + rows)
            d = torch.cdist(fine[r0:r1], coarse[x0:x1], compute_mode="donot_use_mm_for_euclid_dist")
            dk, ik = torch.topk(d, k, dim=1, largest=False)
            idx[r0:r1] = ik + x0
            d2[r0:r1] = dk * dk
    return idx, d2


def torch_interp(x, idx, d2, dy):
    """(out, dx): index_select forward, index_add_ backward, the weights of PyG's knn_interpolate"""
    import torch

    ny, k = idx.shape
    w = 1.0 / d2.clamp(min=1e-16)
    a = w / w.sum(dim=1, keepdim=True)
    out = (x.index_select(0, idx.reshape(-1)).view(ny, k, -1) * a[..., None]).sum(dim=1)
    dx = torch.zeros_like(x).index_add_(0, idx.reshape(-1), (a[..., None] * dy[:, None, :]).reshape(ny * k, -1))
    return out, dx


def engine_fns(fine, coarse, ptr_x, ptr_y, x, dy):
    import torch
    from graph_physics_amd import preprocess as PP
    from graph_physics_amd.hierarchical_pooling import KnnInterpolateFn

    dev = fine.device
    px, py = (torch.tensor(p, dtype=torch.int64, device=dev) for p in (ptr_x, ptr_y))

    def search():
        return PP._knn_search(coarse, fine, K, px, py, len(ptr_x) - 1)

    def interp(idx, d2):
        xg = x.detach().requires_grad_(True)
        out = KnnInterpolateFn.apply(xg, idx, d2)
        out.backward(dy)
        return out.detach(), xg.grad

    return search, interp


def time_device(fn, reps, warm):
    import torch

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


def child(args):
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("kbench_knn needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    fine, coarse, ptr_x, ptr_y, x, dy = case(args.size, dev)
    search, interp = engine_fns(fine, coarse, ptr_x, ptr_y, x, dy)
    rec = {"size": args.size, "mode": args.child, "fine_nodes": int(fine.shape[0]), "coarse_nodes": int(coarse.shape[0]), "dim": int(fine.shape[1]),
           "graphs": len(ptr_x) - 1, "k": K, "features": FEATURES, "device": torch.cuda.get_device_name(0)}
    relmax = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    rows = TORCH_ROWS.get(args.size)
    if rows is not None:
        assert len(ptr_x) == 2
        rec["torch_search_rows"] = rows
    if args.child == "check":
        gi, gd = search()
        ti, td = torch_knn(coarse, fine, K, ptr_x, ptr_y, max_rows=rows)
        n = ti.shape[0]
        same_rows = float((torch.sort(gi[:n], dim=1)[0] == torch.sort(ti, dim=1)[0]).all(dim=1).float().mean())
        d2_close = bool(torch.allclose(gd[:n], td, rtol=1e-4, atol=1e-12))
        go, gdx = interp(gi, gd)
        to, tdx = torch_interp(x, gi, gd, dy)        # the engine's neighbours on both sides: this compares the interpolation alone
        rec.update({"rows_with_identical_neighbour_sets": round(same_rows, 6), "sorted_d2_allclose_rtol_1e-4": d2_close,
                    "interp_fwd_max_rel": relmax(go, to), "interp_bwd_max_rel": relmax(gdx, tdx),
                    "deterministic": bool(torch.equal(search()[0], gi) and torch.equal(interp(gi, gd)[1], gdx))})
        rec["equal"] = bool(d2_close and same_rows > 0.999 and rec["interp_fwd_max_rel"] < 1e-5 and rec["interp_bwd_max_rel"] < 1e-5 and rec["deterministic"])
    else:
        gi, gd = search()
        if args.child == "engine":
            fns = (search, lambda: interp(gi, gd))
        else:
            fns = (lambda: torch_knn(coarse, fine, K, ptr_x, ptr_y, max_rows=rows), lambda: torch_interp(x, gi, gd, dy))
        for what, fn in zip(("search", "interp_fwd_bwd"), fns):
            ts = time_device(fn, args.reps, args.warm)
            rec[f"{what}_ms"] = [round(t, 4) for t in ts]
            rec[f"{what}_ms_median"] = round(float(np.median(ts)), 4)
        rec["reps"], rec["warm"] = args.reps, args.warm
        if args.child == "torch":
            rec["cdist_chunk_entries"] = 1 << 24
            if rows is not None:   # measured on `rows` query rows; linear in the rows (independent chunks)
                rec["search_ms_rows_median"] = rec.pop("search_ms_median")
                rec["search_ms_rows"] = rec.pop("search_ms")
                rec["search_ms_median"] = round(rec["search_ms_rows_median"] * fine.shape[0] / rows, 1)
                rec["search_ms_median_is"] = f"extrapolated from {rows} of {fine.shape[0]} rows"
    print("KBENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="batch16,cube150k,square1m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=None, help="repetitions of the torch side where it differs from --reps (recorded)")
    ap.add_argument("--limit", type=int, default=360, help="time limit of each process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kbench_knn.json"))
    ap.add_argument("--child", choices=["check", "engine", "torch"], default=None)
    ap.add_argument("--size", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    records, stop = [], None
    for size in args.sizes.split(","):
        rec = {"size": size}
        for mode in ("check", "engine", "torch"):
            reps = args.torch_reps if (mode == "torch" and args.torch_reps) else args.reps
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--size", size, "--reps", str(reps), "--warm", str(args.warm)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                rc, out = r.returncode, r.stdout + r.stderr
            except subprocess.TimeoutExpired as e:
                rc, out = 124, (e.stdout or b"").decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            line = next((l[7:] for l in out.splitlines() if l.startswith("KBENCH ")), None)
            if rc != 0 or line is None:
                rec[mode] = {"error": f"exit status {rc}", "tail": out[-600:]}
                print(json.dumps(rec[mode]), flush=True)
                if rc < 0 or rc in (124, 134, 137, 139):
                    stop = f"{size}/{mode} ended with status {rc}: nothing more was started"
                break
            rec[mode] = json.loads(line)
            print(line, flush=True)
            if mode == "check" and not rec[mode]["equal"]:
                rec["error"] = "results differ: not timed"
                break
        if "engine" in rec and "torch" in rec and "error" not in rec["engine"] and "error" not in rec["torch"]:
            for what in ("search", "interp_fwd_bwd"):
                rec[f"{what}_torch_over_engine"] = round(rec["torch"][f"{what}_ms_median"] / rec["engine"][f"{what}_ms_median"], 2)
        records.append(rec)
        if stop:
            break
    result = {"tool": "tools/kbench_knn.py", "k": K, "features": FEATURES, "ratio": RATIO,
              "timing": "device events around a synchronised region, median of reps after warm-up calls; each side in its own process",
              "records": records}
    if stop:
        result["stopped"] = stop
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    if stop or any("error" in r or any("error" in r.get(m, {}) for m in ("check", "engine", "torch")) for r in records):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
