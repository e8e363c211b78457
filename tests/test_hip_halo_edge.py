"""GPU: the ReLU edge kernels of the fp32-grade default (ppr: k_edge_fwd_ppr / k_edge_bwd_ppr, csrc/mgn_ppr.inc) on a
partitioned mesh -- the product halo path (``distributed.PartitionedEPD`` -> ``ops.ProcessorFunction(halo=...)``), whose edge update
runs as TWO launches per round over row ranges of the same tensors (``ops.edge_rows``: interior rows [0, Ei) with the node CSR,
boundary rows [Ei, E) with the CSR shifted by Ei, destinations from n_interior on, ghost rows of Ps past n_own).
tests/test_partitioned_hip_multirank.py runs that path with SiLU or in the bf16 mode, which no ShEdge kernel takes.

All ranks share cuda:0 and the collectives go over gloo, as in tests/test_partitioned_hip_multirank.py.  ReLU, fp32-grade,
latent 128, 3 rounds:
  * small meshes, ppr forced (MGN_PPR=2): world 2 and 4 against the un-partitioned oracle, and against the same workers with the
    x6 kernel (MGN_PPR=0);
  * production row counts under the default environment (MGN_PPR / MGN_PP unset): world 2 on the 32-mesh cylinder batch (60 k
    nodes, 360 k edges), partitioned in coordinate stripes so that rank 0's interior AND boundary launches both pass the
    dispatcher's 65 536-row threshold; a training step and a no-grad forward.
Forward and loss within 1e-5 of the fp32 oracle; gradients by the flip-aware bar of tests/test_hip_configs.py::_check_grads
(the ReLU masks that differ from the fp32 oracle's are counted on every rank); gradients bit-identical run to run.
Which kernels ran is read off torch.profiler in each rank (engine kernels appear under their own names, k_*): k_edge_fwd_ppr
once per launch (interior + boundary, each round) and k_edge_bwd_ppr once per round -- so a change of the dispatch thresholds
cannot silently turn these into x6 tests."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import recipe as R
from conftest import assert_close3, rel_err
from oracle import mgn_oracle as O
from test_hip_configs import _check_grads
from test_partitioned_hip_multirank import _case, _collect, _free_port, _inputs

pytestmark = pytest.mark.gpu

L, H, SEED = 3, 128, 5
STRIPES = 16          # coordinate stripes of the production-size case, alternating between the two ranks
MIN_PPR_ROWS = 65536  # the dispatcher's threshold (fwd_ppr_ok / bwd_ppr_ok, csrc/mgn_kernels.hip)


def _big_case():
    """the 32-mesh cylinder batch (config C2 at batch 32) in STRIPES stripes of x, alternating ranks"""
    import graph_physics_amd as gp

    g = gp.cylinder_batch(32, 1885, 0)
    pos = g.pos.numpy()
    n = pos.shape[0]
    part = np.empty(n, dtype=np.int64)
    part[np.argsort(pos[:, 0], kind="stable")] = (np.arange(n) * STRIPES // n) % 2
    return g.pos, g.edge_index, part


def _processor_ctx(out):
    """the ProcessorFunction node of the autograd graph above ``out`` (its saved activations and local topology)"""
    seen, todo = set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == "ProcessorFunctionBackward":
            return fn
        todo += [nx for nx, _ in fn.next_functions]
    raise AssertionError("no ProcessorFunction in the autograd graph")


def _worker(rank, world, port, q, which, env):
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch.profiler import ProfilerActivity, profile

    import graph_physics_amd as gp
    from graph_physics_amd import distributed as D
    from graph_physics_amd import partition as P

    dev = torch.device("cuda:0")
    pos, ei, part = _case(world) if which == "small" else _big_case()
    N = pos.shape[0]
    params = R.make_params(R.epd_param_shapes(L, H, 11, 3, 2), SEED)
    x_in, e_in, tgt, nt = _inputs(N, ei.shape[1])
    plan = P.build_rank_plan(ei, part, rank, world, pos=pos.numpy())
    net = gp.EncodeProcessDecode(L, 11, 3, 2, hidden_size=H).to(dev)   # ReLU, fp32-grade: the defaults
    net.load_state_dict(params)
    pm = D.PartitionedEPD(net, plan)
    xo, eo, to, no = x_in[plan.owned].to(dev), e_in[plan.edge_ids].to(dev), tgt[plan.owned].to(dev), nt[plan.owned].to(dev)
    runs, signs, counts = [], None, {}
    for it in range(2):   # the second step under the profiler
        net.zero_grad(set_to_none=True)
        prof = profile(activities=[ProfilerActivity.CUDA]) if it == 1 else None
        if prof is not None:
            prof.__enter__()
        out = pm(xo, eo)
        if it == 0:   # the engine's ReLU masks (before the backward releases them): local edge order, owned nodes
            fn = _processor_ctx(out)
            inv = fn.topo.inv_perm.long()
            signs = [([np.packbits((S["He"][l] > 0)[inv].cpu().numpy(), axis=1) for l in range(3)],
                      [np.packbits((S["Hn"][l][:plan.n_own] > 0).cpu().numpy(), axis=1) for l in range(3)]) for S in fn.saved_acts]
        loss = D.partitioned_loss(out, to, no)
        loss.backward()
        if prof is not None:
            torch.cuda.synchronize()
            prof.__exit__(None, None, None)
            names = [e.name for e in prof.events()]
            counts["train"] = (sum("k_edge_fwd_ppr" in s for s in names), sum("k_edge_bwd_ppr" in s for s in names))
        runs.append({k: v.grad.clone() for k, v in net.named_parameters()})
    assert pm._halo is not None and pm._halo.active
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"rank {rank}: {k} not bit-identical run to run"
    with torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
        out_inf = pm(xo, eo)
        torch.cuda.synchronize()
    counts["infer"] = (sum("k_edge_fwd_ppr" in e.name for e in prof.events()), sum("k_edge_bwd_ppr" in e.name for e in prof.events()))
    D.GradAllReduce(average=False)(net.parameters())
    grads = {k: v.grad.cpu().numpy().copy() for k, v in net.named_parameters()}
    E = int(plan.edge_ids.numel())
    q.put(dict(rank=rank, owned=plan.owned.numpy().copy(), edge_ids=plan.edge_ids.numpy().copy(), out=out.detach().cpu().numpy().copy(),
               out_inf=out_inf.cpu().numpy().copy(), loss=float(loss.detach()), grads=grads, signs=signs, counts=counts,
               E=E, Ei=int(plan.n_interior_edges)))
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, which, env, timeout=900):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, which, env)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(q, procs, world, timeout)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def _oracle(world, which):
    """fp32 oracle (with its pre-activations) and fp64 oracle of the un-partitioned mesh: output, loss, gradients"""
    pos, ei, _ = _case(world) if which == "small" else _big_case()
    N = pos.shape[0]
    x_in, e_in, tgt, nt = _inputs(N, ei.shape[1])
    res = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.clone().to(dt).requires_grad_(True) for k, v in R.make_params(R.epd_param_shapes(L, H, 11, 3, 2), SEED).items()}
        inter = [] if dt == torch.float32 else None
        out = O.epd_forward(x_in.to(dt), e_in.to(dt), ei, p, L, intermediates=inter)
        loss = O.l2_loss(out, tgt.to(dt), nt.to(dt))
        loss.backward()
        res[dt] = (out.detach(), float(loss.detach()), {k: v.grad for k, v in p.items()}, inter)
    return N, res


def _check(res, world, which):
    """forward / loss against the fp32 oracle, gradients by the flip-aware bar; returns the assembled forward outputs"""
    N, orc = _oracle(world, which)
    o32, l32, g32, inter = orc[torch.float32]
    _, _, g64, _ = orc[torch.float64]
    full, full_inf = torch.zeros_like(o32), torch.zeros_like(o32)
    total, flips, n_act, worst = 0.0, 0, 0, 0.0
    for r in res:
        own, eids = torch.from_numpy(r["owned"]), torch.from_numpy(r["edge_ids"])
        full[own], full_inf[own] = torch.from_numpy(r["out"]), torch.from_numpy(r["out_inf"])
        total += r["loss"]
        for i, (se, sn) in enumerate(r["signs"]):
            for l in range(3):
                for packed, z in ((se[l], inter[i]["edge_pre"][l][eids]), (sn[l], inter[i]["node_pre"][l][own])):
                    hip = torch.from_numpy(np.unpackbits(packed, axis=1, count=H).astype(bool))
                    diff = hip != (z > 0)
                    flips += int(diff.sum())
                    n_act += z.numel()
                    if bool(diff.any()):
                        worst = max(worst, float(z[diff].abs().max() / z.abs().max()))
    assert n_act == 3 * L * (sum(r["E"] for r in res) + N) * H
    assert_close3(full, o32, 1e-5, "forward")
    assert_close3(full_inf, o32, 1e-5, "no-grad forward")
    assert abs(total - l32) < 1e-5 * abs(l32), (total, l32)
    grads = [{k: torch.from_numpy(g) for k, g in r["grads"].items()} for r in res]
    for g in grads:
        _check_grads(g, g32, g64, flips, worst)
    return full, (flips, n_act, worst)


def _assert_ppr_ran(res):
    """k_edge_fwd_ppr once per edge launch (interior and boundary: two per round where both have rows), k_edge_bwd_ppr once per
    round, in the training step; the no-grad forward likewise, without a backward"""
    for r in res:
        launches = L * (int(r["Ei"] > 0) + int(r["E"] > r["Ei"]))
        assert r["counts"]["train"] == (launches, L), (r["rank"], r["counts"], r["E"], r["Ei"])
        assert r["counts"]["infer"] == (launches, 0), (r["rank"], r["counts"], r["E"], r["Ei"])


@pytest.mark.parametrize("world", [2, 4])
def test_halo_edge_ppr_forced_small(world):
    res = _run_ranks(world, "small", {"MGN_PPR": "2", "MGN_PP": "0"})
    full, _ = _check(res, world, "small")
    _assert_ppr_ran(res)
    assert any(0 < r["Ei"] < r["E"] for r in res)          # a rank with both launches
    base = _run_ranks(world, "small", {"MGN_PPR": "0", "MGN_PP": "0"})  # the x6 kernel on the same split
    full_x6 = torch.zeros_like(full)
    for r in base:
        assert r["counts"]["train"][0] == 0 and r["counts"]["train"][1] == 0
        full_x6[torch.from_numpy(r["owned"])] = torch.from_numpy(r["out"])
    assert rel_err(full, full_x6) < 2e-6


def test_halo_edge_ppr_default_env_production_rows():
    res = _run_ranks(2, "big", {"MGN_PPR": None, "MGN_PP": None, "MGN_PPR_BWD": None})
    r0 = res[0]
    assert r0["Ei"] >= MIN_PPR_ROWS and r0["E"] - r0["Ei"] >= MIN_PPR_ROWS, (r0["Ei"], r0["E"])
    _assert_ppr_ran(res)
    _check(res, 2, "big")
