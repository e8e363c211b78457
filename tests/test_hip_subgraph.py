"""GPU: induced sub-meshes built on the device (csrc/mgn_subgraph.hip through preprocess.subgraph / apply_partition /
build_preprocessing(partitioning=...)) against the numpy restatement of PyG's ``subgraph`` in tests/subgraph_reference.py.
Integer work and row copies throughout: every comparison of indices is ``np.array_equal`` (values, order and the int64
dtype), every comparison of rows is ``torch.equal``; there is no tolerance but the one of the end-to-end training step."""
import numpy as np
import pytest
import torch

import recipe as R
import graph_physics_amd as gp
from graph_physics_amd import _capi, harness, preprocess as P
from subgraph_reference import apply_partition_reference, subgraph_reference

pytestmark = pytest.mark.gpu
LOSS_TOL = 1e-5   # the bound test_hip_khop.py takes from test_hip_parity.test_epd_shipped_json_shape


def _check(subset, ei, N, dev, attr=None):
    """the kernels against the reference: edge_index', edge_attr' and the edge mask; returns the reference edge_index'"""
    subset, ei = np.asarray(subset, dtype=np.int64), np.asarray(ei, dtype=np.int64).reshape(2, -1)
    want, want_attr, want_mask = subgraph_reference(subset, ei, attr, num_nodes=N, return_edge_mask=True)
    t_attr = None if attr is None else torch.as_tensor(attr).to(dev)
    got, got_attr, got_mask = P.subgraph(torch.as_tensor(subset).to(dev), torch.as_tensor(ei).to(dev), t_attr, num_nodes=N,
                                         return_edge_mask=True)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    g = got.cpu().numpy()
    assert g.dtype == want.dtype == np.int64 and np.array_equal(g, want)
    assert got_mask.dtype == torch.bool and np.array_equal(got_mask.cpu().numpy(), want_mask)
    if attr is None:
        assert got_attr is None
    else:
        assert got_attr.dtype == t_attr.dtype and torch.equal(got_attr.cpu(), torch.as_tensor(want_attr))
    plain = P.subgraph(torch.as_tensor(subset).to(dev), torch.as_tensor(ei).to(dev), num_nodes=N)
    assert len(plain) == 2 and plain[1] is None and np.array_equal(plain[0].cpu().numpy(), want)
    return want


def _block_sizes():
    B = _capi.lib().mgn_subgraph_block_edges()
    return B, sorted({1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17})


def test_workgroup_boundaries(dev):
    B, sizes = _block_sizes()
    N = 257
    subset = np.arange(0, N, 3)
    rng = np.random.default_rng(1)
    for E in sizes:
        ei = rng.integers(0, N, size=(2, E))
        want = _check(subset, ei, N, dev)
        if E >= 64:
            assert 0 < want.shape[1] < E
    # kept edges only in the last workgroup, and only in the first: the others run over nodes outside the subset
    E = 2 * B + 17
    out_nodes = np.setdiff1d(np.arange(N), subset)
    for first in (False, True):
        ei = out_nodes[rng.integers(0, out_nodes.size, size=(2, E))]
        where = slice(0, B) if first else slice(2 * B, E)
        ei[:, where] = subset[rng.integers(0, subset.size, size=(2, where.stop - where.start))]
        want = _check(subset, ei, N, dev)
        assert want.shape[1] == where.stop - where.start


def test_one_block_plus_one_edge_all_kept_and_none_kept(dev):
    B, N = _capi.lib().mgn_subgraph_block_edges(), 257
    ei = np.random.default_rng(4).integers(0, N, size=(2, B + 1))
    assert np.array_equal(_check(np.arange(N), ei, N, dev), ei)               # every edge kept: both workgroups full
    subset = np.arange(0, N, 3)
    out_nodes = np.setdiff1d(np.arange(N), subset)
    assert _check(subset, out_nodes[ei % out_nodes.size], N, dev).shape == (2, 0)   # no edge kept, in either workgroup


def test_degenerate_sets(dev):
    N = 300
    ei = R.random_graph(N, 900, 5).numpy()
    got = _check(np.zeros(0, dtype=np.int64), ei, N, dev)                      # S = 0
    assert got.shape == (2, 0) and got.dtype == np.int64
    assert np.array_equal(_check(np.arange(N), ei, N, dev), ei)               # S = N sorted: the input itself
    assert np.array_equal(_check(np.arange(N)[::-1].copy(), ei, N, dev), N - 1 - ei)   # reversed: the relabel is N-1-i
    got = _check(np.arange(0, N, 2), np.zeros((2, 0), dtype=np.int64), N, dev)   # E = 0
    assert got.shape == (2, 0)
    # a subset that keeps no edge: the edges join even nodes to odd ones only
    rng = np.random.default_rng(2)
    bip = np.stack([2 * rng.integers(0, N // 2, 500), 2 * rng.integers(0, N // 2, 500) + 1])
    assert _check(np.arange(0, N, 2), bip, N, dev).shape == (2, 0)
    # num_nodes defaults to the largest entry + 1, as in PyG
    a = P.subgraph(torch.arange(0, 200, device=dev), torch.as_tensor(ei).to(dev))[0].cpu().numpy()
    assert np.array_equal(a, subgraph_reference(np.arange(200), ei)[0])


def test_self_loops_and_duplicates_are_kept_in_order(dev):
    N = 300
    ei = R.random_graph(N, 900, 5).numpy()
    assert int((ei[0] == ei[1]).sum()) == 2                                    # what the recipe carries
    subset = np.random.default_rng(3).permutation(N)[:200]                     # unsorted, and it holds nodes 3 and ei[:, 2]
    subset = np.unique(np.concatenate([subset, [3], ei[:, 2]]))[::-1].copy()
    want = _check(subset, ei, N, dev)
    assert int((want[0] == want[1]).sum()) >= 1                                 # the guaranteed self loop (3, 3) survived
    assert np.array_equal(want[:, 1], want[:, 2])                               # ... and the duplicate pair, side by side


def test_error_paths_leave_the_input_alone(dev):
    N = 50
    ei = R.random_graph(N, 200, 1).to(dev)
    before = ei.clone()
    ids = torch.arange(0, 30, device=dev)
    for bad_id in (N, -1):
        bad = ids.clone()
        bad[7] = bad_id
        with pytest.raises(IndexError):
            P.subgraph(bad, ei, num_nodes=N)
        bad_ei = ei.clone()
        bad_ei[1, 17] = bad_id
        with pytest.raises(IndexError):
            P.subgraph(ids, bad_ei, num_nodes=N)
    twice = ids.clone()
    twice[11] = twice[4]
    with pytest.raises(ValueError):
        P.subgraph(twice, ei, num_nodes=N)
    assert torch.equal(ei, before)
    want = subgraph_reference(ids.cpu().numpy(), before.cpu().numpy(), num_nodes=N)[0]
    assert np.array_equal(P.subgraph(ids, ei, num_nodes=N)[0].cpu().numpy(), want)   # and works after an error


@pytest.mark.parametrize("width", [3, 4, 8])
def test_edge_attr_rows_follow(dev, width):
    N, E = 257, 3000
    ei = np.random.default_rng(4).integers(0, N, size=(2, E))
    _check(np.arange(0, N, 3), ei, N, dev, attr=R.randn((E, width), 5).numpy())


def _gather_ref(srcs, idxs):
    return [s[i] for s, i in zip(srcs, idxs)]


@pytest.mark.parametrize("rows", [0, 1, 65, 5000])
def test_gather_rows_batch_widths_and_rows(dev, rows):
    M = 777
    widths = (1, 3, 12, 128)
    srcs = [R.randn((M, w), 10 + w) for w in widths]
    idxs = [torch.from_numpy(np.random.default_rng(20 + w).integers(0, M, size=rows)) for w in widths]
    got = P.gather_rows_batch([s.to(dev) for s in srcs], [i.to(dev) for i in idxs])
    for g, want in zip(got, _gather_ref(srcs, idxs)):
        assert g.dtype == want.dtype and tuple(g.shape) == tuple(want.shape) and torch.equal(g.cpu(), want)


def test_gather_rows_batch_strided_source_and_other_dtypes(dev):
    M = 500
    wide = R.randn((M, 16), 1).to(dev)
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, M, size=333)).to(dev)
    ints = torch.arange(M * 3, dtype=torch.int64, device=dev).reshape(M, 3)
    flat = R.randn((M,), 3).to(dev)
    view = wide[:, 2:7]                                                         # ld_src = 16 > width = 5, unaligned start
    assert not view.is_contiguous()
    got = P.gather_rows_batch([view, None, ints, flat], [idx, idx, idx, idx])
    assert got[1] is None
    assert torch.equal(got[0], view[idx]) and torch.equal(got[2], ints[idx]) and torch.equal(got[3], flat[idx])
    with pytest.raises(ValueError):
        P.gather_rows_batch([torch.zeros(M, 3, dtype=torch.float16, device=dev)], [idx])


def test_gather_rows_batch_eight_jobs_and_canary(dev):
    """the C entry point itself: eight jobs of different shapes in one launch, dst wider than the copied columns"""
    M, CANARY = 400, -7.0
    rng = np.random.default_rng(6)
    shapes = [(1, 1), (65, 3), (5000, 12), (17, 128), (300, 5), (64, 4), (1000, 1), (257, 31)]   # (rows, width)
    jobs = (_capi.GatherJob * 8)()
    keep, want = [], []
    for j, (rows, w) in zip(jobs, shapes):
        src = R.randn((M, w + 3), rows + w).to(dev)                             # ld_src = w + 3
        idx = torch.from_numpy(rng.integers(0, M, size=rows)).to(dev)
        dst = torch.full((rows, w + 2), CANARY, device=dev)                     # two canary columns beyond width
        j.src, j.ld_src, j.width, j.idx, j.rows, j.dst, j.ld_dst, j.src_rows = src.data_ptr(), w + 3, w, idx.data_ptr(), rows, dst.data_ptr(), w + 2, M
        keep.append((src, idx, dst))
        want.append(src[idx][:, :w])
    rc = _capi.lib().mgn_gather_rows_batch(8, jobs, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _capi.lib().mgn_subgraph_last_error()
    torch.cuda.synchronize()
    for (src, idx, dst), (rows, w), ref in zip(keep, shapes, want):
        assert torch.equal(dst[:, :w], ref)
        assert bool((dst[:, w:] == CANARY).all())


def _mesh_graph(n, seed, dim, dev, traj=None, frame=0):
    pos, ei, ea = R.delaunay_graph(n, seed, dim)
    x, y = R.randn((n, 3), 100 + frame), R.randn((n, 2), 200 + frame)
    g = gp.Graph(x=x.to(dev), y=y.to(dev), pos=pos.to(dev), edge_index=ei.to(dev), edge_attr=ea.to(dev), traj_index=traj,
                 face=torch.zeros(3, 5, dtype=torch.int64, device=dev))
    return g, (x.numpy(), y.numpy(), pos.numpy(), ei.numpy(), ea.numpy())


def _same_graph(sub, ref):
    assert sorted(k for k in sub.__dict__) == sorted(ref)                       # these fields and nothing else: no face
    assert np.array_equal(sub.edge_index.cpu().numpy(), ref["edge_index"]) and sub.edge_index.dtype == torch.int64
    for k in ("x", "y", "pos", "edge_attr"):
        assert torch.equal(getattr(sub, k).cpu(), torch.from_numpy(ref[k])), k
    assert sub.num_nodes == ref["num_nodes"] and sub.traj_index == ref["traj_index"]


@pytest.mark.parametrize("n,seed,dim,parts", [(3000, 7, 2, 4), (2000, 9, 3, 3)])
def test_partitioned_meshes(dev, n, seed, dim, parts):
    g, (x, y, pos, ei, ea) = _mesh_graph(n, seed, dim, dev, traj=3)
    ids = P.partition_node_ids(g, parts)
    assert len(ids) == parts and all(i.dtype == torch.int64 and i.device.type == "cuda" for i in ids)
    every = torch.cat(ids).cpu().numpy()
    assert np.array_equal(np.sort(every), np.arange(n))                         # disjoint and covering
    kept = 0
    for p in range(parts):
        nodes = ids[p].cpu().numpy()
        assert np.array_equal(nodes, np.sort(nodes))
        shuffled = ids[p][torch.randperm(len(nodes), generator=torch.Generator().manual_seed(p)).to(dev)]   # apply_partition sorts
        sub = P.apply_partition(g, shuffled)
        _same_graph(sub, apply_partition_reference(x, y, pos, ei, ea, nodes, traj_index=3))
        kept += int(sub.edge_index.shape[1])
    part_of = np.empty(n, dtype=np.int64)
    for p in range(parts):
        part_of[ids[p].cpu().numpy()] = p
    cut = int((part_of[ei[0]] != part_of[ei[1]]).sum())
    assert cut > 0 and kept + cut == ei.shape[1]                                # cut edges are dropped, nothing else


def test_cached_plan_makes_no_host_synchronisation(dev, monkeypatch):
    n = 3000
    g0, (x0, y0, pos, ei, ea) = _mesh_graph(n, 7, 2, dev, traj=0, frame=0)
    g1, (x1, y1, _, _, _) = _mesh_graph(n, 7, 2, dev, traj=0, frame=1)
    calls = []
    real = P._subgraph_count
    monkeypatch.setattr(P, "_subgraph_count", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    nodes = P.partition_node_ids(g0, 4)[2]
    plan = P.partition_plan(g0, nodes)
    assert len(calls) == 1
    a = P.apply_partition(g0, nodes, plan=plan)
    b = P.apply_partition(g1, None, plan=plan)                                  # a later frame: other x and y, the same mesh
    assert len(calls) == 1                                                      # the count (the one host sync) did not run again
    _same_graph(a, apply_partition_reference(x0, y0, pos, ei, ea, nodes.cpu().numpy(), traj_index=0))
    _same_graph(b, apply_partition_reference(x1, y1, pos, ei, ea, nodes.cpu().numpy(), traj_index=0))
    assert b.edge_index.data_ptr() == a.edge_index.data_ptr() and b.x.data_ptr() != a.x.data_ptr()
    # the same through the callable: the per-trajectory cache holds the node ids and one plan per part seen
    f = P.build_preprocessing(add_edges_features=False, partitioning={"num_partitions": 4})   # edge_attr stays the recipe's
    c = f(g0, 0, part=2)
    d = f(g1, 6)                                                                # step 6 -> part 6 % 4 = 2
    assert len(calls) == 2 and list(f.partition_cache) == [0] and list(f.partition_cache[0]["plans"]) == [2]
    _same_graph(c, apply_partition_reference(x0, y0, pos, ei, ea, nodes.cpu().numpy(), traj_index=0))
    _same_graph(d, apply_partition_reference(x1, y1, pos, ei, ea, nodes.cpu().numpy(), traj_index=0))
    with pytest.raises(ValueError):
        f(g0, 0, part=4)


def test_more_edges_than_one_grid_pass(dev):
    N, E = 50_000, 1_200_000
    rng = np.random.default_rng(8)
    ei = rng.integers(0, N, size=(2, E))
    subset = rng.permutation(N)[: N // 2]
    want = _check(subset, ei, N, dev, attr=R.randn((E, 3), 9).numpy())
    assert abs(want.shape[1] - E // 4) < E // 100                                # about a quarter of the edges survive


def _frames(n, dev, frames):
    """frames of one trajectory on a 1200-node square mesh: the mesh of frame 0, x and y of their own"""
    base = gp.square_mesh(n, seed=0)
    out = []
    for t in range(frames):
        g = base.clone()
        g.x = base.x.clone()
        g.x[:, :2] = R.randn((n, 2), 40 + t)
        g.y = R.randn((n, 2), 50 + t)
        g.traj_index = 0
        out.append(g.to(dev))
    return out


def test_training_on_parts_end_to_end(dev):
    n, parts, frames = 1200, 3, 2
    param = gp.cylinder_config(2, 32)
    f = gp.get_preprocessing(param, dev, use_partitioning=True, num_partitions=parts)
    whole = gp.get_preprocessing(param, dev)                                    # the same pipeline without the cut
    torch.manual_seed(0)
    a = harness.Engine(param, dev)
    torch.manual_seed(0)
    b = harness.Engine(param, dev)
    for pa, pb in zip(a.sim.parameters(), b.sim.parameters()):
        assert torch.equal(pa, pb)
    graphs = _frames(n, dev, frames)
    ids = None
    for sample in range(frames * parts):
        frame, part = P.partition_sample(sample, parts)
        g = graphs[frame]
        sub = f(g.clone(), sample, part=part)
        if ids is None:
            ids = [i.cpu().numpy() for i in f.partition_cache[0]["node_ids"]]
        w = whole(g.clone(), sample)
        ref = apply_partition_reference(w.x.cpu().numpy(), w.y.cpu().numpy(), w.pos.cpu().numpy(), w.edge_index.cpu().numpy(),
                                        w.edge_attr.cpu().numpy(), ids[part], traj_index=0)
        _same_graph(sub, ref)
        fed = gp.Graph(**{k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in ref.items()})
        la, lb = float(a.train_step(sub)), float(b.train_step(fed))
        assert np.isfinite(la) and abs(la - lb) <= LOSS_TOL * abs(lb), (sample, la, lb)
    # one part: the callable hands back the unpartitioned graph's own tensors
    one = gp.get_preprocessing(param, dev, use_partitioning=True, num_partitions=1)
    g = graphs[0]
    ptrs = {k: getattr(g, k).data_ptr() for k in ("x", "y", "pos", "edge_index")}
    out = one(g, 0)
    assert out.num_nodes is None or out.num_nodes == n
    assert all(getattr(out, k).data_ptr() == p for k, p in ptrs.items()) and out.edge_index.shape[1] == g.edge_index.shape[1]
