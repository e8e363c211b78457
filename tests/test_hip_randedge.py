"""GPU: random extra edges drawn on the device (csrc/mgn_randedge.hip through preprocess.add_random_edges and
build_preprocessing(new_edges_ratio=...)) against the numpy restatement of the stream in tests/randedge_reference.py.  Integer
work throughout: in the sparse regime every comparison is ``torch.equal`` -- values, order and the int64 dtype; the dense
regime (toy graphs, sampled with torch ops) is held to the properties of the contract."""
import numpy as np
import pytest
import torch

import recipe as R
import graph_physics_amd as gp
from graph_physics_amd import ops, preprocess as P
import randedge_reference as RR
from randedge_reference import add_random_edges_reference, check_properties

pytestmark = pytest.mark.gpu


def ring(n, chords=()):
    i = np.arange(n)
    one_way = np.concatenate([np.stack([i, (i + d) % n]) for d in (1,) + tuple(chords)], axis=1)
    return np.concatenate([one_way, one_way[::-1]], axis=1).astype(np.int64)


def _check(ei, N, p, dev, seed=0, offset=0, M=None, as_tensor=None):
    """the kernels against the restatement, bit for bit; a result the restatement calls short must raise at resolve, any other
    must not.  Returns the restatement's result."""
    ei = np.asarray(ei, dtype=np.int64)
    want, short = add_random_edges_reference(ei, N, p, seed=seed, offset=offset, M=M)
    K = RR.num_pairs(ei.shape[1], p)
    assert RR.is_sparse(N, ei.shape[1], K) and P.random_edges_sparse(N, ei.shape[1], K)
    t = torch.from_numpy(ei).to(dev) if as_tensor is None else as_tensor
    got = P.add_random_edges(t, N, p, seed=seed, offset=offset, candidates_per_round=M)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    if short:
        with pytest.raises(RuntimeError, match="fewer than K"):
            P.random_edges_resolve()
    else:
        P.random_edges_resolve()
        check_properties(want, ei, N, K)
    return want


def test_one_wave_64_ring(dev):
    _check(ring(64), 64, 0.5, dev, seed=1)


def test_frequent_duplicates_40_ring(dev):
    N, ei = 40, ring(40)
    dups = 0
    for off in range(8):
        _check(ei, N, 0.5, dev, seed=2, offset=off)
        a, b = RR.draw(N, RR.default_candidates(N, 80, 20), 0, 2, off)
        code = (np.minimum(a, b) * N + np.maximum(a, b))[a != b]
        dups += code.size - np.unique(code).size
    assert dups > 0                                                         # the first-of-its-round rule was exercised


@pytest.mark.parametrize("M", [63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_candidate_count_boundaries(dev, M):
    """wave (64), workgroup (256) and compaction-block (2048 = 256 threads x 8 candidates) boundaries of the candidate index;
    K = 30 cuts the acceptance off inside the first wave, K = 600 lets it run through most of the candidates"""
    N, ei = 300, ring(300, chords=(7,))
    assert ei.shape[1] == 1200
    _check(ei, N, 0.05, dev, seed=3, M=M)                                   # K = 30
    if M >= 255:
        _check(ei, N, 1.0, dev, seed=3, offset=1, M=M)                      # K = 600: M = 255 .. 257 need three rounds


def test_compaction_block_plus_one_every_candidate_kept_and_an_empty_block(dev):
    """M = 2049 is one compaction block plus one candidate.  Every candidate kept: a ring of 2049 among 10^6 nodes, the draws
    distinct, loop-free and unoccupied (asserted), K = M.  No candidate kept: the sparse regime leaves three quarters of the
    pairs free, so no draw rejects all M candidates; the workgroup that keeps nothing is the second one, whose only candidate
    (index 2048) repeats an earlier one or an edge (asserted)."""
    N, ei = 1000003, ring(2049)
    a, b = RR.draw(N, 2049, 0, 11, 0)
    code = np.minimum(a, b) * N + np.maximum(a, b)
    assert (a != b).all() and np.unique(code).size == 2049 and not np.isin(code, RR.occupied_codes(ei, N)).any()
    assert RR.num_pairs(ei.shape[1], 1.0) == 2049
    want = _check(ei, N, 1.0, dev, seed=11, M=2049)
    assert np.array_equal(want[:, 4098:4098 + 2049], np.stack([np.minimum(a, b), np.maximum(a, b)]))   # all of them, in draw order

    N, ei = 300, ring(300, chords=(7,))
    a, b = RR.draw(N, 2049, 0, 26, 0)
    code = np.minimum(a, b) * N + np.maximum(a, b)
    earlier = code[:2048][a[:2048] != b[:2048]]
    assert a[2048] == b[2048] or np.isin(code[2048], RR.occupied_codes(ei, N)) or np.isin(code[2048], earlier)
    _check(ei, N, 1.0, dev, seed=26, M=2049)                                # K = 600


def test_several_compaction_blocks_all_written(dev):
    N, E = 5000, 12000
    ei = R.random_graph(N, E, 4).numpy()
    want = _check(ei, N, 1.0, dev, seed=5)                                  # K = 6000, M = 6670: four blocks of candidates
    assert RR.default_candidates(N, E, 6000) > 3 * 2048
    a = P.add_random_edges(torch.from_numpy(ei).to(dev), N, 1.0, seed=5)
    b = P.add_random_edges(torch.from_numpy(ei).to(dev), N, 1.0, seed=5)
    assert torch.equal(a, b) and torch.equal(a.cpu(), torch.from_numpy(want))   # deterministic
    c = P.add_random_edges(torch.from_numpy(ei).to(dev), N, 1.0, seed=5, offset=1)
    assert not torch.equal(a, c)
    P.random_edges_resolve()


def test_later_rounds_skip_earlier_acceptances(dev):
    N, ei = 300, ring(300)
    K = RR.num_pairs(600, 0.5)
    for off in range(6):
        _check(ei, N, 0.5, dev, seed=9, offset=off, M=K // 2)               # rounds 0, 1 and 2 run; the host test shows repeats


def test_shortfall_is_reported_and_stays_in_range(dev):
    N, ei = 300, ring(300)
    p = 1.0 / 3.0
    assert RR.num_pairs(600, p) == 100
    want = _check(ei, N, p, dev, seed=6, M=1)                               # at most 4 of the 100 pairs: resolve raises
    assert (want[:, 600 + 4:700] == 0).all()
    t = torch.from_numpy(ei).to(dev)
    got = P.add_random_edges(t, N, p, seed=6, candidates_per_round=1)
    assert int(got.min()) >= 0 and int(got.max()) < N
    with pytest.raises(RuntimeError, match="fewer than K"):
        P.random_edges_resolve()
    P.random_edges_resolve()                                                # raised once, then cleared
    # without a resolve the flag surfaces at the next call of that device once it has arrived (here: after a synchronise)
    P.add_random_edges(t, N, p, seed=6, candidates_per_round=1)
    torch.cuda.synchronize(dev)
    with pytest.raises(RuntimeError, match="fewer than K"):
        P.add_random_edges(t, N, p, seed=7)
    _check(ei, N, p, dev, seed=6)                                           # and works after an error


def test_messy_input(dev):
    N = 200
    rng = np.random.default_rng(7)
    half = rng.integers(0, N, size=(2, 300))
    ei = np.concatenate([half, half[::-1], half[:, :40], np.stack([np.arange(10), np.arange(10)])], axis=1)   # duplicates, self loops
    ei = ei[:, rng.permutation(ei.shape[1])]                                # unsorted
    one_way = np.array([[150, 199], [3, 0]])                                # present only as (j, i), j > i
    assert not ((ei[0] == 3) & (ei[1] == 150)).any() and not ((ei[0] == 150) & (ei[1] == 3)).any()
    ei = np.concatenate([ei, one_way], axis=1)
    for off in range(4):
        want = _check(ei, N, 1.0, dev, seed=8, offset=off)
        E, K = ei.shape[1], RR.num_pairs(ei.shape[1], 1.0)
        new = set(zip(want[0, E:E + K].tolist(), want[1, E:E + K].tolist()))
        assert (3, 150) not in new and (0, 199) not in new
    t32 = torch.from_numpy(ei).to(dev, torch.int32)
    _check(ei, N, 1.0, dev, seed=8, as_tensor=t32)
    wide = torch.zeros(2, 2 * ei.shape[1], dtype=torch.int64, device=dev)
    wide[:, ::2] = torch.from_numpy(ei).to(dev)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    _check(ei, N, 1.0, dev, seed=8, as_tensor=view)


def test_codes_beyond_32_bits(dev):
    N, E = 2 ** 20 + 3, 4096
    rng = np.random.default_rng(10)
    half = rng.integers(N - 5000, N, size=(2, E // 2))                      # codes lo * N + hi near 2^40
    ei = np.concatenate([half, half[::-1]], axis=1)
    want = _check(ei, N, 1.0, dev, seed=11)                                 # K = 2048
    lo, hi = want[0, E:E + 2048], want[1, E:E + 2048]
    assert ((lo * N + hi) > 2 ** 32).sum() > 2000


def test_stray_index_through_the_deferred_flag(dev):
    N, ei = 300, ring(300)
    for bad in (N, -1):
        e = ei.copy()
        e[1, 17] = bad
        want, _ = add_random_edges_reference(e, N, 0.5, seed=12)
        got = P.add_random_edges(torch.from_numpy(e).to(dev), N, 0.5, seed=12)   # no error yet: the call does not synchronise
        with pytest.raises(IndexError):
            P.random_edges_resolve()
        assert torch.equal(got.cpu(), torch.from_numpy(want))               # copied through, not followed
        P.random_edges_resolve()
    _check(ei, N, 0.5, dev, seed=12)                                        # and works after an error


def test_nothing_to_add_returns_the_input(dev):
    t = torch.from_numpy(ring(64)).to(dev)
    assert P.add_random_edges(t, 64, 0.0) is t
    assert P.add_random_edges(t, 64, 0.01) is t                             # round(1.28) // 2 = 0
    one = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    assert P.add_random_edges(one, 1, 1.0) is one                           # N < 2
    with pytest.raises(ValueError):
        P.add_random_edges(t, 64, 1.5)


def test_dense_regime_properties(dev):
    def run(ei, N, p, **kw):
        K = RR.num_pairs(ei.shape[1], p)
        assert not RR.is_sparse(N, ei.shape[1], K)
        return P.add_random_edges(torch.from_numpy(ei).to(dev), N, p, **kw).cpu().numpy(), K

    k5 = np.array([[i, j] for i in range(5) for j in range(5) if i != j]).T
    out, _ = run(k5, 5, 1.0)
    assert np.array_equal(out, k5)                                          # complete: nothing added
    k6 = np.array([[i, j] for i in range(6) for j in range(6) if i != j and {i, j} != {2, 4}]).T
    for off in range(4):
        out, _ = run(k6, 6, 1.0, offset=off)
        assert np.array_equal(out[:, :28], k6) and out[:, 28:].T.tolist() == [[2, 4], [4, 2]]   # the one free pair, once
    r8 = ring(8)
    draws = []
    for off in range(4):
        out, K = run(r8, 8, 1.0, seed=3, offset=off)
        assert K == 8
        check_properties(out, r8, 8, K)
        again, _ = run(r8, 8, 1.0, seed=3, offset=off)
        assert np.array_equal(out, again)
        draws.append(out)
    assert any(not np.array_equal(draws[0], d) for d in draws[1:])
    bad = r8.copy()
    bad[0, 3] = 8
    with pytest.raises(IndexError):
        P.add_random_edges(torch.from_numpy(bad).to(dev), 8, 1.0)


def _grid_mesh(n):
    """n x n nodes on the unit square, every cell cut into two triangles"""
    xs = np.linspace(0.0, 1.0, n, dtype=np.float32)
    pos = np.stack(np.meshgrid(xs, xs, indexing="ij"), axis=-1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    face = np.concatenate([np.stack([a, a + 1, a + n]), np.stack([a + 1, a + n + 1, a + n])], axis=1).astype(np.int64)
    return pos, face


@pytest.mark.parametrize("n,sparse", [(6, False), (20, True)])
def test_pipeline_after_khop(dev, n, sparse):
    pos, face = _grid_mesh(n)
    N = n * n

    def graph(**kw):
        return gp.Graph(x=torch.zeros(N, 3, device=dev), pos=torch.from_numpy(pos).to(dev), face=torch.from_numpy(face).to(dev), **kw)

    cache = {}
    run = P.build_preprocessing(khop=2, khop_cache=cache, new_edges_ratio=0.25, seed=5)
    a = run(graph(traj_index=0), 0)
    ek, attr_k = cache[0]
    Ek = int(ek.shape[1])
    K = RR.num_pairs(Ek, 0.25)
    assert K > 0 and RR.is_sparse(N, Ek, K) == sparse
    assert tuple(a.edge_index.shape) == (2, Ek + 2 * K)
    check_properties(a.edge_index.cpu().numpy(), ek.cpu().numpy(), N, K)
    if sparse:
        assert torch.equal(a.edge_index.cpu(), torch.from_numpy(add_random_edges_reference(ek.cpu().numpy(), N, 0.25, seed=5, offset=0)[0]))
    assert torch.equal(a.edge_attr, P.edge_features(a.pos, a.edge_index)) and tuple(a.edge_attr.shape) == (Ek + 2 * K, 3)
    assert cache[0][0] is ek and int(cache[0][0].shape[1]) == Ek and int(cache[0][1].shape[0]) == Ek   # the cache is not augmented
    b = run(graph(traj_index=0), 1)
    assert tuple(b.edge_index.shape) == (2, Ek + 2 * K) and not torch.equal(a.edge_index, b.edge_index)
    assert torch.equal(a.edge_index[:, :Ek], b.edge_index[:, :Ek])
    c = run(graph(traj_index=0), 0)
    assert torch.equal(a.edge_index, c.edge_index) and torch.equal(a.edge_attr, c.edge_attr)
    assert int(cache[0][0].shape[1]) == Ek
    bare = P.build_preprocessing(add_edges_features=False, khop=2, new_edges_ratio=0.25, seed=5)(graph(), 0)
    assert bare.edge_attr is None and torch.equal(bare.edge_index, a.edge_index)
    off = P.build_preprocessing(khop=2)(graph())
    assert int(off.edge_index.shape[1]) == Ek                               # ratio 0: the callable of today
    P.random_edges_resolve()


def test_pipeline_with_partitioning(dev):
    pos, face = _grid_mesh(20)
    N, parts = 400, 3

    def graph(**kw):
        return gp.Graph(x=R.randn((N, 3), 1).to(dev), y=R.randn((N, 2), 2).to(dev), pos=torch.from_numpy(pos).to(dev),
                        face=torch.from_numpy(face).to(dev), **kw)

    f = P.build_preprocessing(new_edges_ratio=0.25, seed=5, partitioning={"num_partitions": parts})
    whole = P.build_preprocessing(new_edges_ratio=0.25, seed=5)
    for step, part in ((2, 1), (3, 1), (4, 0)):
        sub = f(graph(traj_index=0), step, part=part)
        w = whole(graph(traj_index=0), step)
        ids = f.partition_cache[0]["node_ids"][part]
        want_ei, want_attr = P.subgraph(ids, w.edge_index, w.edge_attr, num_nodes=N)
        assert torch.equal(sub.edge_index, want_ei) and torch.equal(sub.edge_attr, want_attr)
        assert torch.equal(sub.x, w.x[ids]) and sub.num_nodes == int(ids.numel())
        assert f.partition_cache[0]["plans"] == {}                          # the edges are each sample's own: no plan is kept
    P.random_edges_resolve()


def test_training_step_on_augmented_graphs(dev):
    n = 1200
    base = gp.square_mesh(n, seed=0)
    param = dict(gp.cylinder_config(2, 32), dataset={"new_edges_ratio": 0.5})
    f = gp.get_preprocessing(param, dev)
    torch.manual_seed(0)
    net = gp.EncodeProcessDecode(2, int(base.x.shape[1]), 3, 2, hidden_size=32).to(dev)
    E = int(base.edge_index.shape[1])
    K = RR.num_pairs(E, 0.5)
    seen = []
    for step in range(2):
        g = f(base.clone().to(dev), step)
        assert tuple(g.edge_index.shape) == (2, E + 2 * K) and tuple(g.edge_attr.shape) == (E + 2 * K, 3)
        net.zero_grad()
        loss = net(gp.Graph(x=g.x, edge_attr=g.edge_attr, edge_index=g.edge_index)).square().mean()
        loss.backward()
        assert bool(torch.isfinite(loss))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        assert ops.get_topology(g.edge_index, n).resolve().E == E + 2 * K
        seen.append(g.edge_index)
    assert not torch.equal(seen[0], seen[1])
    P.random_edges_resolve()
