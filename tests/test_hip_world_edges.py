"""GPU: ``mgn_add_world_edges`` and ``mgn_edge_features`` (csrc/mgn_prep.hip) at their edges.

World edges.  The reference here is what the reference program itself calls: ``scipy.spatial.cKDTree.query_pairs`` on
the float32 world positions, then a FLOAT compare of the type column with OBSTACLE / NORMAL, both directions, the mesh
edges symmetrised, ``np.unique`` (graphphysics/dataset/preprocessing.py:92-140 with to_undirected of torch-geometric
2.6.1).  Integer work: results must be equal.  ``query_pairs`` agrees with a double ``s <= r * r`` on float32
coordinates also where pairs lie exactly at the radius (a lattice whose spacing is the radius), on coincident points and
at radius 0; ``test_query_pairs_is_the_double_compare`` (test_sim_reference_host.py, no GPU) keeps that checked.
Cases: both template instances (D = 2, 3), a position window that starts at column 2 behind the type column, N around the 256-node tile (1, 255, 256, 257, 513),
obstacles only in the last partial tile with their partners only in the first (and the reverse), no obstacle at all,
E = 0, ``max_world_pairs`` equal to the pair count and one less, and types 1.5 and 0.5.

Before ``k_world_pairs`` classified from the float (it truncated with ``(int)(long)t``),
``test_non_integral_types_link_to_nothing`` failed for D = 2 and D = 3 (the other 35 tests here passed): nodes of type 1.5 and
1.25 were linked as OBSTACLE, nodes of type 0.5 and -0.5 as NORMAL.

Edge features.  Cartesian columns: the fp32 rounding of the fp64 difference, bit for bit (fp32 subtraction is correctly
rounded).  Distance: within 2 ulp of the fp64 value: with exact differences (coordinates on a 2^-16 grid, or near 1e4
with differences of multiples of 2^-10) the squares and the adds round by half an ulp each, three squares and two adds
are at most 2.5 ulp on the sum, the square root halves that and adds half an ulp of its own: under 2.
"""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from graph_physics_amd import preprocess as P

pytestmark = pytest.mark.gpu
TYPE_COL, POS0 = 1, 2


# ------------------------------------------------------------------------------------------------ world edges
def world_edges_reference(x, edge_index, D, radius):
    N = x.shape[0]
    pairs = cKDTree(x[:, POS0:POS0 + D]).query_pairs(radius, output_type="ndarray").reshape(-1, 2)
    t = x[:, TYPE_COL]
    a, b = pairs[:, 0], pairs[:, 1]
    keep = ((t[a] == 1.0) & (t[b] == 0.0)) | ((t[a] == 0.0) & (t[b] == 1.0))
    a, b = a[keep].astype(np.int64), b[keep].astype(np.int64)
    ei = np.asarray(edge_index, dtype=np.int64)
    src, dst = np.concatenate([a, b, ei[0], ei[1]]), np.concatenate([b, a, ei[1], ei[0]])
    key = np.unique(src * np.int64(N) + dst)
    return np.stack([key // N, key % N], axis=0), int(keep.sum())


def make_x(pos, types):
    """[other | type | world position (D) | other]: the window starts at column 2, the type column before it"""
    N = pos.shape[0]
    filler = (np.arange(N, dtype=np.float32) % 5) + 7.0   # values that would classify wrongly if a kernel read them as the type
    return np.ascontiguousarray(np.concatenate([filler[:, None], types.astype(np.float32)[:, None], pos.astype(np.float32), filler[:, None]], axis=1))


def mesh_edges(N, E, seed):
    """random directed edges with duplicates, one-directional edges and self loops"""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    if E >= 4:
        ei[:, 1] = ei[:, 0]          # a duplicate
        ei[1, 2] = ei[0, 2]          # a self loop
    return ei


def run(dev, x, ei, D, radius, **kw):
    got = P.add_world_edges(torch.from_numpy(x).to(dev), torch.from_numpy(ei).to(dev), POS0, POS0 + D, TYPE_COL, radius=radius, **kw)
    assert got.dtype == torch.int64 and got.shape[0] == 2
    return got.cpu().numpy()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_world_edges_around_the_tile(dev, D, N):
    rng = np.random.default_rng(100 * D + N)
    pos = rng.random((N, D)).astype(np.float32)
    types = rng.choice([0.0, 1.0, 3.0], size=N, p=[0.5, 0.3, 0.2])
    x = make_x(pos, types)
    radius = 0.08 if D == 2 else 0.2
    for E in (0, 2 * N):   # E = 0: world pairs only
        ei = mesh_edges(N, E, N + E) if E else np.zeros((2, 0), dtype=np.int64)
        want, pairs = world_edges_reference(x, ei, D, radius)
        assert N == 1 or pairs > N // 4   # the case really adds world edges
        got = run(dev, x, ei, D, radius)
        assert np.array_equal(got, want), (D, N, E)
        # max_world_pairs equal to the pair count passes, one less raises
        assert np.array_equal(run(dev, x, ei, D, radius, max_world_pairs=pairs), want)
        if pairs:
            with pytest.raises(RuntimeError, match="max_world_pairs"):
                run(dev, x, ei, D, radius, max_world_pairs=pairs - 1)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("N", [257, 513])
@pytest.mark.parametrize("obstacles_last", [True, False])
def test_partners_in_another_tile(dev, D, N, obstacles_last):
    """one kind only in the last, partial tile (padded with 'neither' in LDS), its partners only in the first tile"""
    rng = np.random.default_rng(7 * N + D)
    pos = (rng.random((N, D)) * 0.1).astype(np.float32)   # everything within reach of everything else or nearly
    first, last = np.arange(N) < 256, np.arange(N) >= (N - 1) // 256 * 256
    types = np.full(N, 3.0)
    types[last], types[first] = (1.0, 0.0) if obstacles_last else (0.0, 1.0)
    x = make_x(pos, types)
    ei = mesh_edges(N, 300, N)
    want, pairs = world_edges_reference(x, ei, D, 0.05)
    assert pairs >= 20 and pairs < int(last.sum()) * 256
    assert np.array_equal(run(dev, x, ei, D, 0.05), want)


@pytest.mark.parametrize("D", [2, 3])
def test_pairs_exactly_at_the_radius_and_coincident_points(dev, D):
    side = 17 if D == 2 else 7
    grid = np.stack(np.meshgrid(*[np.arange(side)] * D, indexing="ij"), axis=-1).reshape(-1, D)
    types = (grid.sum(axis=1) % 2).astype(np.float32)   # checkerboard: every lattice neighbour is of the other kind
    pos = grid.astype(np.float32) * np.float32(0.25)
    assert pos.shape[0] > 256
    x = make_x(pos, types)
    none = np.zeros((2, 0), dtype=np.int64)
    want, pairs = world_edges_reference(x, none, D, 0.25)
    assert pairs == D * side ** (D - 1) * (side - 1)       # every lattice edge, each exactly at the radius
    assert np.array_equal(run(dev, x, none, D, 0.25), want)
    assert run(dev, x, none, D, 0.2499999).shape[1] == 0
    # coincident obstacle / normal points, radius 0
    pos2 = np.concatenate([pos[:40], pos[:40], pos[:5]])
    types2 = np.concatenate([np.ones(40), np.zeros(40), np.zeros(5)]).astype(np.float32)
    x2 = make_x(pos2, types2)
    want2, pairs2 = world_edges_reference(x2, none, D, 0.0)
    assert pairs2 == 45
    assert np.array_equal(run(dev, x2, none, D, 0.0), want2)


@pytest.mark.parametrize("D", [2, 3])
def test_no_obstacle_returns_the_input_symmetrised(dev, D):
    N = 300
    rng = np.random.default_rng(D)
    x = make_x((rng.random((N, D)) * 0.05).astype(np.float32), rng.choice([0.0, 3.0, 5.0], size=N))
    ei = mesh_edges(N, 500, 3)
    assert (ei[0] == ei[1]).any()
    got = run(dev, x, ei, D, 0.5)
    key = np.unique(np.concatenate([ei[0] * N + ei[1], ei[1] * N + ei[0]]))
    assert np.array_equal(got, np.stack([key // N, key % N]))        # symmetrised, coalesced, self loops kept
    assert np.array_equal(got, world_edges_reference(x, ei, D, 0.5)[0])
    assert (got[0] == got[1]).any()


@pytest.mark.parametrize("D", [2, 3])
def test_non_integral_types_link_to_nothing(dev, D):
    """the reference compares the float: 1.5 is no OBSTACLE, 0.5 no NORMAL (a truncating kernel links both)"""
    N = 260
    rng = np.random.default_rng(40 + D)
    pos = (rng.random((N, D)) * 0.05).astype(np.float32)   # all within the radius of each other
    types = np.where(np.arange(N) % 2 == 0, 1.0, 0.0)
    odd = {3: 1.5, 4: 0.5, 258: 1.5, 259: 0.5, 100: -0.5, 101: 1.25}
    for i, v in odd.items():
        types[i] = v
    x = make_x(pos, types)
    none = np.zeros((2, 0), dtype=np.int64)
    want, pairs = world_edges_reference(x, none, D, 0.2)
    assert pairs == 127 * 127 and not np.isin(want, list(odd)).any()
    got = run(dev, x, none, D, 0.2, max_world_pairs=130 * 130)   # room for what a truncating kernel would link as well
    assert not np.isin(got, list(odd)).any()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ edge features
def _ulp_distance_check(got, want64):
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want64) <= 2.0 * ulp)
    assert np.array_equal(got[want64 == 0.0], np.zeros(int((want64 == 0.0).sum()), dtype=np.float32))


def _edge_feature_case(dev, pos, ei, with_out):
    D, E = pos.shape[1], ei.shape[1]
    p, e = torch.from_numpy(pos).to(dev), torch.from_numpy(ei).to(dev)
    if with_out:
        out = torch.full((E, D + 1), float("nan"), dtype=torch.float32, device=dev)
        got = P.edge_features(p, e, out=out)
        assert got is out
    else:
        got = P.edge_features(p, e)
    got = got.cpu().numpy()
    assert got.shape == (E, D + 1) and got.dtype == np.float32
    p64 = pos.astype(np.float64)
    diff = p64[ei[0]] - p64[ei[1]]
    assert np.array_equal(got[:, :D].view(np.int32), diff.astype(np.float32).view(np.int32))   # bit for bit
    _ulp_distance_check(got[:, D], np.sqrt((diff ** 2).sum(axis=1)))
    return got


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("E", [0, 1, 255, 256, 257])
def test_edge_features_around_the_block(dev, D, E):
    rng = np.random.default_rng(10 * E + D)
    N = 64
    pos = (rng.integers(0, 2 ** 16, size=(N, D)).astype(np.float64) / 2 ** 16).astype(np.float32)   # 2^-16 grid: exact differences
    pos[1] = pos[0]                                                                                 # coincident nodes
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    if E >= 1:
        ei[:, E - 1] = (5, 5)        # a self loop in the last row
    if E >= 255:
        ei[:, 0] = (0, 1)            # coincident end points
        ei[:, E // 2] = (1, 0)
    for with_out in (False, True):
        got = _edge_feature_case(dev, pos, ei, with_out)
        if E >= 1:
            assert np.array_equal(got[E - 1].view(np.int32), np.zeros(D + 1, dtype=np.int32))   # exactly +0
        if E >= 255:
            assert not got[0].any() and not got[E // 2].any()


@pytest.mark.parametrize("D", [2, 3])
def test_edge_features_small_differences_of_large_coordinates(dev, D):
    rng = np.random.default_rng(D)
    N, E = 200, 700
    step = 2.0 ** -10   # the spacing of fp32 numbers in [8192, 16384)
    pos = (10000.0 + rng.integers(-40, 41, size=(N, D)) * step).astype(np.float32)
    assert np.array_equal(pos.astype(np.float64), 10000.0 + np.round((pos.astype(np.float64) - 10000.0) / step) * step)
    ei = rng.integers(0, N, size=(2, E)).astype(np.int64)
    got = _edge_feature_case(dev, pos, ei, False)
    assert 0 < np.abs(got[:, :D]).max() <= 80 * step and np.abs(got[:, :D])[got[:, :D] != 0].min() == step


def test_edge_features_refuses_other_dimensions(dev):
    ei = torch.zeros(2, 3, dtype=torch.int64, device=dev)
    for D in (1, 4):
        with pytest.raises(ValueError):
            P.edge_features(torch.zeros(5, D, device=dev), ei)
