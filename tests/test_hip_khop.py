"""GPU: k-hop edge sets built on the device (csrc/mgn_khop.hip through preprocess.khop_edges / khop_graph /
build_preprocessing(khop=...)) against the scipy formulation of tests/khop_reference.py.  Integer work throughout: every
comparison of indices is ``np.array_equal`` (values, order and the int64 dtype), there is no tolerance.  Both search paths
are pinned from the overflow count the C ABI returns: the hub case must use the bitmap path, the 2-D mesh must not."""
import numpy as np
import pytest
import torch

import recipe as R
import graph_physics_amd as gp
from conftest import rel_err
from graph_physics_amd import _capi, preprocess as P
from khop_reference import hub_graph, khop_reference
from oracle import mgn_oracle as O

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-5   # the bound of test_hip_parity.test_epd_shipped_json_shape


def _run(ei, N, k, dev):
    """(edge_index as numpy, rows that took the bitmap path)"""
    out, n_ovf = P._khop(torch.as_tensor(ei).to(dev), N, k)
    assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] == 2
    return out.cpu().numpy(), n_ovf


def _check(ei, N, k, dev):
    ei = np.asarray(ei)
    got, n_ovf = _run(ei, N, k, dev)
    want = khop_reference(ei, N, k)
    assert got.dtype == want.dtype == np.int64
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    cap = _capi.lib().mgn_khop_row_capacity()
    assert n_ovf == int((np.bincount(want[0], minlength=N) > cap).sum())   # exactly the rows above the capacity
    return want, n_ovf


@pytest.mark.parametrize("k,edges", [(2, 3554), (3, 10807), (5, 49824)])
def test_khop_random_graph(dev, k, edges):
    """unsorted input with a duplicate, a self loop and an isolated node"""
    want, _ = _check(R.random_graph(300, 900, 5).numpy(), 300, k, dev)
    assert want.shape[1] == edges
    assert not (want[0] == 299).any() and not (want[1] == 299).any()   # the isolated node stays isolated


@pytest.mark.parametrize("k,edges", [(2, 59030), (3, 129014), (4, 232184)])
def test_khop_delaunay_2d(dev, k, edges):
    _, ei, _ = R.delaunay_graph(3000, 7)
    want, n_ovf = _check(ei.numpy(), 3000, k, dev)
    assert want.shape[1] == edges
    assert n_ovf == 0   # largest row 202: the on-chip path alone


@pytest.mark.parametrize("k,largest", [(2, 225), (3, 664), (4, 1246)])
def test_khop_tetrahedral(dev, k, largest):
    _, ei, _ = R.delaunay_graph(2000, 9, 3)
    want, _ = _check(ei.numpy(), 2000, k, dev)
    assert int(np.bincount(want[0]).max()) == largest
    if k == 4:
        assert want.shape[1] == 1102292


def test_khop_directed_ring_distance_k_in_k_plus_1_out(dev):
    ring = np.stack([np.arange(64), (np.arange(64) + 1) % 64])
    want, _ = _check(ring, 64, 5, dev)
    got, _ = _run(ring, 64, 5, dev)
    pairs = set(map(tuple, got.T.tolist()))
    assert len(pairs) == 64 * 5
    for i in range(64):
        assert (i, (i + 5) % 64) in pairs and (i, (i + 6) % 64) not in pairs and ((i + 1) % 64, i) not in pairs


def test_khop_path_and_empty(dev):
    path = np.stack([np.arange(0, 9), np.arange(1, 10)])
    want, _ = _check(path, 10, 3, dev)
    assert want.shape[1] == 9 + 8 + 7
    got, n_ovf = _run(np.zeros((2, 0), dtype=np.int64), 5, 2, dev)
    assert got.shape == (2, 0) and got.dtype == np.int64 and n_ovf == 0
    only_loops = np.array([[1, 2], [1, 2]])
    got, _ = _run(only_loops, 4, 2, dev)
    assert got.shape == (2, 0)


def _pairs(*cols):
    """the distinct (row0, row1) columns in ascending order: what coalescing leaves"""
    p = np.concatenate([np.asarray(c, dtype=np.int64).reshape(2, -1) for c in cols], axis=1)
    return np.unique(p, axis=1) if p.shape[1] else p


@pytest.mark.parametrize("case", ["none dropped", "all dropped", "mixed"])
def test_shared_edge_key_convention_on_five_nodes(dev, case):
    """The three callers of the shared sort + unique (khop_edges, faces_to_edges, add_world_edges) against numpy.unique on
    (row0, row1) pairs: a dropped pair gets the all-ones key, all of them collapse into one trailing key, and that one is left
    out -- with no such key in the list, with nothing else in it, and with both kinds."""
    N = 5
    ei, face = {"none dropped": ([[0, 1, 2, 3, 1, 4], [1, 2, 3, 4, 2, 0]], [[0, 1, 2], [1, 2, 3], [2, 3, 4]]),
                "all dropped": ([[1, 2, 2, 4], [1, 2, 2, 4]], [[0, 1, 4], [0, 1, 4], [0, 1, 4]]),
                "mixed": ([[0, 3, 1, 2, 3, 1, 4], [1, 3, 2, 3, 4, 2, 4]], [[0, 1, 2, 4], [0, 2, 2, 4], [1, 2, 3, 4]])}[case]
    ei, face = np.array(ei, dtype=np.int64), np.array(face, dtype=np.int64)

    # khop_edges, two hops: walks of one or two edges, self loops carry nothing, (i, i) is never a pair
    e = ei[:, ei[0] != ei[1]]
    two = [(a, d) for a, b in e.T for c, d in e.T if b == c and a != d]
    got = P.khop_edges(torch.from_numpy(ei).to(dev), N, 2).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, _pairs(e, np.array(two, dtype=np.int64).reshape(-1, 2).T))

    # faces_to_edges: every pair of distinct corners of a face, both ways
    both = [(f[a], f[b]) for f in face.T for a in range(3) for b in range(3) if f[a] != f[b]]
    got = P.faces_to_edges(torch.from_numpy(face).to(dev), N).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, _pairs(np.array(both, dtype=np.int64).reshape(-1, 2).T))

    # add_world_edges: the input in both directions (self loops stay) plus the one OBSTACLE - NORMAL pair in reach, (4, 0).
    # Its key list always ends in unused all-ones slots; "none dropped" leaves the single spare one, "all dropped" only those.
    x = np.zeros((N, 3), dtype=np.float32)                                   # [world x, world y, node type]
    x[:, 0] = np.arange(N)
    wei, world = ei, np.zeros((2, 0), dtype=np.int64)
    if case == "all dropped":
        wei = np.zeros((2, 0), dtype=np.int64)
    if case == "mixed":
        x[4] = (0.01, 0.0, 1.0)
        world = np.array([[4, 0], [0, 4]])
    got = P.add_world_edges(torch.from_numpy(x).to(dev), torch.from_numpy(wei).to(dev), 0, 2, 2, radius=0.03,
                            max_world_pairs=0 if case == "none dropped" else None).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, _pairs(wei, wei[::-1], world))


@pytest.mark.parametrize("k", [2, 3])
def test_khop_both_paths_in_one_call(dev, k):
    """a mesh plus a hub with capacity + 1 leaves: rows of the on-chip path and rows of the bitmap path in one result"""
    cap = _capi.lib().mgn_khop_row_capacity()
    ei, N = hub_graph(cap)
    want, n_ovf = _check(ei, N, k, dev)
    assert n_ovf >= 9                                       # the hub and the 8 leaves that reach it, at least
    assert int(np.bincount(want[0]).max()) > cap
    _, ei2, _ = R.delaunay_graph(3000, 7)
    assert _run(ei2.numpy(), 3000, 2, dev)[1] == 0          # and the plain mesh used the bitmap path for none


def test_khop_block_diagonal_batch(dev):
    n, k = 500, 3
    blocks = [R.delaunay_graph(n, 20 + i)[1].numpy() for i in range(4)]
    batch = np.concatenate([b + i * n for i, b in enumerate(blocks)], axis=1)
    got, _ = _run(batch, 4 * n, k, dev)
    per = [_run(b, n, k, dev)[0] + i * n for i, b in enumerate(blocks)]
    assert np.array_equal(got, np.concatenate(per, axis=1))
    assert np.array_equal(got[0] // n, got[1] // n)         # no pair crosses a block
    assert np.array_equal(got, khop_reference(batch, 4 * n, k))


def test_khop_is_deterministic(dev):
    _, ei, _ = R.delaunay_graph(2000, 9, 3)
    ei = ei.to(dev)
    a, b = P.khop_edges(ei, 2000, 3), P.khop_edges(ei, 2000, 3)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_khop_errors_and_one_hop(dev):
    ei = R.random_graph(50, 200, 1).to(dev)
    assert P.khop_edges(ei, 50, 1) is ei
    with pytest.raises(ValueError):
        P.khop_edges(ei, 50, 0)
    bad = ei.clone()
    bad[1, 17] = 50
    with pytest.raises(IndexError):
        P.khop_edges(bad, 50, 2)
    bad[1, 17] = -1
    with pytest.raises(IndexError):
        P.khop_edges(bad, 50, 2)
    assert np.array_equal(P.khop_edges(ei, 50, 2).cpu().numpy(), khop_reference(ei.cpu().numpy(), 50, 2))   # and works after an error


def _face_mesh(n, seed):
    from scipy.spatial import Delaunay

    pts = np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 2)).astype(np.float32)
    return pts, Delaunay(pts.astype(np.float64)).simplices.T.astype(np.int64)


def _check_graph(g, pos, face, k):
    N = pos.shape[0]
    want = khop_reference(O.faces_to_edges_oracle(face, N), N, k)
    assert np.array_equal(g.edge_index.cpu().numpy(), want)
    ref = O.edge_features_oracle(torch.from_numpy(pos), torch.from_numpy(want))
    got = g.edge_attr.cpu()
    assert got.shape == ref.shape == (want.shape[1], 3)
    assert torch.equal(got[:, :2], ref[:, :2])
    assert rel_err(got[:, 2], ref[:, 2]) < 2e-7             # the bound of test_edge_features_vs_oracle


def test_khop_graph_and_build_preprocessing(dev):
    pos, face = _face_mesh(400, 11)
    N = pos.shape[0]

    def graph(**kw):
        return gp.Graph(x=torch.zeros(N, 3, device=dev), pos=torch.from_numpy(pos).to(dev), face=torch.from_numpy(face).to(dev), **kw)

    g = graph()
    g.edge_index = P.faces_to_edges(g.face, N)
    g.edge_attr = torch.ones(g.edge_index.shape[1], 7, device=dev)          # earlier extra columns are dropped
    _check_graph(P.khop_graph(g, 2), pos, face, 2)
    g = graph()
    g.edge_index = P.faces_to_edges(g.face, N)
    g.edge_attr = torch.ones(g.edge_index.shape[1], 3, device=dev)
    g = P.khop_graph(g, 2, add_edge_features=False)
    assert g.edge_attr is None
    assert np.array_equal(g.edge_index.cpu().numpy(), khop_reference(O.faces_to_edges_oracle(face, N), N, 2))

    cache = {}
    run = P.build_preprocessing(khop=2, khop_cache=cache)
    a = run(graph(traj_index=4))
    _check_graph(a, pos, face, 2)
    assert list(cache) == [4]
    b = run(graph(traj_index=4), 1)
    assert b.edge_index.data_ptr() == a.edge_index.data_ptr() and b.edge_attr.data_ptr() == a.edge_attr.data_ptr()
    c = run(graph(traj_index=5))
    assert c.edge_index.data_ptr() != a.edge_index.data_ptr() and sorted(cache) == [4, 5]
    _check_graph(c, pos, face, 2)
    d = run(graph())                                                         # no trajectory index: computed, not cached
    assert d.edge_index.data_ptr() != a.edge_index.data_ptr() and sorted(cache) == [4, 5]
    # khop = 1: the callable of today
    e = P.build_preprocessing()(graph())
    assert np.array_equal(e.edge_index.cpu().numpy(), O.faces_to_edges_oracle(face, N))
    # and through the config surface
    f = gp.get_preprocessing({"index": {"node_type_index": 2}, "dataset": {"khop": 2}}, dev)(graph(traj_index=0))
    _check_graph(f, pos, face, 2)


def test_epd_forward_on_a_khop_graph(dev):
    """tens of edges per node through ops.Topology and the edge kernels: the model on the k = 2 graph of a 1 500-node mesh
    against the oracle, at the bound and with the comparison of test_epd_shipped_json_shape"""
    L, H, N = 2, 128, 1500
    pos, ei, _ = R.delaunay_graph(N, 31)
    ek = P.khop_edges(ei.to(dev), N, 2)
    assert np.array_equal(ek.cpu().numpy(), khop_reference(ei.numpy(), N, 2))
    assert ek.shape[1] > 15 * N
    ea = P.edge_features(pos.to(dev), ek)
    params = R.make_params(R.epd_param_shapes(L, H, 11, 3, 2), 9)
    net = gp.EncodeProcessDecode(L, 11, 3, 2, hidden_size=H).to(dev)
    net.load_state_dict(params)
    x_in = R.randn((N, 11), 1)
    out = net(gp.Graph(x=x_in.to(dev), edge_attr=ea, edge_index=ek))
    assert rel_err(out, O.epd_forward(x_in, ea.cpu(), ek.cpu(), params, L)) < FWD_TOL
