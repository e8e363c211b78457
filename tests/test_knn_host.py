"""CPU: the host side of the k-nearest-neighbour feature -- the numpy restatement (tests/knn_reference.py) against hand-written
answers and against scipy's k-d tree, the C ABI of csrc/mgn_knn.hip (declared, exported, prototyped; every argument error
refused before a launch), the pooling modules' parameters and the ``ceil(ratio * n)`` arithmetic.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import knn_reference as KR

KNN_SYMBOLS = ("mgn_knn_max_k", "mgn_knn_tile_points", "mgn_knn_search", "mgn_knn_interp_fwd", "mgn_knn_interp_bwd", "mgn_knn_last_error")


def test_restatement_on_a_five_point_line():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [4.0, 0.0], [8.0, 0.0]], dtype=np.float32)
    idx, d2 = KR.knn_reference(x, x, 2, exclude_self=True)
    assert idx.dtype == np.int64 and d2.dtype == np.float32
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0], [2, 1], [3, 2]]        # node 2: 0 and 3 tie at 4, the lower index wins
    assert d2.tolist() == [[1.0, 4.0], [1.0, 1.0], [1.0, 4.0], [4.0, 9.0], [16.0, 36.0]]
    idx, d2 = KR.knn_reference(x, x, 2)                                     # with itself: every node is its own nearest
    assert idx[:, 0].tolist() == [0, 1, 2, 3, 4] and not d2[:, 0].any()
    assert KR.assign_index(idx).tolist() == [[0, 0, 1, 1, 2, 2, 3, 3, 4, 4], [0, 1, 1, 0, 2, 1, 3, 2, 4, 3]]
    # two segments (3 + 2 points): the second one runs out of references at k = 2 with exclude_self
    idx, d2 = KR.knn_reference(x, x, 2, [0, 3, 5], [0, 3, 5], exclude_self=True)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0], [4, -1], [3, -1]]
    assert np.isinf(d2[3:, 1]).all() and d2[3:, 0].tolist() == [16.0, 16.0]
    assert KR.assign_index(idx).shape == (2, 8)
    g = KR.knn_graph_reference(x, 1)                                        # (neighbour, centre)
    assert g.tolist() == [[1, 0, 1, 2, 3], [0, 1, 2, 3, 4]]
    assert KR.knn_graph_reference(x, 1, flow="target_to_source").tolist() == [[0, 1, 2, 3, 4], [1, 0, 1, 2, 3]]
    und = KR.knn_graph_reference(x, 1, force_undirected=True)
    assert und.T.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2], [3, 4], [4, 3]]


def test_restatement_on_a_lattice_with_four_equidistant_neighbours():
    xs, ys = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    x = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)    # node 3 i + j at (i, j); the centre is node 4
    idx, d2 = KR.knn_reference(x, x, 4, exclude_self=True)
    assert idx[4].tolist() == [1, 3, 5, 7] and d2[4].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert idx[0].tolist() == [1, 3, 4, 2] and d2[0].tolist() == [1.0, 1.0, 2.0, 4.0]   # 2 and 6 tie at 4: the lower index
    idx3, _ = KR.knn_reference(x, x, 3, exclude_self=True)
    assert idx3[4].tolist() == [1, 3, 5]                                             # the tie is cut at the lower indices
    x3 = np.concatenate([x, np.zeros((9, 1), dtype=np.float32)], axis=1)             # the same lattice in 3-D
    assert np.array_equal(KR.knn_reference(x3, x3, 4, exclude_self=True)[0], idx)
    # wide rows take the restatement's short cut (only entries up to the k-th smallest value are ordered): same answer as
    # ordering whole rows, on a lattice full of ties
    g = np.arange(15, dtype=np.float32)
    big = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    D = KR.squared_distances(big, big)
    full = np.lexsort((np.broadcast_to(np.arange(225), D.shape), D), axis=-1)[:, :6]
    d_fast, i_fast = KR._first_k(D, 6)
    assert np.array_equal(i_fast, full) and np.array_equal(d_fast, np.take_along_axis(D, full, axis=1))
    # coincident points: the node itself is dropped by index, its twin stays
    twin = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]], dtype=np.float32)
    idx, d2 = KR.knn_reference(twin, twin, 2, exclude_self=True)
    assert idx.tolist() == [[1, 2], [0, 2], [0, 1]] and d2[:2, 0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dim", [2, 3])
def test_restatement_against_the_kd_tree(dim):
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    rng = np.random.default_rng(3 + dim)
    x = rng.uniform(0, 1, (400, dim)).astype(np.float32)
    y = rng.uniform(0, 1, (150, dim)).astype(np.float32)
    idx, d2 = KR.knn_reference(x, y, 7)
    assert (np.diff(d2.astype(np.float64), axis=1) > 0).all()                        # tie-free, so the order is the tree's
    dist, want = cKDTree(x.astype(np.float64)).query(y.astype(np.float64), k=7)
    assert np.array_equal(idx, want)
    assert np.allclose(np.sqrt(d2.astype(np.float64)), dist, rtol=1e-5, atol=0)


def test_restated_selection_and_interpolation():
    assert KR.num_selected(0.25, [1, 4, 5, 1885, 150000]).tolist() == [1, 1, 2, 472, 37500]
    score = np.array([0.1, 0.9, 0.5, 0.3, 0.2, 0.8, 0.7])
    assert KR.topk_reference(score, 0.5, [0, 4, 7]).tolist() == [1, 2, 5, 6]
    assert KR.topk_reference(score, 0.25, [0, 4, 4, 7]).tolist() == [1, 5]           # an empty graph keeps nothing
    x = np.array([[1.0, 10.0], [3.0, 30.0], [100.0, 1000.0]])
    idx = np.array([[0, 1], [1, -1], [2, 0]])
    d2 = np.array([[1.0, 1.0], [4.0, np.inf], [0.0, 1.0]], dtype=np.float32)
    out, scale = KR.interpolate_reference(x, idx, d2)
    assert np.allclose(out[0], [2.0, 20.0]) and np.allclose(out[1], [3.0, 30.0])
    assert np.allclose(out[2], [100.0, 1000.0], rtol=1e-12)                          # a coincident node: weight 1e16
    assert np.allclose(scale, np.abs(out))
    dx, _ = KR.interpolate_backward_reference(np.ones((3, 2)), idx, d2, 4)
    assert np.allclose(dx.sum(axis=0), [3.0, 3.0]) and not dx[3].any()               # weights sum to 1 per query


def test_knn_symbols_declared_exported_and_prototyped():
    from conftest import REPO
    from graph_physics_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mgn_hip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in KNN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in mgn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.SYMBOLS, f"{name} has no ctypes prototype"
    assert any(s.endswith("mgn_knn.hip") for s in _capi.SOURCES)
    assert "mgn_knn.hip" in open(os.path.join(REPO, "graph-physics_amd", "csrc", "Makefile")).read()
    assert lib.mgn_version() == _capi.EXPECTED_VERSION == 136   # additive change: the ABI number stays
    assert lib.mgn_knn_max_k() == 32
    assert lib.mgn_knn_tile_points() > 0 and lib.mgn_knn_tile_points() % 4 == 0


def test_knn_argument_errors_are_refused_before_any_launch():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)      # a host address: a call that launched anything would fault, these return first

    def search(dim=2, k=3, nseg=1, nx=10, ny=10, x=p, y=p, ptr_x=p, ptr_y=p, idx=p, d2=p):
        return lib.mgn_knn_search(x, nx, y, ny, dim, k, ptr_x, ptr_y, nseg, 0, idx, d2, None)

    err = lib.mgn_knn_last_error
    for dim in (1, 4, 0):
        assert search(dim=dim) == 1 and b"dim must be 2 or 3" in err()
    assert search(k=0) == 1 and b"k must be >= 1" in err()
    assert search(k=-3) == 1 and b"k must be >= 1" in err()
    assert search(k=33) == 1 and b"mgn_knn_max_k" in err()
    assert search(nseg=0) == 1 and b"nseg" in err()
    assert search(nx=-1) == 1 and b"nx and ny" in err()
    assert search(ny=2 ** 31) == 1 and b"nx and ny" in err()
    assert search(x=None) == 1 and b"x must not be null" in err()
    assert search(y=None) == 1 and b"y / idx / d2" in err()
    assert search(idx=None) == 1 and b"y / idx / d2" in err()
    assert search(d2=None) == 1 and b"y / idx / d2" in err()
    assert search(ptr_x=None) == 1 and b"ptr_x / ptr_y" in err()
    assert search(ptr_y=None) == 1 and b"ptr_x / ptr_y" in err()
    # empty inputs are not errors, and launch nothing: no queries; no references needs no x
    assert search(ny=0, y=None, idx=None, d2=None) == 0
    assert search(nx=0, ny=0, x=None, y=None, idx=None, d2=None) == 0

    def fwd(F=4, k=3, nx=10, ny=10, x=p, idx=p, d2=p, a=p, out=p):
        return lib.mgn_knn_interp_fwd(x, nx, F, idx, d2, ny, k, a, out, None)

    assert fwd(F=0) == 1 and b"F must be >= 1" in err()
    assert fwd(k=0) == 1 and b"k must be in" in err()
    assert fwd(k=33) == 1 and b"k must be in" in err()
    assert fwd(x=None) == 1 and b"x must not be null" in err()
    assert fwd(a=None) == 1 and b"idx / d2 / a / out" in err()
    assert fwd(ny=0, idx=None, d2=None, a=None, out=None) == 0

    def bwd(F=4, k=3, nx=10, ny=10, dy=p, a=p, rowptr=p, perm=p, dx=p):
        return lib.mgn_knn_interp_bwd(dy, a, rowptr, perm, nx, ny, k, F, dx, None)

    assert bwd(F=0) == 1 and b"F must be >= 1" in err()
    assert bwd(k=40) == 1 and b"k must be in" in err()
    assert bwd(dx=None) == 1 and b"rowptr / dx" in err()
    assert bwd(perm=None) == 1 and b"dy / a / perm" in err()
    assert bwd(nx=0, rowptr=None, dx=None) == 0


def test_pooling_modules_parameters():
    import graph_physics_amd as gp

    up = gp.UpSampler(48, 128)
    assert up.k == 6 and gp.UpSampler(8, 8, k=3).k == 3
    assert {k: tuple(v.shape) for k, v in up.state_dict().items()} == {"lin.weight": (128, 48), "lin.bias": (128,)}
    down = gp.DownSampler(128, 64)
    assert down.ratio == 0.25 and gp.DownSampler(8, 8, ratio=0.5).ratio == 0.5
    assert {k: tuple(v.shape) for k, v in down.state_dict().items()} == {"lin.weight": (64, 128), "lin.bias": (64,), "select.weight": (1, 128)}
    assert float(down.select.weight.detach().abs().max()) <= 1.0 / np.sqrt(128.0)
    for name in ("knn", "knn_graph", "min_distance_to_type", "knn_interpolate", "UpSampler", "DownSampler"):
        assert hasattr(gp, name)


def test_number_of_selected_nodes_is_ceil_ratio_n_in_fp32():
    from graph_physics_amd import hierarchical_pooling as HP

    n = np.arange(0, 5000)
    for ratio in (0.25, 0.5, 0.1, 0.3, 1.0):
        got = HP.num_selected(ratio, n)
        assert got.dtype == np.int64
        assert np.array_equal(got, KR.num_selected(ratio, n))
        # PyG's arithmetic, on torch: (ratio * n.to(float32)).ceil()
        assert np.array_equal(got, (float(ratio) * torch.from_numpy(n).to(torch.float32)).ceil().to(torch.long).numpy())
    assert HP.num_selected(0.25, [1, 4, 5, 1885, 150000]).tolist() == [1, 1, 2, 472, 37500]


def test_cpu_tensors_raise():
    import graph_physics_amd as gp

    pos = torch.rand(10, 2)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.knn(pos, pos, 3)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.knn_graph(pos, 3)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.knn_interpolate(torch.rand(10, 4), pos, pos)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.min_distance_to_type(gp.Graph(pos=pos), gp.NodeType.WALL_BOUNDARY, torch.zeros(10))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.DownSampler(16, 16)(torch.rand(10, 16), pos, torch.zeros(10, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        gp.UpSampler(16, 16)(torch.rand(10, 16), pos, pos)
    with pytest.raises(ValueError, match="flow"):
        gp.knn_graph(pos, 3, flow="sideways")
