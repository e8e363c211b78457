"""GPU: exact k-nearest-neighbour search, inverse-distance interpolation and the pooling modules built on them
(csrc/mgn_knn.hip through preprocess.knn / knn_graph / min_distance_to_type and hierarchical_pooling) against the numpy
restatement of tests/knn_reference.py.

The search is compared WITHOUT a tolerance: indices with ``np.array_equal``, squared distances bit for bit -- the contract of
include/mgn_hip.h fixes the operation order and the order of ties.  The interpolation is compared per element against fp64
within ``4 (k + 2) 2^-24 sum_j a_j |x[idx_j]|``: one rounding per weight, per normalisation and per accumulate, a factor 4 of
slack.  The modules' round trip also crosses two Linear layers and is held to the project's fp32 parity bar (1e-5 of the
tensor's scale, conftest.rel_err)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import knn_reference as KR
import recipe as R
import graph_physics_amd as gp
from conftest import rel_err
from graph_physics_amd import _capi, preprocess as P
from graph_physics_amd import hierarchical_pooling as HP

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
PARITY = 1e-5


def _search(x, y, k, dev, ptr_x=None, ptr_y=None, exclude_self=False):
    """the raw search on numpy inputs -> (idx, d2) as numpy"""
    ptr_x = [0, len(x)] if ptr_x is None else ptr_x
    ptr_y = [0, len(y)] if ptr_y is None else ptr_y
    px, py = (torch.tensor(p, dtype=torch.int64, device=dev) for p in (ptr_x, ptr_y))
    idx, d2 = P._knn_search(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), k, px, py, len(ptr_x) - 1, exclude_self)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(y), k)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same(got, want):
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.int32), wd.view(np.int32))      # bit for bit, +inf in the empty slots included


_cache = {}


def _points(dim):
    """(references, queries) drawn once per dimension; the sizes of a case are prefixes"""
    if dim not in _cache:
        T = _capi.lib().mgn_knn_tile_points()
        rng = np.random.default_rng(100 + dim)
        _cache[dim] = (rng.uniform(0, 1, (2 * T + 1, dim)).astype(np.float32), rng.uniform(0, 1, (257, dim)).astype(np.float32))
    return _cache[dim]


def _want32(dim, nx, ny):
    """the restatement at k = 32, computed once per shape: the answer for a smaller k is its first k columns"""
    key = (dim, nx, ny)
    if key not in _cache:
        x, y = _points(dim)
        _cache[key] = KR.knn_reference(x[:nx], y[:ny], 32)
    return _cache[key]


@pytest.mark.parametrize("k", [1, 3, 6, 16, 32])
@pytest.mark.parametrize("dim", [2, 3])
def test_search_around_the_tile_and_the_wave(dev, dim, k):
    T = _capi.lib().mgn_knn_tile_points()
    x, y = _points(dim)
    for nx in (T - 1, T, T + 1, 2 * T + 1):
        for ny in (1, 63, 64, 65, 257):
            wi, wd = _want32(dim, nx, ny)
            _same(_search(x[:nx], y[:ny], k, dev), (wi[:, :k].copy(), wd[:, :k].copy()))


@pytest.mark.parametrize("dim", [2, 3])
def test_search_in_a_batch_with_an_empty_and_a_small_segment(dev, dim):
    rng = np.random.default_rng(7)
    ptr_x, ptr_y = [0, 1, 71, 71, 200], [0, 2, 67, 71, 201]      # references (1, 70, 0, 129), queries (2, 65, 4, 130)
    x, y = rng.uniform(0, 1, (200, dim)).astype(np.float32), rng.uniform(0, 1, (201, dim)).astype(np.float32)
    k = 6
    want = KR.knn_reference(x, y, k, ptr_x, ptr_y)
    got = _search(x, y, k, dev, ptr_x, ptr_y)
    _same(got, want)
    assert (got[0][:2, 0] == 0).all() and (got[0][:2, 1:] == -1).all()          # one reference: k - 1 empty slots
    assert (got[0][67:71] == -1).all() and np.isinf(got[1][67:71]).all()         # no reference at all
    assert (got[0][2:67] >= 1).all() and (got[0][2:67] < 71).all() and (got[0][71:] >= 71).all()   # nobody leaves its segment
    # the public call, from host offsets and from batch vectors
    wa = KR.assign_index(want[0])
    assert wa.shape[1] == 2 * 1 + 65 * k + 0 + 130 * k < 201 * k
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    bx = torch.repeat_interleave(torch.arange(4), torch.tensor(np.diff(ptr_x))).to(dev)
    by = torch.repeat_interleave(torch.arange(4), torch.tensor(np.diff(ptr_y))).to(dev)
    for a in (P.knn(xd, yd, k, ptr_x=ptr_x, ptr_y=torch.tensor(ptr_y)), P.knn(xd, yd, k, bx, by), gp.knn(xd, yd, k, batch_x=bx, ptr_y=ptr_y)):
        assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy(), wa)
    # no batch: one segment, nothing to drop
    a = P.knn(xd, yd, 3)
    assert a.shape == (2, 201 * 3) and np.array_equal(a.cpu().numpy(), KR.assign_index(KR.knn_reference(x, y, 3)[0]))
    with pytest.raises(ValueError):
        P.knn(xd, yd, 3, ptr_x=[0, 1, 200], ptr_y=ptr_y)
    with pytest.raises(ValueError):
        P.knn(xd, yd, 3, ptr_x=[0, 1, 71, 71, 199], ptr_y=ptr_y)
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError):
            P.knn(xd, yd, bad)


@pytest.mark.parametrize("k", [4, 6, 32])
def test_ties_on_integer_lattices_go_to_the_lower_index(dev, k):
    g = np.arange(12, dtype=np.float32)
    lat2 = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)            # 144 points, distances tie in fours and eights
    lat3 = np.stack(np.meshgrid(g[:6], g[:6], g[:6], indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    for lat in (lat2, lat3, lat2[rng.permutation(len(lat2))], lat3[rng.permutation(len(lat3))]):
        want = KR.knn_reference(lat, lat, k, exclude_self=True)
        ties = (np.diff(want[1], axis=1) == 0).sum()
        assert ties > len(lat)                                                           # the case is about ties
        _same(_search(lat, lat, k, dev, exclude_self=True), want)
        _same(_search(lat, lat, k, dev), KR.knn_reference(lat, lat, k))


def test_coincident_points_cost_no_neighbour_with_exclude_self(dev):
    rng = np.random.default_rng(11)
    base = rng.uniform(0, 1, (90, 3)).astype(np.float32)
    pts = np.concatenate([base, base[:40], base[:10]])[rng.permutation(140)]             # 40 points twice, 10 of them three times
    want = KR.knn_reference(pts, pts, 6, exclude_self=True)
    got = _search(pts, pts, 6, dev, exclude_self=True)
    _same(got, want)
    assert not (got[0] == np.arange(140)[:, None]).any()                                 # never itself ...
    assert (got[1][:, 0] == 0).sum() == 2 * 40 + 10                                      # ... but its twins, at distance 0
    assert (got[0] >= 0).all()
    # and without exclude_self the node and its twins come first, lowest index first
    _same(_search(pts, pts, 6, dev), KR.knn_reference(pts, pts, 6))


@pytest.mark.parametrize("case", ["delaunay2d", "points3d"])
def test_knn_graph(dev, case):
    pos = R.delaunay_graph(3000, 7)[0].numpy() if case == "delaunay2d" else np.random.default_rng(9).uniform(0, 1, (1500, 3)).astype(np.float32)
    N = len(pos)
    pd = torch.from_numpy(pos).to(dev)
    got = P.knn_graph(pd, 6).cpu().numpy()
    want = KR.knn_graph_reference(pos, 6)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got.shape == (2, 6 * N) and not (got[0] == got[1]).any()                      # (neighbour, centre), no self loops
    assert np.array_equal(got[1], np.repeat(np.arange(N), 6))
    assert np.array_equal(P.knn_graph(pd, 6, flow="target_to_source").cpu().numpy(), want[::-1])
    loops = P.knn_graph(pd, 3, loop=True).cpu().numpy()
    assert np.array_equal(loops, KR.knn_graph_reference(pos, 3, loop=True)) and (loops[0, ::3] == loops[1, ::3]).all()
    und = P.knn_graph(pd, 6, force_undirected=True).cpu().numpy()
    assert und.dtype == np.int64 and np.array_equal(und, KR.to_undirected(want, N))      # values and order
    assert not (und[0] == und[1]).any()
    pairs = set(map(tuple, und.T.tolist()))
    assert len(pairs) == und.shape[1] and all((j, i) in pairs for i, j in pairs)
    # a batch of two graphs: the halves do not see each other
    half = N // 2
    batch = (torch.arange(N) >= half).long().to(dev)
    b = P.knn_graph(pd, 6, batch, force_undirected=True).cpu().numpy()
    assert np.array_equal(b, KR.knn_graph_reference(pos, 6, [0, half, N], force_undirected=True))
    assert ((b[0] < half) == (b[1] < half)).all()


def _interp_case(dev, k, seed=21, nx=100, ny=300, dim=3):
    """coarse nodes = every third fine node (so a third of the queries coincide with a coarse node) plus one coarse node far away"""
    rng = np.random.default_rng(seed)
    fine = rng.uniform(0, 1, (ny, dim)).astype(np.float32)
    coarse = np.concatenate([fine[::3][:nx - 1], np.full((1, dim), 50.0, dtype=np.float32)])
    idx, d2 = _search(coarse, fine, k, dev)
    _same((idx, d2), KR.knn_reference(coarse, fine, k))
    return fine, coarse, idx, d2


@pytest.mark.parametrize("Fw", [1, 3, 128, 130])
@pytest.mark.parametrize("k", [3, 6])
def test_interpolation_forward(dev, k, Fw):
    fine, coarse, idx, d2 = _interp_case(dev, k)
    x = np.random.default_rng(Fw).standard_normal((len(coarse), Fw)).astype(np.float32)
    got = gp.knn_interpolate(torch.from_numpy(x).to(dev), torch.from_numpy(coarse).to(dev), torch.from_numpy(fine).to(dev), k=k)
    assert got.dtype == torch.float32 and got.shape == (len(fine), Fw)
    got = got.cpu().numpy().astype(np.float64)
    want, scale = KR.interpolate_reference(x, idx, d2)
    bound = 4 * (k + 2) * U * scale
    excess = np.abs(got - want) - bound
    print(f"k={k} F={Fw}: max |err| / bound = {float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (excess <= 0).all()
    # a query on a coarse node returns that node's row: the clamp gives it weight 1e16
    on = np.arange(0, 3 * (len(coarse) - 1), 3)
    assert (d2[on, 0] == 0).all() and np.array_equal(idx[on, 0], np.arange(len(coarse) - 1))
    assert (np.abs(got[on] - x[:len(coarse) - 1]) <= 4 * (k + 2) * U * np.abs(x[:len(coarse) - 1])).all()


def test_interpolation_with_empty_slots_and_an_empty_segment(dev):
    rng = np.random.default_rng(2)
    ptr_x, ptr_y = [0, 2, 2, 30], [0, 5, 9, 40]
    cx, fy = rng.uniform(0, 1, (30, 2)).astype(np.float32), rng.uniform(0, 1, (40, 2)).astype(np.float32)
    x = rng.standard_normal((30, 5)).astype(np.float32)
    idx, d2 = KR.knn_reference(cx, fy, 4, ptr_x, ptr_y)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = gp.knn_interpolate(xd, torch.from_numpy(cx).to(dev), torch.from_numpy(fy).to(dev), k=4, ptr_x=ptr_x, ptr_y=ptr_y)
    want, scale = KR.interpolate_reference(x, idx, d2)
    assert (np.abs(out.detach().cpu().numpy() - want) <= 4 * 6 * U * scale).all()
    assert not out[5:9].detach().any()                                   # queries of the graph without a coarse node: exactly 0
    dy = rng.standard_normal((40, 5)).astype(np.float32)
    out.backward(torch.from_numpy(dy).to(dev))
    wdx, wscale = KR.interpolate_backward_reference(dy, idx, d2, 30)
    assert (np.abs(xd.grad.cpu().numpy() - wdx) <= 4 * 6 * U * wscale).all()


@pytest.mark.parametrize("Fw", [1, 3, 128, 130])
def test_interpolation_backward(dev, Fw):
    k = 6
    fine, coarse, idx, d2 = _interp_case(dev, k)
    nx = len(coarse)
    rng = np.random.default_rng(40 + Fw)
    x, dy = rng.standard_normal((nx, Fw)).astype(np.float32), rng.standard_normal((len(fine), Fw)).astype(np.float32)
    cd, fd, dyd = (torch.from_numpy(a).to(dev) for a in (coarse, fine, dy))
    grads = []
    for _ in range(2):
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        cd.requires_grad_(True)
        gp.knn_interpolate(xd, cd, fd, k=k).backward(dyd)
        assert cd.grad is None                                            # positions take no gradient
        grads.append(xd.grad.cpu().numpy())
    assert np.array_equal(grads[0].view(np.int32), grads[1].view(np.int32))   # no atomics: two runs, identical bits
    # fp64 autograd of the restated formula
    a = torch.from_numpy(KR.interpolation_weights(idx, d2))
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    (a[..., None] * x64[torch.from_numpy(np.maximum(idx, 0))]).sum(dim=1).backward(torch.from_numpy(dy).double())
    want, scale = KR.interpolate_backward_reference(dy, idx, d2, nx)
    assert np.allclose(x64.grad.numpy(), want, rtol=1e-12, atol=1e-14)
    bound = 4 * (k + 2) * U * scale
    err = np.abs(grads[0].astype(np.float64) - x64.grad.numpy())
    print(f"F={Fw}: max |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}, largest in-degree {int(np.bincount(idx.reshape(-1)).max())}")
    assert (err <= bound).all()
    assert not (idx == nx - 1).any() and not grads[0][nx - 1].any()       # the far coarse node: nobody selected it, exactly 0


def _three_graphs(dev, d_in, seed=31):
    rng = np.random.default_rng(seed)
    sizes = [40, 1, 75]
    ptr = [0] + np.cumsum(sizes).tolist()
    N = ptr[-1]
    pos = torch.from_numpy(rng.uniform(0, 1, (N, 2)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((N, d_in)).astype(np.float32)).to(dev)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(dev)
    return x, pos, batch, ptr


@pytest.mark.parametrize("d_in,d_out", [(16, 32), (11, 7)])     # the engine's fused Linear; widths that fall back to F.linear
def test_downsampler(dev, d_in, d_out):
    torch.manual_seed(0)
    x, pos, batch, ptr = _three_graphs(dev, d_in)
    down = gp.DownSampler(d_in, d_out).to(dev)
    assert HP._engine_linear_ok(d_in, d_out) == (d_in == 16)
    score = down.score(x).cpu().numpy()
    assert len(np.unique(score)) == len(score)                            # distinct scores: the selection is unambiguous
    g = down(x, pos, batch)
    perm = KR.topk_reference(score, 0.25, ptr)
    assert len(perm) == 10 + 1 + 19 and np.array_equal(g.perm.cpu().numpy(), perm)
    assert isinstance(g, gp.Graph) and g.edge_attr is None
    assert g.x.dtype == torch.float32 and g.x.shape == (30, d_out) and g.pos.dtype == torch.float32 and g.pos.shape == (30, 2)
    assert g.batch.dtype == torch.int64 and g.batch.cpu().tolist() == [0] * 10 + [1] + [2] * 19
    assert g.edge_index.dtype == torch.int64 and g.edge_index.shape[0] == 2
    assert torch.equal(g.pos, pos[g.perm])
    want_x = F.linear(x.cpu().double()[perm], down.lin.weight.detach().cpu().double(), down.lin.bias.detach().cpu().double())
    assert rel_err(g.x, want_x) < PARITY
    assert torch.equal(g.edge_index, P.knn_graph(g.pos, 6, g.batch, force_undirected=True))
    assert np.array_equal(g.edge_index.cpu().numpy(), KR.knn_graph_reference(g.pos.cpu().numpy(), 6, [0, 10, 11, 30], force_undirected=True))
    # an attention signal instead of the features decides the selection
    attn = torch.from_numpy(np.random.default_rng(1).standard_normal((x.shape[0], d_in)).astype(np.float32)).to(dev)
    g2 = down(x, pos, batch, attn=attn)
    assert np.array_equal(g2.perm.cpu().numpy(), KR.topk_reference(down.score(x, attn).cpu().numpy(), 0.25, ptr))
    assert not torch.equal(g2.perm, g.perm)


@pytest.mark.parametrize("d_in,d_mid", [(16, 32), (11, 7)])
def test_pooling_round_trip_gradients(dev, d_in, d_mid):
    torch.manual_seed(1)
    x, pos, batch, ptr = _three_graphs(dev, d_in)
    down, up = gp.DownSampler(d_in, d_mid).to(dev), gp.UpSampler(d_mid, d_in, k=3).to(dev)
    x.requires_grad_(True)
    pos.requires_grad_(True)
    g = down(x, pos, batch)
    out = up(g.x, g.pos, pos, g.batch, batch)
    assert out.shape == x.shape and out.dtype == torch.float32
    dout = torch.from_numpy(np.random.default_rng(3).standard_normal(tuple(out.shape)).astype(np.float32)).to(dev)
    out.backward(dout)
    assert down.select.weight.grad is None and pos.grad is None           # nothing else takes a gradient
    got = [x.grad, down.lin.weight.grad, down.lin.bias.grad, up.lin.weight.grad, up.lin.bias.grad]
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in got)
    # the same construction with torch ops in fp64: index_select, the restated weights, F.linear
    perm = g.perm.cpu()
    ptr_c = [0, 10, 11, 30]
    idx, d2 = KR.knn_reference(g.pos.detach().cpu().numpy(), pos.detach().cpu().numpy(), 3, ptr_c, ptr)
    a = torch.from_numpy(KR.interpolation_weights(idx, d2))
    x64 = x.detach().cpu().double().requires_grad_(True)
    ps = [p.detach().cpu().double().requires_grad_(True) for p in (down.lin.weight, down.lin.bias, up.lin.weight, up.lin.bias)]
    xc = F.linear(x64.index_select(0, perm), ps[0], ps[1])
    interp = (a[..., None] * xc[torch.from_numpy(np.maximum(idx, 0))]).sum(dim=1)
    want_out = F.linear(interp, ps[2], ps[3])
    want_out.backward(dout.cpu().double())
    assert rel_err(out, want_out) < PARITY
    for name, t, w in zip(("x", "down.lin.weight", "down.lin.bias", "up.lin.weight", "up.lin.bias"), got, [x64.grad] + [p.grad for p in ps]):
        assert t.shape == w.shape and rel_err(t, w) < PARITY, name
    unselected = np.setdiff1d(np.arange(x.shape[0]), perm.numpy())
    assert not x.grad[torch.from_numpy(unselected).to(dev)].any()         # a node that was not kept: exactly 0


def test_min_distance_to_type(dev):
    rng = np.random.default_rng(17)
    pos = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    types = rng.choice([0.0, 4.0, 6.0], size=500, p=[0.8, 0.1, 0.1]).astype(np.float32)
    g = gp.Graph(pos=torch.from_numpy(pos).to(dev), batch=torch.zeros(500, dtype=torch.int64, device=dev))
    td = torch.from_numpy(types).to(dev)
    got = gp.min_distance_to_type(g, gp.NodeType.WALL_BOUNDARY, td)
    assert got.dtype == torch.float32 and got.shape == (500,)
    want = np.sqrt(KR.knn_reference(pos[types == 6.0], pos, 1)[1][:, 0])
    assert want.dtype == np.float32 and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not got[td == 6.0].any() and bool((got[td != 6.0] > 0).all())
    # the reference's broadcast formula (dataset/preprocessing.py:241-274), with torch on the device
    p = g.pos
    upstream = torch.min(torch.sqrt(torch.sum((p.unsqueeze(1) - p[td == 6.0].unsqueeze(0)) ** 2, dim=-1)), dim=1)[0]
    assert torch.allclose(got, upstream, rtol=1e-6, atol=0)
    g2 = gp.Graph(pos=g.pos[:, :2].contiguous())
    want2 = np.sqrt(KR.knn_reference(pos[types == 4.0][:, :2], pos[:, :2], 1)[1][:, 0])
    assert np.array_equal(gp.min_distance_to_type(g2, 4, td).cpu().numpy().view(np.int32), want2.view(np.int32))
    with pytest.raises(ValueError, match="no node of type"):
        gp.min_distance_to_type(g, gp.NodeType.OBSTACLE, td)
