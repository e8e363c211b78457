"""GPU: the aggregation family of csrc/mgn_kernels.hip -- mgn_csr_build, mgn_topology_build[_async], mgn_segsum, mgn_segsum2,
mgn_segsum2_b16, the hub chunk tables of ops.Topology (segsum_topo) -- and mgn_transpose_blocks, against the references and over
the cases of tests/agg_cases.py.  tests/test_agg_cases_host.py shows on the CPU that those references are CPU ``index_add_`` bit
for bit and that every case has the property it is listed for.

All of it is integer or order-exact work: every assertion here is an equality, a refusal, or the bound of recursive summation
against fp64 (agg_cases.gamma_bound); there is no measured tolerance.  Sources are followed by NaN rows, index arrays by entries
that point at those rows, and outputs start NaN-filled, so a read past a segment's end or a row left unwritten shows in the
result instead of going unnoticed."""
import functools
import time

import numpy as np
import pytest
import torch

import agg_cases as AC
from graph_physics_amd import _capi, ops
from graph_physics_amd._launch import call
from oracle import mgn_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 8     # sentinel rows / entries behind every source and index array
_t0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _t0[0] = time.time()
    yield


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)


def _rows(src, dev):
    """the rows of ``src`` as the leading rows of a buffer that goes on with PAD rows of NaN"""
    src = torch.from_numpy(np.ascontiguousarray(src))
    buf = torch.full((src.shape[0] + PAD, src.shape[1]), NAN, dtype=torch.float32)
    buf[:src.shape[0]] = src
    return buf.to(dev)[:src.shape[0]]


def _perm(perm, n_rows, dev):
    """``perm`` as the leading entries of a buffer that goes on with PAD entries pointing at the first NaN row"""
    buf = np.concatenate([np.asarray(perm, dtype=np.int64), np.full(PAD, n_rows, dtype=np.int64)])
    return _i32(buf, dev)[:len(perm)]


def _nan_out(n, H, dev):
    return torch.full((n, H), NAN, dtype=torch.float32, device=dev)


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    return torch.equal(got.cpu(), torch.from_numpy(want))


@functools.lru_cache(maxsize=None)
def _ladder_refs(H, n):
    """(seq32 over the rows in order, seq32 through the permutation) of one ladder case; computed once, never written to"""
    c = AC.degree_ladder(H, n)
    return AC.seq32(c.src, c.rowptr), AC.seq32(c.src, c.rowptr2, c.perm2)


def _inside_gamma(got, src, rowptr, perm):
    s64, a64 = AC.sum64(src, rowptr, perm)
    return bool((np.abs(got.cpu().numpy().astype(np.float64) - s64) <= AC.gamma_bound(rowptr, a64)).all())


# ---------------------------------------------------------------------------------------------------- CSR
@pytest.mark.parametrize("name", list(AC.csr_cases()))
def test_csr_build_is_the_stable_sort(dev, name):
    c = AC.csr_cases()[name]
    key = torch.from_numpy(c.key)
    rp, pm = ops.csr_build(key.to(dev), c.n)
    orp, opm = O.csr_by_key(key, c.n)
    assert rp.dtype == torch.int32 and pm.dtype == torch.int32 and rp.shape == (c.n + 1,) and pm.shape == (c.key.size,)
    assert torch.equal(rp.cpu(), orp), name
    assert torch.equal(pm.cpu(), opm), name


_TOPO_FIELDS = ("rowptr_dst", "perm_dst", "src_s", "dst_s", "rowptr_src", "perm_src")


@pytest.mark.parametrize("name", list(AC.csr_cases()))
def test_topology_eager_and_lazy(dev, name):
    """the case's keys as destinations, random sources: both CSRs, the sorted endpoints and the degree maxima"""
    c = AC.csr_cases()[name]
    src = AC.random_src(c)
    ei = torch.from_numpy(np.stack([src, c.key])).to(dev)
    want = AC.topology_reference(src, c.key, c.n)
    eager = ops.Topology(ei, c.n)
    lazy = ops.Topology(ei, c.n, lazy=True)
    assert eager.resolved and not lazy.resolved and lazy.max_in_degree is None
    assert lazy.resolve() is lazy and lazy.resolved
    for t in (eager, lazy):
        for f in _TOPO_FIELDS:
            got = getattr(t, f)
            assert got.dtype == torch.int32 and got.shape == want[f].shape, (name, f)
            assert torch.equal(got.cpu(), want[f]), (name, f)
        assert (t.max_in_degree, t.max_out_degree) == (want["max_in_degree"], want["max_out_degree"]), name
        assert (t.hub_dst is not None) == (want["max_in_degree"] > AC.CHUNK) and (t.hub_src is not None) == (want["max_out_degree"] > AC.CHUNK)
    for f in _TOPO_FIELDS:
        assert torch.equal(getattr(eager, f), getattr(lazy, f)), (name, f)


@pytest.mark.parametrize("n", [0, 1, 5])
def test_no_edges_gives_well_formed_arrays(dev, n):
    rp, pm = ops.csr_build(torch.zeros(0, dtype=torch.int64, device=dev), n)
    assert rp.shape == (n + 1,) and pm.shape == (0,) and not bool(rp.any())
    t = ops.Topology(torch.zeros(2, 0, dtype=torch.int64, device=dev), n)
    assert t.rowptr_dst.shape == (n + 1,) and t.rowptr_src.shape == (n + 1,) and not bool(t.rowptr_dst.any()) and not bool(t.rowptr_src.any())
    assert t.perm_dst.numel() == 0 and t.perm_src.numel() == 0 and t.src_s.numel() == 0 and t.dst_s.numel() == 0
    assert (t.max_in_degree, t.max_out_degree) == (0, 0) and not t.has_hubs
    if n:     # a segment sum over it writes zeros into every row
        out = _nan_out(n, 16, dev)
        ops.segsum_topo(torch.zeros(PAD, 16, device=dev)[:0], t, "dst", out)
        assert _same(out, np.zeros((n, 16), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ mgn_segsum
LADDER_NS = [None, 1, 8, 13]


@pytest.mark.parametrize("n", LADDER_NS)
@pytest.mark.parametrize("H", AC.HS)
def test_segsum_ladder(dev, H, n):
    """rows in segment order (perm = None) and the gathered form: the sequential fp32 sum, bit for bit; every row of a
    preallocated NaN-filled ``out`` is written, the empty segments with +0"""
    c = AC.degree_ladder(H, n)
    R = c.src.shape[0]
    src = _rows(c.src, dev)
    want, want2 = _ladder_refs(H, n)
    out = _nan_out(c.n, H, dev)
    assert ops.segsum(src, _i32(c.rowptr, dev), None, out) is out
    assert _same(out, want), (c.name, "in order")
    assert _inside_gamma(out, c.src, c.rowptr, None)
    out2 = _nan_out(c.n, H, dev)
    ops.segsum(src, _i32(c.rowptr2, dev), _perm(c.perm2, R, dev), out2)
    assert _same(out2, want2), (c.name, "gathered")
    assert _inside_gamma(out2, c.src, c.rowptr2, c.perm2)
    fresh = ops.segsum(src, _i32(c.rowptr, dev), None)      # an output of the engine's own
    assert fresh.shape == (c.n, H) and _same(fresh, want)
    empty = np.flatnonzero(np.diff(c.rowptr) == 0)
    assert not bool(torch.signbit(out[torch.from_numpy(empty).to(dev)]).any())


def test_segsum_refuses_other_widths(dev):
    rp = _i32([0, 1, 2], dev)
    with pytest.raises(RuntimeError, match="H must be 16, 32, 64 or 128"):
        ops.segsum(torch.zeros(2, 48, device=dev), rp, None)
    wide = torch.zeros(2, 32, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        ops.segsum(wide[:, :16], rp, None)
    with pytest.raises(ValueError, match="contiguous"):
        ops.segsum2(torch.zeros(2, 256, device=dev)[:, :128], rp, None, _nan_out(2, 128, dev), rp, None, _nan_out(2, 128, dev))


# --------------------------------------------------------------------------------- mgn_segsum2, mgn_segsum2_b16
def _two_jobs(c, dev):
    R = c.src.shape[0]
    return (_i32(c.rowptr, dev), None), (_i32(c.rowptr2, dev), _perm(c.perm2, R, dev))


@pytest.mark.parametrize("swap", [False, True], ids=["in_order_first", "gathered_first"])
@pytest.mark.parametrize("n", LADDER_NS)
def test_segsum2_is_two_segsums(dev, n, swap):
    """both jobs of the launch, at node counts that fill less than one workgroup (1), exactly one (8), one and a part (13) and
    several with a ragged last one; the CSRs swapped between the jobs"""
    c = AC.degree_ladder(128, n)
    src = _rows(c.src, dev)
    jobs, wants = _two_jobs(c, dev), _ladder_refs(128, n)
    if swap:
        jobs, wants = jobs[::-1], wants[::-1]
    out0, out1 = _nan_out(c.n, 128, dev), _nan_out(c.n, 128, dev)
    ops.segsum2(src, jobs[0][0], jobs[0][1], out0, jobs[1][0], jobs[1][1], out1)
    assert _same(out0, wants[0]) and _same(out1, wants[1]), c.name
    assert torch.equal(out0, ops.segsum(src, *jobs[0])) and torch.equal(out1, ops.segsum(src, *jobs[1]))


def test_segsum2_refuses_other_widths(dev):
    c = AC.degree_ladder(64, 8)
    (rp, _), (rp2, pm2) = _two_jobs(c, dev)
    for src in (_rows(c.src, dev), _rows(c.src, dev).to(torch.bfloat16)):
        with pytest.raises(RuntimeError, match="H must be 128"):
            ops.segsum2(src, rp, None, _nan_out(c.n, 64, dev), rp2, pm2, _nan_out(c.n, 64, dev))


@pytest.mark.parametrize("swap", [False, True], ids=["in_order_first", "gathered_first"])
@pytest.mark.parametrize("n", LADDER_NS)
def test_segsum2_b16_unpacks_the_packed_order(dev, n, swap):
    """two-byte rows in the packed feature order of include/mgn_hip.h: the sums come out in the true feature order and equal the
    sequential fp32 sums of the unpacked rows exactly (a bf16 value widens to fp32 without rounding)"""
    c = AC.degree_ladder(128, n)
    R = c.src.shape[0]
    packed = AC.pack_b16(AC.bf16_round(c.src))
    rows = AC.unpack_b16(packed)
    buf = np.full((R + PAD, 128), 0x7FC0, dtype=np.uint16)      # (bf16 NaN behind the rows)
    buf[:R] = packed
    src = torch.from_numpy(buf.view(np.int16)).to(dev).view(torch.bfloat16)[:R]
    jobs, wants = _two_jobs(c, dev), (AC.seq32(rows, c.rowptr), AC.seq32(rows, c.rowptr2, c.perm2))
    if swap:
        jobs, wants = jobs[::-1], wants[::-1]
    out0, out1 = _nan_out(c.n, 128, dev), _nan_out(c.n, 128, dev)
    ops.segsum2(src, jobs[0][0], jobs[0][1], out0, jobs[1][0], jobs[1][1], out1)
    assert _same(out0, wants[0]) and _same(out1, wants[1]), c.name


# ----------------------------------------------------------------------------------------------- hub path
@pytest.mark.parametrize("H", [16, 128])
@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_hub_chunking_at_the_boundary_degrees(dev, d, H):
    """in- and out-hub of degree d: no tables up to HUB_CHUNK, tables from HUB_CHUNK + 1, and segsum_topo equal to the
    two-level reference bit for bit (which differs from the one-level sum from degree 2048 on); n_rows below N leaves the
    rows behind it alone"""
    c = AC.hub(d)
    topo = ops.Topology(torch.from_numpy(c.edge_index).to(dev), c.n)
    t = AC.topology_reference(c.edge_index[0], c.edge_index[1], c.n)
    assert (topo.max_in_degree, topo.max_out_degree) == (d, d)
    for tab, rp in ((topo.hub_dst, t["rowptr_dst"]), (topo.hub_src, t["rowptr_src"])):
        assert (tab is None) == (d <= AC.CHUNK), d
        if tab is not None:
            crp, ncp = AC.chunk_tables(rp)
            assert torch.equal(tab[0].cpu().long(), torch.from_numpy(crp)) and torch.equal(tab[1].cpu().long(), torch.from_numpy(ncp))
    ms = AC.hub_rows(d, H)[t["perm_dst"].long().numpy()]      # the edge rows in dst-sorted order, as the engine holds them
    src = _rows(ms, dev)
    n_rows = 30
    assert max(c.hub_in, c.hub_out) < n_rows < c.n
    for by, rp, pm in (("dst", t["rowptr_dst"], None), ("src", t["rowptr_src"], t["perm_src"])):
        want = AC.two_level(ms, rp, pm)
        out = _nan_out(c.n, H, dev)
        assert ops.segsum_topo(src, topo, by, out) is out
        assert _same(out, want), (d, H, by)
        part = _nan_out(c.n, H, dev)
        ops.segsum_topo(src, topo, by, part, n_rows)
        assert _same(part[:n_rows], want[:n_rows]) and bool(torch.isnan(part[n_rows:]).all()), (d, H, by, "n_rows")


# ------------------------------------------------------------------------------------ mgn_transpose_blocks
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [1, 3, 128, 129, 300])
@pytest.mark.parametrize("H", [1, 16, 24, 32, 48, 64, 80, 100, 127, 128])
def test_transpose_blocks(dev, H, n):
    """n blocks, column slabs of a wide source (pitch n H + 3) into slabs of a NaN-filled destination that are two columns apart
    and one row short of its height: every H x H block is the transpose, every other element is still the NaN it was"""
    ld_s, gap = n * H + 3, H + 2
    ld_d = n * gap + 1
    S = torch.arange(H * ld_s, dtype=torch.float32).view(H, ld_s)      # distinct values, exact in fp32 (below 2^24)
    assert H * ld_s < 2 ** 24
    want = torch.full((H + 1, ld_d), NAN)
    for i in range(n):
        want[:H, i * gap:i * gap + H] = S[:, i * H:(i + 1) * H].t()
    Sd, D = S.to(dev), torch.full((H + 1, ld_d), NAN, device=dev)
    ops.transpose_blocks([(Sd.data_ptr() + 4 * i * H, ld_s, D.data_ptr() + 4 * i * gap, ld_d) for i in range(n)], H, dev)
    assert torch.equal(_bits(D.cpu()), _bits(want)), (H, n)


def test_transpose_blocks_refusals_and_no_blocks(dev):
    S, D = torch.zeros(128, 128, device=dev), torch.full((128, 128), NAN, device=dev)
    blk = [(S.data_ptr(), 128, D.data_ptr(), 128)]
    for H in (0, 129, -1):
        with pytest.raises(RuntimeError, match="bad arguments"):
            ops.transpose_blocks(blk, H, dev)
    ops.transpose_blocks([], 32, dev)
    assert call("mgn_transpose_blocks", dev, 0, (_capi.TBlock * 1)(), 32) == 0      # n = 0 through the C entry point: no launch
    assert bool(torch.isnan(D).all())


def test_report_wall_time():
    """the figure of this file (pytest -s); last in file order"""
    print(f"wall time of this file so far: {time.time() - _t0[0]:.1f} s")
