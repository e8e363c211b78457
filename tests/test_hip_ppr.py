"""GPU: the register-resident-weights generation of the edge update (csrc/mgn_ppr.inc; MGN_PPR: default = launches from 65 536 rows, both modes) through the C ABI (mgn_mlp_fwd):
every output of the launch -- e', the fused aggregation, the saved activations with their sign bits, U, rms -- against an fp64
evaluation of the reference's edge update (layers.py:1044-1060, 163-210, 104-129) on ragged row counts (tile tails, one row,
rows past the last tile) in inference and training mode, and against the x6 static-shape kernel it replaces: saved activations and sign bits BIT-identical (same MFMA terms in the same
order on the same packed weights), u / e' / aggregate to rounding (the row norm adds its squares in another order).
Also: the interior + boundary launch pair of a partitioned rank (ops.edge_rows) for the ppr, pp and x6 kernels, the backward chain on a
row range, and gather sources past 2^23 rows (where the ppr kernels' 32-bit byte offsets would wrap: the dispatcher must refuse them)."""
import os

import pytest
import torch

import graph_physics_amd as gp
from graph_physics_amd import _capi, ops

pytestmark = pytest.mark.gpu
H = 128


@pytest.fixture(scope="module")
def case():
    dev = torch.device("cuda:0")
    g = gp.cylinder_batch(6, 1885, 0).to(dev)
    topo = ops.Topology(g.edge_index, g.x.shape[0])
    f = dict(dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, **f)  # noqa: E731
    x, e = rn(topo.N, H), rn(topo.E, H)
    W0 = rn(H, 3 * H) * 0.05
    Wh = [rn(H, H) * 0.09 for _ in range(3)]
    bs = [rn(H) * 0.1 for _ in range(4)]
    sc = torch.rand(H, generator=gen, **f) + 0.5
    Pd, Ps = x @ W0[:, H:2 * H].t(), x @ W0[:, 2 * H:].t()
    pk = torch.empty(4 * _capi.WPACK_BYTES, dtype=torch.uint8, device=dev)
    units = [pk.data_ptr() + u * _capi.WPACK_BYTES for u in range(4)]
    ops.wpack([(W0.data_ptr(), 3 * H, False, units[0])] + [(Wh[l].data_ptr(), H, False, units[l + 1]) for l in range(3)], dev)
    d = torch.float64
    z = e.to(d) @ W0[:, :H].to(d).t() + Pd.to(d)[topo.dst_s.long()] + Ps.to(d)[topo.src_s.long()] + bs[0].to(d)
    hs = []
    for l in range(3):
        h = z.clamp_min(0)
        hs.append(h)
        z = h @ Wh[l].to(d).t() + bs[l + 1].to(d)
    rms = z.norm(dim=1, keepdim=True) / H ** 0.5
    u = z / (rms + 1e-8)
    m = sc.to(d) * u
    return dict(dev=dev, topo=topo, e=e, W0=W0, Wh=Wh, bs=bs, sc=sc, Pd=Pd, Ps=Ps, units=units, pk=pk,
                ref=dict(e_new=e.to(d) + m, m=m, H=hs, U=u, R=rms[:, 0]))


def _run(c, M, save, pp):
    dev, topo = c["dev"], c["topo"]
    f = dict(dtype=torch.float32, device=dev)
    old = os.environ.get("MGN_PP"), os.environ.get("MGN_PPR")
    os.environ["MGN_PP"] = "0"
    os.environ["MGN_PPR"] = "2" if pp else "0"
    try:
        sl = slice(0, M)
        nn = int(topo.dst_s[M - 1]) + 1
        dst = topo.dst_s[sl].contiguous()
        rowptr = torch.searchsorted(dst, torch.arange(nn + 1, device=dev, dtype=torch.int32)).to(torch.int32)
        e_new = torch.full((M, H), float("nan"), **f)
        agg = torch.full((nn, H), float("nan"), **f)
        part = torch.full(((M + 15) // 16, 2, H), float("nan"), **f)
        He = [torch.full((M, H), float("nan"), **f) for _ in range(3)] if save else None
        Ue, Re = (torch.full((M, H), float("nan"), **f), torch.full((M,), float("nan"), **f)) if save else (None, None)
        Me = [torch.zeros(M, 4, dtype=torch.int32, device=dev) for _ in range(3)] if save else None
        ops.mlp_fwd(M, H, [(c["e"][sl], None, H)], [c["W0"]] + c["Wh"], c["bs"], c["sc"], H, c["e"][sl], e_new, None, He, Ue, Re, ldw0=3 * H,
                    adds=[(c["Pd"], dst), (c["Ps"], topo.src_s[sl].contiguous())], wpk=c["units"], saveM=Me, seg=(dst, rowptr, agg, part))
        ops.seg_fix(rowptr, part, agg)
        torch.cuda.synchronize()
    finally:
        for k, v in zip(("MGN_PP", "MGN_PPR"), old):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return dict(e_new=e_new, agg=agg, H=He, U=Ue, R=Re, M=Me)


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("M", [0, -10, -23, 40000, 8193, 257, 129, 128, 33, 32, 31, 17, 16, 1])
def test_ppr_edge_update_vs_fp64_and_x6(case, M, save):
    """M <= 0: all rows of the 6-mesh batch (E ~ 67 500: several tiles per workgroup), minus |M|"""
    topo, ref = case["topo"], case["ref"]
    M = topo.E + M if M <= 0 else M
    got = _run(case, M, save, True)
    base = _run(case, M, save, False)
    nn = int(topo.dst_s[M - 1]) + 1
    agg_ref = torch.zeros(nn, H, dtype=torch.float64, device=case["dev"]).index_add_(0, topo.dst_s[:M].long(), ref["m"][:M])
    tol = 2e-6
    assert _rel(got["e_new"], ref["e_new"][:M]) < tol and not bool(torch.isnan(got["e_new"]).any())
    assert _rel(got["agg"], agg_ref) < tol and not bool(torch.isnan(got["agg"]).any())
    assert _rel(got["e_new"], base["e_new"].double()) < tol and _rel(got["agg"], base["agg"].double()) < tol   # the kernel it replaces
    if save:
        for l in range(3):
            assert _rel(got["H"][l], ref["H"][l][:M]) < tol
            bits = (got["H"][l].view(M, 8, 4, 4) > 0).permute(0, 2, 1, 3).reshape(M, 4, 32).long()   # [row][g][4 ib + r]
            want = (bits << torch.arange(32, device=case["dev"])).sum(-1)
            assert torch.equal(got["M"][l].long() & 0xffffffff, want), f"sign bits of layer {l + 1}"
            assert torch.equal(got["H"][l], base["H"][l]) and torch.equal(got["M"][l], base["M"][l]), f"layer {l + 1} differs from the x6 kernel"
        assert _rel(got["U"], ref["U"][:M]) < tol and _rel(got["R"], ref["R"][:M]) < tol


# ------------------------------------------------------------------ the backward chain (k_edge_bwd_ppr)
@pytest.fixture(scope="module")
def bcase(case):
    """forward saves of the whole batch (x6 kernel) + an fp64 backward FROM THOSE saves (both kernels read the same mask bits)"""
    c = case
    dev, topo = c["dev"], c["topo"]
    f = dict(dtype=torch.float32, device=dev)
    E = topo.E
    fwd = _run(c, E, True, False)
    gen = torch.Generator(device=dev).manual_seed(7)
    dOut = torch.randn(E, H, generator=gen, **f)
    dAgg = torch.randn(topo.N, H, generator=gen, **f)
    pk = torch.empty(4 * _capi.WPACK_BYTES, dtype=torch.uint8, device=dev)
    bu = [pk.data_ptr() + u * _capi.WPACK_BYTES for u in range(4)]
    Wh, W0 = c["Wh"], c["W0"]
    ops.wpack([(Wh[2].data_ptr(), H, True, bu[0]), (Wh[1].data_ptr(), H, True, bu[1]), (Wh[0].data_ptr(), H, True, bu[2]), (W0.data_ptr(), 3 * H, True, bu[3])], dev)
    d = torch.float64
    dY = dOut.to(d) + dAgg.to(d)[topo.dst_s.long()]
    U64, R64 = fwd["U"].to(d), fwd["R"].to(d)
    gg = c["sc"].to(d) * dY
    dz3 = gg / (R64[:, None] + 1e-8) - U64 * ((gg * U64).sum(1, keepdim=True) / (H * R64[:, None]))
    dz2 = (dz3 @ Wh[2].to(d)) * (fwd["H"][2] > 0)
    dz1 = (dz2 @ Wh[1].to(d)) * (fwd["H"][1] > 0)
    dz0 = (dz1 @ Wh[0].to(d)) * (fwd["H"][0] > 0)
    dE = dOut.to(d) + dz0 @ W0[:, :H].to(d)
    return dict(fwd=fwd, dOut=dOut, dAgg=dAgg, bu=bu, pk=pk, ref=dict(dZ=[dz0, dz1, dz2, dz3], dE=dE, dYU=dY * U64))


def _run_bwd(c, b, M, ppr, r0=0):
    """the chain on rows [r0, M) (every row pointer offset by r0 rows; dAgg / idx2 keep the global node numbering)"""
    dev, topo = c["dev"], c["topo"]
    f = dict(dtype=torch.float32, device=dev)
    old = os.environ.get("MGN_PPR")
    os.environ["MGN_PPR"] = "2" if ppr else "0"
    try:
        sl = slice(r0, M)
        n = M - r0
        dZ = [torch.full((n, H), float("nan"), **f) for _ in range(4)]
        dE = torch.full((n, H), float("nan"), **f)
        dsc = torch.full((H,), float("nan"), **f)
        fw = b["fwd"]
        ops.mlp_bwd(n, H, 4, b["dOut"][sl], b["dAgg"], topo.dst_s[sl].contiguous(), H, fw["U"][sl], fw["R"][sl], c["sc"], [t[sl] for t in fw["H"]],
                    [None] * 4, dZ, [(None, b["dOut"][sl], dE)], [None] * 4, dsc, wpk=b["bu"], Ms=[t[sl] for t in fw["M"]])
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("MGN_PPR", None)
        else:
            os.environ["MGN_PPR"] = old
    return dict(dZ=dZ, dE=dE, dscale=dsc)


@pytest.mark.parametrize("M", [0, -10, -23, 40000, 8193, 257, 129, 128, 33, 32, 31, 17, 16, 1])
def test_ppr_edge_backward_chain_vs_fp64_and_x6(case, bcase, M):
    """every output of the launch -- dZ[3..0], dE, dscale -- against the fp64 backward of the reference's edge update (RMSNorm
    layers.py:104-129, build_mlp :163-210, edge_update :1044-1060) and against the x6 static-shape chain it replaces"""
    topo, ref = case["topo"], bcase["ref"]
    M = topo.E + M if M <= 0 else M
    got = _run_bwd(case, bcase, M, True)
    base = _run_bwd(case, bcase, M, False)
    tol = 2e-6
    for l in range(4):
        assert _rel(got["dZ"][l], ref["dZ"][l][:M]) < tol and not bool(torch.isnan(got["dZ"][l]).any()), f"dZ[{l}]"
        assert _rel(got["dZ"][l], base["dZ"][l].double()) < tol
    assert _rel(got["dE"], ref["dE"][:M]) < tol and not bool(torch.isnan(got["dE"]).any())
    assert _rel(got["dscale"], ref["dYU"][:M].sum(0)) < tol and _rel(got["dscale"], base["dscale"].double()) < 2 * tol


# ------------------------------------------------------------------ the halo split: two launches over row ranges (ops.edge_rows)
KERNELS = {"ppr": {"MGN_PPR": "2", "MGN_PP": "0"}, "pp": {"MGN_PPR": "0", "MGN_PP": "2"}, "x6": {"MGN_PPR": "0", "MGN_PP": "0"}}
SENT = -7777.0         # what the rows of the OTHER launch hold until that launch runs
SENT_M = 0x13579BDF    # likewise for the mask words
N_EMPTY = 3            # trailing nodes without an incoming edge (seg_fix zeroes their aggregate)


class _env:
    """set (value) / unset (None) environment variables for a block, restored afterwards"""

    def __init__(self, kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _split_points(topo):
    """name -> (M, ni): the edge prefix [0, M) of the batch and the node split; the interior launch covers rows [0, rowptr[ni])"""
    rp = topo.rowptr_dst.long().cpu()
    E, N = topo.E, topo.N
    pts = {}
    for r in (0, 1, 3, 4, 8, 15):    # Ei mod 16: every row-indexed pointer of the boundary launch is offset by that many rows
        pts[f"Ei%16={r}"] = (E, next(k for k in range(N // 2, N) if int(rp[k]) % 16 == r))
    k = N - 40                       # a 1-row boundary launch: the prefix ends one row into node k's segment
    pts["bnd=1"] = (int(rp[k]) + 1, k)
    pts["bnd<16"] = (E, next(k for k in range(N - 1, 0, -1) if 4 < E - int(rp[k]) < 16))
    pts["Ei=0"] = (E, 0)             # no interior rows: the interior launch is skipped
    return pts


def _ghosted(c, M, Ei, seed=3):
    """Ps with ghost rows: exact copies of the Ps rows about a third of the boundary rows read, appended past N; those rows' src
    re-pointed at the copies (what a rank's receive buffer holds).  The results must not change."""
    topo, dev = c["topo"], c["dev"]
    src = topo.src_s[:M].clone()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    pick = Ei + torch.nonzero(torch.rand(M - Ei, generator=gen) < 1 / 3)[:, 0].to(dev)
    if pick.numel() == 0:
        pick = torch.tensor([Ei], device=dev)
    uniq = torch.unique(src[pick].long())
    Ps = torch.cat([c["Ps"], c["Ps"][uniq]])
    src[pick] = (topo.N + torch.searchsorted(uniq, src[pick].long())).to(torch.int32)
    return Ps, src, int(pick.numel())


def _run_split(c, M, ni, save, kern):
    """ops.edge_rows as a partitioned rank runs it: rows [0, Ei) with the node CSR, then rows [Ei, M) with the CSR shifted by Ei
    (HaloState.rowptr_bnd), each launch finished by seg_fix on its own node range; every output checked for rows the launch must
    not touch (they hold a sentinel until their own launch)"""
    dev, topo = c["dev"], c["topo"]
    f = dict(dtype=torch.float32, device=dev)
    dst = topo.dst_s[:M].contiguous()
    nn = int(dst[M - 1]) + 1 + N_EMPTY
    rowptr = torch.searchsorted(dst, torch.arange(nn + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    Ei = int(rowptr[ni])
    Ps, src, n_ghost = _ghosted(c, M, Ei)
    rowptr_bnd = (rowptr - Ei).contiguous()
    lo, hi, nlo, nhi = slice(0, Ei), slice(Ei, M), slice(0, ni), slice(ni, nn)

    def fill(shape, dt=torch.float32):
        """NaN (zero mask words) on the interior rows, the sentinel on the boundary rows"""
        t = torch.full(shape, float("nan"), dtype=dt, device=dev) if dt == torch.float32 else torch.zeros(shape, dtype=dt, device=dev)
        t[Ei:M] = SENT if dt == torch.float32 else SENT_M
        return t

    e_new = fill((M, H))
    agg = torch.full((nn, H), float("nan"), **f)
    agg[nhi] = SENT
    He = [fill((M, H)) for _ in range(3)] if save else None
    Ue, Re = (fill((M, H)), fill((M,))) if save else (None, None)
    Me = [fill((M, 4), torch.int32) for _ in range(3)] if save else None
    outs = lambda: [e_new] + ((He + [Ue, Re] + Me) if save else [])  # noqa: E731

    def launch(sl, rp, nodes):
        n = sl.stop - sl.start
        part = torch.full(((n + 15) // 16, 2, H), float("nan"), **f)
        sv = lambda ts: [t[sl] for t in ts] if ts is not None else None  # noqa: E731
        ops.mlp_fwd(n, H, [(c["e"][sl], None, H)], [c["W0"]] + c["Wh"], c["bs"], c["sc"], H, c["e"][sl], e_new[sl], None, sv(He),
                    Ue[sl] if save else None, Re[sl] if save else None, ldw0=3 * H,
                    adds=[(c["Pd"], dst[sl]), (Ps, src[sl])], wpk=c["units"], saveM=sv(Me), seg=(dst[sl], rp, agg, part))
        ops.seg_fix(rp[nodes.start:nodes.stop + 1], part, agg[nodes])
        torch.cuda.synchronize()

    with _env(KERNELS[kern]):
        if Ei > 0:
            launch(lo, rowptr, nlo)
            for t in outs():
                want = SENT_M if t.dtype == torch.int32 else SENT
                assert bool((t[hi] == want).all()), f"{kern}: the interior launch wrote a boundary row"
            assert bool((agg[nhi] == SENT).all()), f"{kern}: the interior launch wrote the aggregate of a boundary node"
        first = [t[lo].clone() for t in outs()] + [agg[nlo].clone()]
        launch(hi, rowptr_bnd, nhi)
        for a, b in zip([t[lo] for t in outs()] + [agg[nlo]], first):
            assert torch.equal(a, b), f"{kern}: the boundary launch wrote an interior row / node"
    return dict(e_new=e_new, agg=agg, H=He, U=Ue, R=Re, M=Me, Ei=Ei, nn=nn, n_ghost=n_ghost)


def _mask_words(Hl):
    M = Hl.shape[0]
    bits = (Hl.view(M, 8, 4, 4) > 0).permute(0, 2, 1, 3).reshape(M, 4, 32).long()   # [row][g][4 ib + r]
    return (bits << torch.arange(32, device=Hl.device)).sum(-1)


@pytest.mark.parametrize("kern", ["ppr", "pp", "x6"])
@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("split", ["Ei%16=0", "Ei%16=1", "Ei%16=3", "Ei%16=4", "Ei%16=8", "Ei%16=15", "bnd=1", "bnd<16", "Ei=0"])
def test_edge_update_halo_split_vs_fp64(case, split, save, kern):
    """The edge update as ops.edge_rows runs it on a partitioned rank (interior rows, then boundary rows with every row-indexed
    pointer offset by Ei, destinations from n_interior on, the shifted rowptr, seg_fix on the boundary node range, ghost copies
    of Ps rows past N): e', the aggregate of every node (trailing nodes without edges included), the saves and U / R against
    the un-split fp64 evaluation; the ppr saves and sign bits bit-identical to the x6 kernel on the same split; no launch writes
    a row of the other"""
    topo, ref = case["topo"], case["ref"]
    M, ni = _split_points(topo)[split]
    got = _run_split(case, M, ni, save, kern)
    Ei, nn = got["Ei"], got["nn"]
    assert got["n_ghost"] > 0
    if split == "bnd=1":
        assert M - Ei == 1
    elif split == "bnd<16":
        assert 1 < M - Ei < 16
    elif split == "Ei=0":
        assert Ei == 0
    else:
        assert Ei % 16 == int(split.split("=")[1]) and 0 < Ei < M
    agg_ref = torch.zeros(nn, H, dtype=torch.float64, device=case["dev"]).index_add_(0, topo.dst_s[:M].long(), ref["m"][:M])
    tol = 2e-6
    assert not bool(torch.isnan(got["e_new"]).any()) and not bool(torch.isnan(got["agg"]).any())
    assert _rel(got["e_new"], ref["e_new"][:M]) < tol, "e'"
    assert _rel(got["agg"], agg_ref) < tol, "aggregate"
    assert bool((got["agg"][nn - N_EMPTY:] == 0).all()), "nodes without an incoming edge"
    if save:
        for l in range(3):
            assert not bool(torch.isnan(got["H"][l]).any())
            assert _rel(got["H"][l], ref["H"][l][:M]) < tol, f"H{l + 1}"
            assert torch.equal(got["M"][l].long() & 0xffffffff, _mask_words(got["H"][l])), f"sign bits of layer {l + 1}"
        assert not bool(torch.isnan(got["U"]).any()) and not bool(torch.isnan(got["R"]).any())
        assert _rel(got["U"], ref["U"][:M]) < tol and _rel(got["R"], ref["R"][:M]) < tol
        if kern == "ppr":
            base = _run_split(case, M, ni, save, "x6")
            for l in range(3):
                assert torch.equal(got["H"][l], base["H"][l]) and torch.equal(got["M"][l], base["M"][l]), f"layer {l + 1} differs from x6"


@pytest.mark.parametrize("r0", [1, 4])
def test_ppr_edge_backward_chain_on_row_range(case, bcase, r0):
    """the backward chain on rows [r, E) with r mod 16 = r0 (every row pointer offset by a non-multiple of the 16-row tile),
    dAgg / idx2 in the global node numbering: ppr against fp64 and the x6 chain"""
    topo, ref = case["topo"], bcase["ref"]
    r = next(k for k in range(topo.E // 3, topo.E) if k % 16 == r0)
    got = _run_bwd(case, bcase, topo.E, True, r)
    base = _run_bwd(case, bcase, topo.E, False, r)
    tol = 2e-6
    for l in range(4):
        assert not bool(torch.isnan(got["dZ"][l]).any()), f"dZ[{l}]"
        assert _rel(got["dZ"][l], ref["dZ"][l][r:]) < tol, f"dZ[{l}]"
        assert _rel(got["dZ"][l], base["dZ"][l].double()) < tol
    assert not bool(torch.isnan(got["dE"]).any()) and _rel(got["dE"], ref["dE"][r:]) < tol
    assert _rel(got["dscale"], ref["dYU"][r:].sum(0)) < tol and _rel(got["dscale"], base["dscale"].double()) < 2 * tol


# ------------------------------------------------------------------ gather sources past 2^23 rows
BIG = (1 << 23) + 4096   # rows of Pd / Ps / dAgg: a 512-byte row at index >= 2^23 lies past 2^32 bytes


@pytest.fixture(scope="module")
def big(case):
    """Pd, Ps, dAgg of BIG rows (4.3 GB each), ~70 000 dst-sorted edge rows whose gathered indices lie mostly in
    [2^23 - 2048, 2^23 + 4096) -- with some far below 2^23, so that a row offset wrapped at 32 bits reads real, different data"""
    dev = case["dev"]
    f = dict(dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    M = 70001
    near = torch.randint((1 << 23) - 2048, BIG, (M,), generator=gen, device=dev)
    far = torch.randint(0, 1 << 23, (M,), generator=gen, device=dev)
    pick_far = lambda: torch.rand(M, generator=gen, device=dev) < 0.1  # noqa: E731
    dst = torch.where(pick_far(), far, near).sort().values.to(torch.int32)
    src = torch.where(pick_far(), far.flip(0), near.flip(0)).to(torch.int32)
    assert int(dst.max()) >= 1 << 23 and int(src.max()) >= 1 << 23 and int(dst.min()) < (1 << 23) - 2048
    Pd, Ps, dAgg = (torch.randn(BIG, H, generator=gen, **f) for _ in range(3))
    e, dOut = torch.randn(M, H, generator=gen, **f), torch.randn(M, H, generator=gen, **f)
    return dict(M=M, dst=dst, src=src, Pd=Pd, Ps=Ps, dAgg=dAgg, e=e, dOut=dOut)


def _fwd64(c, b, rows_d, rows_s):
    d = torch.float64
    z = b["e"].to(d) @ c["W0"][:, :H].to(d).t() + rows_d.to(d) + rows_s.to(d) + c["bs"][0].to(d)
    hs = []
    for l in range(3):
        h = z.clamp_min(0)
        hs.append(h)
        z = h @ c["Wh"][l].to(d).t() + c["bs"][l + 1].to(d)
    rms = z.norm(dim=1, keepdim=True) / H ** 0.5
    u = z / (rms + 1e-8)
    m = c["sc"].to(d) * u
    return dict(e_new=b["e"].to(d) + m, m=m, H=hs, U=u, R=rms[:, 0])


@pytest.mark.parametrize("kern", ["default", "pp", "x6"])
def test_edge_update_gathers_past_2pow23_rows(case, big, kern):
    """Forward (inference and training) and backward chain with gather sources of 2^23 + 4096 rows, against fp64 computed on the
    gathered rows.  "default": the dispatcher's own choice at 70 000 rows (the ppr kernels, unless the source row counts rule them
    out: their gathers use 32-bit byte offsets, row * 512, which wrap past row 2^23 -- silently, inside the same buffer)."""
    c, b = case, big
    dev, M, dst, src = c["dev"], big["M"], big["dst"], big["src"]
    f = dict(dtype=torch.float32, device=dev)
    env = {"MGN_PPR": None, "MGN_PP": None} if kern == "default" else KERNELS[kern]
    ref = _fwd64(c, b, b["Pd"][dst.long()], b["Ps"][src.long()])
    uniq, inv = torch.unique(dst.long(), return_inverse=True)
    agg_ref = torch.zeros(uniq.numel(), H, dtype=torch.float64, device=dev).index_add_(0, inv, ref["m"])
    rowptr = torch.searchsorted(dst, torch.arange(BIG + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    tol = 2e-6
    saves = {}
    for save in (False, True):
        e_new = torch.full((M, H), float("nan"), **f)
        agg = torch.full((BIG, H), float("nan"), **f)
        part = torch.full(((M + 15) // 16, 2, H), float("nan"), **f)
        He = [torch.full((M, H), float("nan"), **f) for _ in range(3)] if save else None
        Ue, Re = (torch.full((M, H), float("nan"), **f), torch.full((M,), float("nan"), **f)) if save else (None, None)
        Me = [torch.zeros(M, 4, dtype=torch.int32, device=dev) for _ in range(3)] if save else None
        with _env(env):
            ops.mlp_fwd(M, H, [(b["e"], None, H)], [c["W0"]] + c["Wh"], c["bs"], c["sc"], H, b["e"], e_new, None, He, Ue, Re, ldw0=3 * H,
                        adds=[(b["Pd"], dst), (b["Ps"], src)], wpk=c["units"], saveM=Me, seg=(dst, rowptr, agg, part))
            ops.seg_fix(rowptr, part, agg)
            torch.cuda.synchronize()
        mode = "training" if save else "inference"
        assert not bool(torch.isnan(e_new).any()), mode
        assert _rel(e_new, ref["e_new"]) < tol, f"{mode}: e'"
        assert _rel(agg[uniq], agg_ref) < tol, f"{mode}: aggregate"
        touched = torch.zeros(BIG, dtype=torch.bool, device=dev)
        touched[uniq] = True
        assert float(agg.abs().amax(1)[~touched].max()) == 0.0, f"{mode}: aggregate of nodes without an edge"
        del agg
        if save:
            for l in range(3):
                assert _rel(He[l], ref["H"][l]) < tol, f"H{l + 1}"
                assert torch.equal(Me[l].long() & 0xffffffff, _mask_words(He[l])), f"sign bits of layer {l + 1}"
            assert _rel(Ue, ref["U"]) < tol and _rel(Re, ref["R"]) < tol
            saves = dict(H=He, U=Ue, R=Re, M=Me)

    # backward chain from these saves: dY = dOut + dAgg[dst] (the gather under test), fp64 from the same saves
    d = torch.float64
    dY = b["dOut"].to(d) + b["dAgg"][dst.long()].to(d)
    U64, R64 = saves["U"].to(d), saves["R"].to(d)
    gg = c["sc"].to(d) * dY
    dz3 = gg / (R64[:, None] + 1e-8) - U64 * ((gg * U64).sum(1, keepdim=True) / (H * R64[:, None]))
    dz2 = (dz3 @ c["Wh"][2].to(d)) * (saves["H"][2] > 0)
    dz1 = (dz2 @ c["Wh"][1].to(d)) * (saves["H"][1] > 0)
    dz0 = (dz1 @ c["Wh"][0].to(d)) * (saves["H"][0] > 0)
    dE_ref = b["dOut"].to(d) + dz0 @ c["W0"][:, :H].to(d)
    pk = torch.empty(4 * _capi.WPACK_BYTES, dtype=torch.uint8, device=dev)
    bu = [pk.data_ptr() + u * _capi.WPACK_BYTES for u in range(4)]
    Wh, W0 = c["Wh"], c["W0"]
    ops.wpack([(Wh[2].data_ptr(), H, True, bu[0]), (Wh[1].data_ptr(), H, True, bu[1]), (Wh[0].data_ptr(), H, True, bu[2]), (W0.data_ptr(), 3 * H, True, bu[3])], dev)
    dZ = [torch.full((M, H), float("nan"), **f) for _ in range(4)]
    dE = torch.full((M, H), float("nan"), **f)
    dsc = torch.full((H,), float("nan"), **f)
    with _env(env):
        ops.mlp_bwd(M, H, 4, b["dOut"], b["dAgg"], dst, H, saves["U"], saves["R"], c["sc"], saves["H"], [None] * 4, dZ,
                    [(None, b["dOut"], dE)], [None] * 4, dsc, wpk=bu, Ms=saves["M"])
        torch.cuda.synchronize()
    for l, want in enumerate([dz0, dz1, dz2, dz3]):
        assert not bool(torch.isnan(dZ[l]).any()) and _rel(dZ[l], want) < tol, f"backward: dZ[{l}]"
    assert not bool(torch.isnan(dE).any()) and _rel(dE, dE_ref) < tol, "backward: dE"
    assert _rel(dsc, (dY * U64).sum(0)) < tol, "backward: dscale"
