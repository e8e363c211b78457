"""GPU: masked-mesh training on the engine's kernels -- the two-source row merge ``reconstruct_graph`` launches
(``mgn_gather_rows_batch``, csrc/mgn_subgraph.hip), ``filter_edges`` / ``build_masked_graph`` against the numpy restatement of
the reference (tests/meshmask_reference.py, pinned to the reference by tests/test_meshmask_host.py), the ``exclude`` gate of the
loss kernels (csrc/mgn_loss.hip) against the fp64 reference of tests/loss_reference.py, a composed masked-pretraining step, and
the preprocessing callable.  Row copies and integer work are compared with ``torch.equal`` / ``np.array_equal``; the losses go
through ``loss_cases.check`` with its own bars."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err

import graph_physics_amd as gp
from graph_physics_amd import losses as LS, meshmask as MM, preprocess as P
import loss_cases as LC
import loss_reference as REF
import meshmask_reference as MR
import recipe as R
from meshmask_fixture import Case

pytestmark = pytest.mark.gpu
LOSS_TOL = 1e-5   # tests/test_hip_subgraph.py
GRAD_TOL = 1e-4   # tests/test_hip_losses.py


@pytest.fixture(autouse=True)
def _kernels_only(monkeypatch):
    monkeypatch.delenv("MGN_TORCH_LOSS", raising=False)


# ------------------------------------------------------------------------------- 1. the row merge of one launch
def _tile_rows(width):
    return min(max(4096 // width, 1), 1024)   # SG_GATHER_ELEMS / width, clamped to [1, SG_GATHER_ROWS]


@pytest.mark.parametrize("full_height", [False, True], ids=["one_row_source", "full_height_source"])
@pytest.mark.parametrize("width", [1, 3, 128, 4097])
def test_two_sources_merge_into_one_destination(dev, width, full_height):
    """every destination row comes from exactly one of two jobs of the SAME launch: the latent rows by an inverse index (-1 where
    masked), the others from a one-row source (a token) or a full-height one; tile = clamp(4096 // width, 1, 1024) rows"""
    tr = _tile_rows(width)
    rng = np.random.default_rng(width)
    for rows in (tr - 1, tr, tr + 1, 2 * tr + 17):
        if rows == 0:
            continue
        for pattern in ("all", "none", "first_tile", "last_tile", "mixed"):
            kept = np.zeros(rows, dtype=bool)
            if pattern == "all":
                kept[:] = True
            elif pattern == "first_tile":
                kept[:min(tr, rows)] = rng.random(min(tr, rows)) < 0.7
                kept[0] = True
            elif pattern == "last_tile":
                first = ((rows - 1) // tr) * tr
                kept[first:] = True
            elif pattern == "mixed":
                kept = rng.random(rows) < 0.5
            k = int(kept.sum())
            inv = np.full(rows, -1, dtype=np.int64)
            inv[kept] = rng.permutation(k)
            pos = np.empty(k, dtype=np.int64)
            pos[inv[kept]] = np.nonzero(kept)[0]
            a = torch.from_numpy(rng.standard_normal((k, width)).astype(np.float32)).to(dev)
            b = torch.from_numpy(rng.standard_normal((rows if full_height else 1, width)).astype(np.float32)).to(dev)
            side = MM._Side(torch.from_numpy(inv).to(dev), torch.from_numpy(pos).to(dev), full_height=full_height)
            out = torch.full((rows, width), float("nan"), device=dev)
            beside = torch.full((rows, width), 7.0, device=dev)      # a third job with one source only: its other rows stay untouched
            MM._launch_row_jobs(dev, [(a, side.inv, out), (b, side.other, out), (a, side.inv, beside)])
            keep_t = torch.from_numpy(kept).to(dev)
            want = b.expand(rows, width).clone()
            want[keep_t] = a[torch.from_numpy(inv[kept]).to(dev)]
            assert torch.equal(out, want), (width, rows, pattern)
            want_beside = torch.full((rows, width), 7.0, device=dev)
            want_beside[keep_t] = want[keep_t]
            assert torch.equal(beside, want_beside), (width, rows, pattern)


# ------------------------------------------------------------------------------- 2. reconstruct_graph
def _int_grads(shape, seed, dev):
    """integer-valued floats in [-8, 8]: every column sum over at most 4096 rows is exact in fp32 whatever the order"""
    return torch.from_numpy(np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)).to(dev)


@pytest.mark.parametrize("k_of", ["some", "none", "all"])
@pytest.mark.parametrize("with_edges", [False, True], ids=["nodes", "nodes_and_edges"])
def test_reconstruct_forward_and_gradients(dev, with_edges, k_of):
    n, E, f, fe, fin = 300, 900, 33, 20, 3
    assert n <= 4096 and E <= 4096
    rng = np.random.default_rng(5)
    k = {"some": 255, "none": 0, "all": n}[k_of]
    sel = torch.from_numpy(rng.permutation(n)[:k]).to(dev)
    ei = R.random_graph(n, E, 6).to(dev)
    full = gp.Graph(x=R.randn((n, f), 7).to(dev), edge_index=ei, edge_attr=R.randn((E, fin), 8).to(dev) if with_edges else None)
    _, _, edges_mask = gp.filter_edges(ei, sel, num_nodes=n)
    ke = int(edges_mask.sum())
    if k_of == "some":
        assert 0 < ke < E
    class Encoder(torch.nn.Module):
        """one Linear that keeps its output's gradient: what ``reconstruct_graph`` hands back to the encoder"""

        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(fin, fe)

        def forward(self, a):
            self.out = self.lin(a)
            self.out.retain_grad()
            return self.out

    enc = Encoder().to(dev)

    def inputs():
        return (R.randn((k, f), 9).to(dev).requires_grad_(True), torch.nn.Parameter(R.randn((f,), 10).to(dev)),
                R.randn((ke, fe), 11).to(dev).requires_grad_(True), torch.nn.Parameter(R.randn((fe,), 12).to(dev)))

    gx, ge = _int_grads((n, f), 13, dev), _int_grads((E, fe), 14, dev)
    # the torch formulas on the device (the reference's statements)
    lat_x, tok, lat_e, etok = inputs()
    want_x = torch.zeros(n, f, device=dev) + tok.expand(n, -1)
    want_x[sel] = lat_x
    if with_edges:
        want_e = enc(full.edge_attr) + etok.expand(E, -1)
        want_e[edges_mask] = lat_e
        ((gx * want_x).sum() + (ge * want_e).sum()).backward()
        want_enc = enc.out.grad.clone()
        assert not bool(want_enc[edges_mask].any()) and (ke == E or bool(want_enc.any()))
    else:
        (gx * want_x).sum().backward()
    want = [t.grad for t in (lat_x, tok, lat_e, etok)]

    lat_x, tok, lat_e, etok = inputs()
    rec = gp.reconstruct_graph(full, gp.Graph(x=lat_x, edge_attr=lat_e if with_edges else None), sel, tok, edges_mask,
                               edge_encoder=enc if with_edges else None, edge_mask_token=etok if with_edges else None)
    assert rec is not full and type(rec.x.grad_fn).__name__.startswith("_ReconstructFn")
    assert torch.equal(rec.x, want_x) and torch.equal(rec.edge_index, ei)
    if with_edges:
        assert torch.equal(rec.edge_attr, want_e)
        ((gx * rec.x).sum() + (ge * rec.edge_attr).sum()).backward()
        assert torch.equal(enc.out.grad, want_enc), "encoder output"
    else:
        assert rec.edge_attr is None
        (gx * rec.x).sum().backward()
    for name, got, w in zip(("latent x", "node token", "latent edge_attr", "edge token"), (lat_x.grad, tok.grad, lat_e.grad, etok.grad), want):
        if w is None:
            assert got is None, name
        else:
            assert got is not None and torch.equal(got, w), name
    if k_of != "all":
        assert bool(tok.grad.any())


def test_reconstruct_refusals(dev):
    n, f = 40, 8
    full = gp.Graph(x=torch.zeros(n, f, device=dev))
    mask = torch.zeros(0, dtype=torch.bool, device=dev)
    tok = torch.zeros(f, device=dev)
    with pytest.raises(ValueError, match="twice"):     # as mgn_subgraph_count refuses it (code 5)
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(3, f, device=dev)), torch.tensor([4, 9, 4], device=dev), tok, mask)
    with pytest.raises(IndexError):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(2, f, device=dev)), torch.tensor([4, n], device=dev), tok, mask)
    with pytest.raises(ValueError, match="widths"):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(2, f, device=dev)), torch.tensor([4, 5], device=dev), torch.zeros(f + 1, device=dev), mask)


# ------------------------------------------------------------------------------- 3. filter_edges / build_masked_graph
def _check_masked(x, pos, ei, attr, sel, dev):
    N = x.shape[0]
    want, want_mask = MR.build_masked_graph_reference(x, pos, ei, attr, sel, num_nodes=N)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    got_ei, got_attr, got_mask = gp.filter_edges(t(ei), t(sel), t(attr), num_nodes=N)
    g = got_ei.cpu().numpy()
    assert g.dtype == np.int64 and np.array_equal(g, want["edge_index"])                 # values, input order, int64
    assert got_mask.dtype == torch.bool and np.array_equal(got_mask.cpu().numpy(), want_mask)
    assert (got_attr is None) == (attr is None) and (attr is None or np.array_equal(got_attr.cpu().numpy(), want["edge_attr"]))
    graph = gp.Graph(x=t(x), y=t(x[:, :1]), pos=t(pos), edge_index=t(ei), edge_attr=t(attr))
    y = graph.y
    mg, mask = gp.build_masked_graph(graph, t(sel))
    assert mg is graph and mg.y is y and np.array_equal(mask.cpu().numpy(), want_mask)
    assert np.array_equal(mg.x.cpu().numpy(), want["x"]) and np.array_equal(mg.edge_index.cpu().numpy(), want["edge_index"])
    assert (mg.pos is None) == (pos is None) and (pos is None or np.array_equal(mg.pos.cpu().numpy(), want["pos"]))
    assert (mg.edge_attr is None) == (attr is None) and (attr is None or np.array_equal(mg.edge_attr.cpu().numpy(), want["edge_attr"]))
    return want_mask


def test_filter_and_build_on_the_messy_mesh(dev):
    c = Case("messy")
    mask = _check_masked(c.a["x"], c.a["pos"], c.edge_index, c.a["edge_attr"], c.a["selected"], dev)
    assert np.array_equal(mask, c.mask)                                                  # ... which is the reference's own
    # num_nodes=None sizes the table by the edges, as the reference does
    ei, _, m = gp.filter_edges(torch.from_numpy(c.edge_index).to(dev), torch.from_numpy(c.a["selected"]).to(dev))
    assert np.array_equal(ei.cpu().numpy(), c.a["filter.edge_index"]) and np.array_equal(m.cpu().numpy(), c.mask)


@pytest.mark.parametrize("seed", [0, 1])
def test_filter_and_build_on_a_random_graph(dev, seed):
    n, E = 300, 900
    ei = R.random_graph(n, E, 20 + seed).numpy()
    sel = np.random.default_rng(30 + seed).permutation(n)[:255]                          # unsorted
    assert not np.array_equal(sel, np.sort(sel))
    mask = _check_masked(R.randn((n, 5), 31).numpy(), R.randn((n, 2), 32).numpy(), ei, R.randn((E, 3), 33).numpy(), sel, dev)
    assert 0 < mask.sum() < E
    _check_masked(R.randn((n, 5), 31).numpy(), None, ei, None, sel, dev)


def test_build_masked_graph_is_one_gather_launch_and_one_count(dev, monkeypatch):
    c = Case("messy")
    graph = c.graph().to(dev)
    launches, counts = [], []
    real_call, real_count = P.call, P._subgraph_count
    monkeypatch.setattr(P, "call", lambda name, *a, **k: (launches.append(name), real_call(name, *a, **k))[1])
    monkeypatch.setattr(P, "_subgraph_count", lambda *a, **k: (counts.append(1), real_count(*a, **k))[1])
    gp.build_masked_graph(graph, c.t("selected").to(dev))
    assert launches.count("mgn_gather_rows_batch") == 1 and len(counts) == 1


# ------------------------------------------------------------------------------- 4. losses with selected_indexes
def _with_type9(p, S):
    """the reference side: the same problem with the types of rows ``S`` replaced by 9 (no mask selects 9); the geometry is shared"""
    q = copy.copy(p)
    q.node_type = p.node_type.clone()
    q.node_type[torch.as_tensor(S, dtype=torch.int64)] = 9.0
    q._ref = {}
    return q


def _run_selected(p, S, kinds, weights, method, dev):
    """``loss_cases.run`` with ``selected_indexes``: the engine on the ORIGINAL types"""
    to = lambda t: t.to(device=dev)  # noqa: E731
    net, u = to(p.net).requires_grad_(True), to(p.u_out).requires_grad_(True)
    sel = None if S is None else torch.as_tensor(S, dtype=torch.int64).to(dev)
    total, terms = LS.evaluate(list(kinds), list(weights), [1.0] * len(kinds), graph=p.mesh.graph(dev), target=to(p.tgt), network_output=net,
                               node_type=to(p.node_type), masks=list(p.masks), network_output_physical=u, target_physical=to(p.u_tgt),
                               gradient_method=method, selected_indexes=sel)
    r = LC.Run()
    r.fused = type(total.grad_fn).__name__.startswith("_FusedLossFn")
    r.total, r.terms = total.detach(), torch.stack([t.detach() for t in terms])
    r.finite = bool(torch.isfinite(total))
    r.d_net = r.d_u = None
    if r.finite:
        total.backward()
        r.d_net, r.d_u = net.grad, u.grad
    return r


def _pattern(name, N, seed):
    """(what the engine is given, the rows it names)"""
    rng = np.random.default_rng(seed)
    if name == "random":
        S = rng.permutation(N)[:max(1, int(0.15 * N))]
        return S, S
    if name == "block":
        S = np.arange(0, 32)                        # one whole 32-row block of the node pass: its partial sums are all zero
        return S, S
    S = rng.permutation(N)[:max(1, int(0.15 * N))]  # out-of-range and repeated ids change nothing
    return np.concatenate([S, S[:5], [-1, -7, N, N + 1000], S[::-1][:3]]), S


def _masked_problem(mesh_name, pattern):
    F = 3 if mesh_name == "tet3d" else 2

    def make(s):
        p = LC.Problem(LC.SMALL[mesh_name](300 + s), F, F, 400 + s)
        given, rows = _pattern(pattern, p.mesh.N, 900 + s)
        q = _with_type9(p, rows)
        q.original, q.given, q.rows = p, given, rows
        return q
    return LC.cached(("meshmask", mesh_name, pattern), lambda: LC.seeded(make))


@pytest.mark.parametrize("pattern", ["random", "block", "noisy"])
@pytest.mark.parametrize("mesh_name", sorted(LC.SMALL))
@pytest.mark.parametrize("method", LC.METHODS)
def test_losses_leave_the_listed_rows_out(dev, method, mesh_name, pattern):
    q = _masked_problem(mesh_name, pattern)
    # preconditions on the reference alone: |div| of every row that stays is away from zero (so DIV_L1 leaves no row out of the
    # comparison), rows of both kinds exist, and the listed rows do change the result
    assert q.div_margin(method) >= 1e-3
    assert float(LC.div_l1_rows_left_out(q, method).double().mean()) <= 0.01
    sel9, sel0 = REF.select(q.node_type, q.masks), REF.select(q.original.node_type, q.masks)
    assert 0 < int(sel9.sum()) < int(sel0.sum())
    got = _run_selected(q.original, q.given, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    assert got.fused, "the fused kernels did not run"
    LC.check(q, REF.ALL_KINDS, LC.WEIGHTS, method, dev, torch.float32, f"selected_indexes {pattern} {mesh_name} {method}",
             leave_out_div_l1=True, got=got)
    rows = torch.as_tensor(q.rows).to(dev)
    assert not bool(got.d_net[rows].any())            # a listed row's own residual has left every mean
    plain = LC.run(q.original, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    assert not torch.equal(plain.total, got.total)


@pytest.mark.parametrize("method", LC.METHODS)
def test_losses_empty_all_and_twice(dev, method):
    p = LC.small_problem("tri2d", 2)
    plain = LC.run(p, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    empty = _run_selected(p, np.empty(0, dtype=np.int64), REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    assert plain.fused and empty.fused
    for a, b in ((plain.total, empty.total), (plain.terms, empty.terms), (plain.d_net, empty.d_net), (plain.d_u, empty.d_u)):
        assert torch.equal(a, b), "an empty selected_indexes is not the call without the argument"
    # every row of a selected type listed: 0 / 0 = nan on both sides, nothing raises (loss_cases.case_zero_selected)
    every = torch.nonzero(REF.select(p.node_type, p.masks)).reshape(-1).numpy()
    ref = _with_type9(p, every).reference(REF.ALL_KINDS, LC.WEIGHTS, method)
    got = _run_selected(p, every, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    torch.cuda.synchronize()
    assert got.fused and bool(torch.isnan(ref.total)) and bool(torch.isnan(got.total))
    # two runs: bit-identical
    S, _ = _pattern("random", p.mesh.N, 77)
    a, b = (_run_selected(p, S, REF.ALL_KINDS, LC.WEIGHTS, method, dev) for _ in range(2))
    for x, y in ((a.total, b.total), (a.terms, b.terms), (a.d_net, b.d_net), (a.d_u, b.d_u)):
        assert torch.equal(x, y), "two runs differ"


def test_losses_beyond_the_grid_stride(dev):
    """32 942 rows: more than the 1024 blocks of 32 rows one pass of the node kernel covers"""
    method = "finite_diff"
    p = LC.Problem(LC.grid2d(181, 182, 500), 2, 2, 600)
    assert p.mesh.N == 32942 > 32768
    S, _ = _pattern("random", p.mesh.N, 78)
    S = np.concatenate([S, np.arange(32768, 32800)])          # a whole block of the second pass
    q = _with_type9(p, S)
    got = _run_selected(p, S, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    assert got.fused
    LC.check(q, REF.ALL_KINDS, LC.WEIGHTS, method, dev, torch.float32, "selected_indexes N=32942", leave_out_div_l1=True, got=got)
    assert not bool(got.d_net[torch.as_tensor(S).to(dev)].any())
    again = _run_selected(p, S, REF.ALL_KINDS, LC.WEIGHTS, method, dev)
    for x, y in ((got.total, again.total), (got.terms, again.terms), (got.d_net, again.d_net), (got.d_u, again.d_u)):
        assert torch.equal(x, y), "two runs differ"


def test_l2_loss_object_routes_by_the_argument(dev):
    p = LC.small_problem("tri2d", 2)
    net, tgt, ty = p.net.to(dev).requires_grad_(True), p.tgt.to(dev), p.node_type.to(dev)
    S, _ = _pattern("random", p.mesh.N, 79)
    with_s = gp.L2Loss()(target=tgt, network_output=net, node_type=ty, masks=list(p.masks), selected_indexes=torch.as_tensor(S).to(dev))
    assert type(with_s.grad_fn).__name__.startswith("_FusedLossFn")
    keep = REF.select(_with_type9(p, S).node_type, p.masks)
    want = ((p.net.double() - p.tgt.double()) ** 2)[keep].mean()
    assert rel_err(with_s, want) < LC.FWD_TOL
    without = gp.L2Loss()(target=tgt, network_output=net, node_type=ty, masks=list(p.masks))
    assert not type(without.grad_fn).__name__.startswith("_FusedLossFn")   # the existing masked-MSE path, untouched
    ml = gp.MultiLoss([gp.L2Loss(), gp.CosineLoss()], [1.0, 0.0])
    total = ml(target=tgt, network_output=net, node_type=ty, masks=list(p.masks), selected_indexes=torch.as_tensor(S).to(dev))
    assert rel_err(total, want) < LC.FWD_TOL


# ------------------------------------------------------------------------------- 5. a composed masked-pretraining step
def test_composed_step(dev):
    n, H, L = 256, 32, 2
    pos, ei, ea = R.delaunay_graph(n, 3)
    E = ei.shape[1]
    x0, ea0, y = R.randn((n, H), 41), R.randn((E, H), 42), R.randn((n, 2), 43)
    node_type = torch.zeros(n)
    node_type[::7] = 4.0
    torch.manual_seed(0)
    enc = gp.EncodeProcessDecode(L, H, H, H, hidden_size=H, only_processor=True).to(dev)
    dec = gp.EncodeProcessDecode(L, H, 3, 2, hidden_size=H).to(dev)
    token = torch.nn.Parameter(R.randn((H,), 44).to(dev))
    params = [("token", token)] + [("enc." + k, v) for k, v in enc.named_parameters()] + [("dec." + k, v) for k, v in dec.named_parameters()]
    sel = gp.get_masked_indexes(gp.Graph(x=x0.to(dev)), 0.15, seed=5, offset=2)
    assert sel.shape == (217,)
    left_out = sel   # the visible nodes are left out of the mean: the loss is on the masked ones

    def step(kernels):
        for _, p in params:
            p.grad = None
        g = gp.Graph(x=x0.to(dev), pos=pos.to(dev), edge_index=ei.to(dev), edge_attr=ea0.to(dev))
        full = gp.Graph(x=x0.to(dev), pos=pos.to(dev), edge_index=ei.to(dev))
        if kernels:
            g, edges_mask = gp.build_masked_graph(g, sel)
        else:
            table = torch.full((n,), -1, dtype=torch.int64, device=dev)
            table[sel] = torch.arange(sel.numel(), device=dev)
            s, r = table[g.edge_index[0]], table[g.edge_index[1]]
            edges_mask = (s >= 0) & (r >= 0)
            g.edge_index, g.edge_attr = torch.stack([s[edges_mask], r[edges_mask]]), g.edge_attr[edges_mask]
            g.x, g.pos = g.x[sel], g.pos[sel]
        latent = gp.Graph(x=enc(g))
        if kernels:
            rec = gp.reconstruct_graph(full, latent, sel, token, edges_mask)
        else:
            feats = torch.zeros(n, H, device=dev) + token.expand(n, -1)
            feats[sel] = latent.x
            rec = full.clone()
            rec.x = feats
        rec.edge_attr = ea.to(dev)
        out = dec(rec)
        ty, tgt = node_type.to(dev), y.to(dev)
        if kernels:
            loss = gp.L2Loss()(target=tgt, network_output=out, node_type=ty, masks=[0, 5], selected_indexes=left_out)
            assert type(loss.grad_fn).__name__.startswith("_FusedLossFn")
        else:
            keep = ((ty == 0) | (ty == 5)) & ~torch.isin(torch.arange(n, device=dev), left_out)
            loss = ((out - tgt) ** 2)[keep].mean()
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in params}

    want, want_g = step(False)
    got, got_g = step(True)
    r = rel_err(got, want)
    print(f"composed step: loss {float(got):.8e} vs {float(want):.8e}  rel {r:.2e}")
    assert bool(torch.isfinite(got)) and r < LOSS_TOL
    worst = max((rel_err(got_g[k], want_g[k]), k) for k in want_g)
    print(f"composed step: worst parameter gradient {worst[0]:.2e} ({worst[1]}) over {len(want_g)} tensors")
    for k in want_g:
        assert rel_err(got_g[k], want_g[k]) < GRAD_TOL, k
    assert bool(got_g["token"].any()), "the [MASK] token has no gradient"


# ------------------------------------------------------------------------------- 6. the preprocessing callable
def test_preprocessing_returns_the_pair_after_khop(dev, monkeypatch):
    base = gp.square_mesh(200, seed=1)
    make = lambda: gp.Graph(x=base.x.to(dev), y=base.y.to(dev), pos=base.pos.to(dev), edge_index=base.edge_index.to(dev))  # noqa: E731
    seen = []
    real = MM.get_masked_indexes
    monkeypatch.setattr(MM, "get_masked_indexes", lambda g, *a, **k: (seen.append(int(g.edge_index.shape[1])), real(g, *a, **k))[1])
    f = P.build_preprocessing(masking_ratio=0.15, khop=2, seed=9)
    plain = P.build_preprocessing(khop=2, seed=9)(make(), 4)
    graph, idx = f(make(), 4)
    assert torch.equal(graph.edge_index, plain.edge_index) and torch.equal(graph.edge_attr, plain.edge_attr) and torch.equal(graph.x, plain.x)
    assert seen == [int(plain.edge_index.shape[1])] and seen[0] > base.edge_index.shape[1]      # the draw saw the 2-hop edges
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.shape == (MM.masked_count(200, 0.15),) == (170,)
    assert torch.equal(idx, real(graph, 0.15, seed=9, offset=4)) and idx.unique().numel() == 170
    assert not torch.equal(idx, f(make(), 5)[1])
    assert not isinstance(P.build_preprocessing(khop=2)(make(), 4), tuple)
