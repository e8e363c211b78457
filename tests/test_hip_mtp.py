"""GPU: the kernels of ``training.use_spatial_mtp`` (csrc/mgn_starattn.inc) against fp64 torch on the same packed rows, the module
against the reference's arrays (tests/golden/mtp.npz) and the fp64 restatement (tests/mtp_reference.py), and the Engine's step against
the CPU Engine on a torch stand-in of the model."""
import math

import numpy as np
import pytest
import torch

import graph_physics_amd as gp
import mtp_reference as MR
from conftest import assert_close3, rel_err
from graph_physics_amd import _capi, harness, ops, spatial_mtp as SM

pytestmark = pytest.mark.gpu


def _off(lens, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------- star attention alone
def _attention64(qkv, lens, heads):
    """(y, lse, dqkv for the upstream gradient dy) per segment in fp64; dy is drawn here"""
    R, d3 = qkv.shape
    d, dh = d3 // 3, d3 // 3 // heads
    x = qkv.double().cpu().requires_grad_(True)
    ys, lses, at = [], [], 0
    for L in lens:
        q, k, v = x[at:at + L].split(d, dim=1)
        yh, lh = [], []
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            s = q[:, sl] @ k[:, sl].t() / math.sqrt(dh)
            yh.append(torch.softmax(s, dim=-1) @ v[:, sl])
            lh.append(torch.logsumexp(s, dim=-1))
        ys.append(torch.cat(yh, dim=1))
        lses.append(torch.stack(lh, dim=1))
        at += L
    y = torch.cat(ys)
    dy = torch.randn(R, d, dtype=torch.float64, generator=torch.Generator().manual_seed(R + d))
    (dqkv,) = torch.autograd.grad(y, x, dy)
    return y.detach(), torch.cat(lses).detach(), dy, dqkv


@pytest.mark.parametrize("d,heads", [(16, 1), (32, 4), (64, 8), (128, 4), (128, 16)])
def test_star_attention_against_fp64(dev, d, heads):
    T = _capi.lib().mgn_star_attn_tile_rows()
    lens = [1, 2, 3, 7, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
    R = sum(lens)
    qkv = torch.randn(R, 3 * d, generator=torch.Generator().manual_seed(17 * d + heads))
    y64, lse64, dy64, dqkv64 = _attention64(qkv, lens, heads)
    off = _off(lens, dev)
    runs = []
    for _ in range(2):
        x = qkv.to(dev).requires_grad_(True)
        y = gp.star_attention(x, off, heads)
        lse = y.grad_fn.saved_tensors[2].clone()
        (dqkv,) = torch.autograd.grad(y, x, dy64.float().to(dev))
        runs.append((y.detach().clone(), lse, dqkv.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                 # bit-identical from run to run
    y, lse, dqkv = runs[0]
    print("y", assert_close3(y, y64, 1e-5, "y"), "lse", rel_err(lse, lse64), "dqkv", assert_close3(dqkv, dqkv64, 2e-5, "dqkv"))
    assert rel_err(lse, lse64) < 1e-5


def test_star_attention_one_segment_and_no_rows(dev):
    d, heads, L = 32, 4, 21
    qkv = torch.randn(L, 3 * d, generator=torch.Generator().manual_seed(3))
    y64, _, dy64, dqkv64 = _attention64(qkv, [L], heads)
    x = qkv.to(dev).requires_grad_(True)
    y = gp.star_attention(x, _off([L], dev), heads)                # B = 1
    (dqkv,) = torch.autograd.grad(y, x, dy64.float().to(dev))
    assert_close3(y, y64, 1e-5, "y")
    assert_close3(dqkv, dqkv64, 2e-5, "dqkv")
    lib = _capi.lib()
    assert lib.mgn_star_attn_fwd(None, None, 0, 0, d, heads, None, None, None) == 0        # R = 0: 0 without a launch
    assert lib.mgn_star_attn_bwd(None, None, None, None, None, 0, 0, d, heads, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- pack and its backward
def _csr(edge_index, N, dev):
    rowptr, nbr = SM._csr_of_edges(edge_index.to(dev), N, True)
    return rowptr.to(torch.int32).contiguous(), nbr.to(torch.int32).contiguous()


def _hub_graph():
    """30 nodes; node 7 is a neighbour of the centres 2, 11 and 20 and a centre itself; nodes 25..29 touch no star"""
    pairs = [(2, 7), (2, 3), (11, 7), (11, 12), (11, 13), (20, 7), (20, 21), (7, 8), (7, 9), (4, 5), (26, 27)]
    e = torch.tensor(pairs, dtype=torch.int64).t()
    return torch.cat([e, e.flip(0)], dim=1), 30, torch.tensor([2, 11, 7, 20, 24])   # (24: a centre without neighbours)


@pytest.mark.parametrize("d,shared", [(64, False), (128, False), (16, True)])
def test_pack_and_its_backward(dev, d, shared):
    ei, N, centers = _hub_graph()
    g = torch.Generator().manual_seed(d)
    H, Hn, scale = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g), 1 + 0.1 * torch.randn(d, generator=g)
    rowptr, nbr = _csr(ei, N, dev)
    nb = MR.neighbours(ei, N)
    row_node = [v for c in centers.tolist() for v in [c] + nb[c]]
    row_star = [b for b, c in enumerate(centers.tolist()) for _ in range(1 + len(nb[c]))]
    is_c = torch.tensor([i == 0 for c in centers.tolist() for i in range(1 + len(nb[c]))])
    R = len(row_node)
    dX = torch.randn(R, d, generator=g)
    # fp64 index ops
    H64, Hn64, s64 = (t.double().requires_grad_(True) for t in (H, Hn, scale))
    idx = torch.tensor(row_node)
    X64 = MR.rms(torch.where(is_c.unsqueeze(1), H64[idx], (H64 if shared else Hn64)[idx]), s64)
    X64.backward(dX.double())
    runs = []
    for _ in range(2):
        Hd, Hnd, sd = (t.to(dev).requires_grad_(True) for t in (H, Hn, scale))
        tabs, stats = SM.star_tables(rowptr, nbr, centers.to(dev), N)
        X = SM.pack_stars(Hd, None if shared else Hnd, sd, tabs)
        X.backward(dX.to(dev))
        runs.append((X.detach().clone(), Hd.grad.clone(), sd.grad.clone()) + (() if shared else (Hnd.grad.clone(),)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert tabs["R"] == R and tabs["B"] == 5 and stats.tolist() == [float(R - 5), 5.0]
    # (neighbour order inside a star: the CSR's, stable by edge id = the edge order MR.neighbours walks)
    assert tabs["row_node"].tolist() == row_node and tabs["row_star"].tolist() == row_star
    assert tabs["nb_rows"][:R - 5].tolist() == [r for r in range(R) if not is_c[r]]
    assert tabs["nb_ptr"].tolist() == [int((~is_c[:r]).sum()) for r in range(R + 1)]
    X, dH, dscale = runs[0][:3]
    assert_close3(X, X64, 1e-5, "X")
    assert_close3(dH, H64.grad, 2e-5, "dH")
    assert_close3(dscale, s64.grad, 2e-5, "dscale")
    touched_c = set(centers.tolist())
    touched_n = {v for c in centers.tolist() for v in nb[c]}
    if shared:
        zero = [i for i in range(N) if i not in touched_c | touched_n]
    else:
        dHn = runs[0][3]
        assert_close3(dHn, Hn64.grad, 2e-5, "dH_neigh")
        zero = [i for i in range(N) if i not in touched_c]
        assert bool((dHn[[i for i in range(N) if i not in touched_n]] == 0).all())
        # node 7: three neighbour rows summed into dH_neigh, its one centre row into dH
        assert sum(1 for r in range(R) if row_node[r] == 7 and not is_c[r]) == 3 and bool((dHn[7] != 0).all()) and bool((dH[7] != 0).all())
    assert 25 in zero and bool((dH[zero] == 0).all())             # rows of untouched nodes are exactly zero


def test_pack_sums_a_repeated_centre(dev):
    ei, N, _ = _hub_graph()
    d = 32
    centers = torch.tensor([7, 2, 7])
    H = torch.randn(N, d, generator=torch.Generator().manual_seed(1))
    rowptr, nbr = _csr(ei, N, dev)
    Hd, sd = H.to(dev).requires_grad_(True), torch.ones(d, device=dev)
    tabs, _ = SM.star_tables(rowptr, nbr, centers.to(dev), N)
    X = SM.pack_stars(Hd, H.to(dev), sd, tabs)
    dX = torch.randn(tabs["R"], d, generator=torch.Generator().manual_seed(2))
    X.backward(dX.to(dev))
    H64 = H.double().requires_grad_(True)
    rows = [int(tabs["off"][b]) for b in range(3)]
    MR.rms(H64[centers], torch.ones(d, dtype=torch.float64)).backward(dX[rows].double())
    assert_close3(Hd.grad, H64.grad, 2e-5, "dH with a repeated centre")


# ------------------------------------------------------------------------------- loss tail
@pytest.mark.parametrize("reduction", ["mean_per_center", "mean"])
@pytest.mark.parametrize("O", [1, 3, 32])
def test_loss_tail_against_fp64(dev, reduction, O):
    ei, N, centers = _hub_graph()
    rowptr, nbr = _csr(ei, N, dev)
    tabs, _ = SM.star_tables(rowptr, nbr, centers.to(dev), N)
    SM.pack_stars(torch.zeros(N, 16, device=dev), None, torch.ones(16, device=dev), tabs)     # fills row_node
    T = tabs["R"] - tabs["B"]
    g = torch.Generator().manual_seed(O)
    yhat, target = torch.randn(T, O, generator=g), torch.randn(N, O, generator=g)
    nb = MR.neighbours(ei, N)
    degs = [len(nb[c]) for c in centers.tolist()]
    assert 0 in degs                                                # a degree-0 star among the others
    y64 = yhat.double().requires_grad_(True)
    nodes = torch.tensor([v for c in centers.tolist() for v in nb[c]])
    err = (y64 - target.double()[nodes]).pow(2).mean(dim=-1)
    owner = torch.tensor([b for b, k in enumerate(degs) for _ in range(k)])
    per = torch.zeros(len(degs), dtype=torch.float64).index_add(0, owner, err) / torch.tensor(degs, dtype=torch.float64).clamp_min(1)
    want = err.mean() if reduction == "mean" else per.mean()
    want.backward()
    yd = yhat.to(dev).requires_grad_(True)
    loss, pair = SM.star_loss(yd, target.to(dev), tabs, reduction)
    (3.0 * loss).backward()
    assert rel_err(loss, want.detach()) < 1e-5 and rel_err(pair, err.mean().detach()) < 1e-5
    assert_close3(yd.grad, 3.0 * y64.grad, 1e-5, "dyhat")


# ------------------------------------------------------------------------------- neighbour cap
def _ring_lattice(N, dev):
    i = torch.arange(N)
    e = torch.cat([torch.stack([i, (i + s) % N]) for s in (1, 2, 3, 4)], dim=1)
    return _csr(torch.cat([e, e.flip(0)], dim=1), N, dev)


def test_neighbour_cap(dev):
    N = B = 2000
    rowptr, nbr = _ring_lattice(N, dev)
    assert bool(((rowptr[1:] - rowptr[:-1]) == 8).all())
    centers = torch.randperm(N, generator=torch.Generator().manual_seed(9)).to(dev)
    tabs, stats = SM.star_tables(rowptr, nbr, centers, N, max_neighbors=4, seed=11, step=5)
    assert tabs["R"] == 5 * B and stats.tolist() == [4.0 * B, 4.0]
    keep = tabs["keep"].cpu().reshape(B, 4)
    assert bool(((keep >= 0) & (keep < 8)).all()) and all(len(set(r)) == 4 for r in keep.tolist())   # 4 distinct positions of its own row
    again, _ = SM.star_tables(rowptr, nbr, centers, N, max_neighbors=4, seed=11, step=5)
    other, _ = SM.star_tables(rowptr, nbr, centers, N, max_neighbors=4, seed=11, step=6)
    assert torch.equal(again["keep"], tabs["keep"]) and not torch.equal(other["keep"], tabs["keep"])
    freq = torch.bincount(keep.flatten(), minlength=8).double() / B
    print("kept frequency per position", freq.tolist())
    assert bool(((freq - 0.5).abs() < 0.06).all())                 # five standard deviations of sqrt(0.25 / 2000)
    # the kept rows are the centre's own neighbours at those positions
    H = torch.arange(N, dtype=torch.float32, device=dev).unsqueeze(1).repeat(1, 16)
    SM.pack_stars(H, None, torch.ones(16, device=dev), tabs)
    rn = tabs["row_node"].cpu().reshape(B, 5)
    base = rowptr.cpu()[centers.cpu().long()].long()
    assert torch.equal(rn[:, 0], centers.cpu().int()) and torch.equal(rn[:, 1:].long(), nbr.cpu().long()[base.unsqueeze(1) + keep.long()])
    # a cap that cuts nothing: the uncapped stars
    plain, _ = SM.star_tables(rowptr, nbr, centers, N)
    SM.pack_stars(H, None, torch.ones(16, device=dev), plain)
    for k in (8, 20):
        t, st = SM.star_tables(rowptr, nbr, centers, N, max_neighbors=k, seed=11, step=5)
        SM.pack_stars(H, None, torch.ones(16, device=dev), t)
        assert torch.equal(t["off"], plain["off"]) and torch.equal(t["row_node"], plain["row_node"]) and st.tolist() == [8.0 * B, 8.0]
        assert torch.equal(t["keep"].cpu().reshape(B, 8), torch.arange(8, dtype=torch.int32).repeat(B, 1))


# ------------------------------------------------------------------------------- the module
def _device_module(c, dev):
    m = gp.SpatialMTP1Hop(c.d, num_heads=c.heads, num_layers=c.layers, assume_undirected=c.assume_undirected)
    m.load_state_dict(c.w, strict=True)
    head = gp.build_mlp(c.d, c.d, c.O, layer_norm=False)
    head.load_state_dict(c.head, strict=True)
    return m.to(dev), head.to(dev)


def _run_device(m, head, H, Hn, ei, centers, target, dev, **kw):
    Hd = H.to(dev).requires_grad_(True)
    Hnd = Hn.to(dev).requires_grad_(True) if Hn is not None else None
    for p in list(m.parameters()) + list(head.parameters()):
        p.grad = None
    loss, stats = m(Hd, ei.to(dev), centers.to(dev), head, target.to(dev), H_neigh=Hnd, **kw)
    grads = {}
    if loss.requires_grad:
        loss.backward()
        grads = {"H": Hd.grad, "H_neigh": Hnd.grad if Hnd is not None else None}
        grads.update({"w." + k: p.grad.clone() for k, p in m.named_parameters()})
        grads.update({"head." + k: p.grad.clone() for k, p in head.named_parameters()})
    return loss.detach(), stats, grads


@pytest.mark.parametrize("name", MR.CASES)
def test_module_against_the_reference(dev, name):
    c = MR.Case(name)
    m, head = _device_module(c, dev)
    loss, stats, grads = _run_device(m, head, c.H, c.H_neigh if c.has_neigh else None, c.edge_index, c.centers, c.target, dev,
                                     **c.forward_kwargs(dev))
    assert all(v.is_cuda for v in stats.values())                  # device scalars
    seen = MR.check_against_case(c, loss, stats, grads)
    assert (seen > 0) == (name not in ("isolated", "empty"))


def _random_mesh(N, seed):
    g = gp.square_mesh(N, seed)
    return g.edge_index


@pytest.mark.parametrize("d", [64, 128])
def test_module_wide_against_the_restatement(dev, d):
    N, O, heads, B = 300, 3, 4, 48
    ei = _random_mesh(N, 5)
    N = int(ei.max()) + 1 if int(ei.max()) + 1 > N else N
    torch.manual_seed(d)
    m = gp.SpatialMTP1Hop(d, num_heads=heads, num_layers=1)
    head = gp.build_mlp(d, d, O, layer_norm=False)
    g = torch.Generator().manual_seed(d + 1)
    with torch.no_grad():
        for p in list(m.parameters()) + list(head.parameters()):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    H, Hn, target = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g), torch.randn(N, O, generator=g)
    centers = torch.randperm(N, generator=g)[:B]
    w, hw = {k: v.detach().clone() for k, v in m.state_dict().items()}, {k: v.detach().clone() for k, v in head.state_dict().items()}
    want = MR.star_mtp(w, hw, H, Hn, ei, centers, target, heads, 1)
    m, head = m.to(dev), head.to(dev)
    loss, stats, grads = _run_device(m, head, H, Hn, ei, centers, target, dev)
    assert rel_err(loss, want["loss"]) < 1e-5
    for k, v in want["stats"].items():
        assert abs(float(stats[k]) - v) <= 1e-5 * max(1.0, abs(v)), k
    for k, v in want["g"].items():
        print(k, assert_close3(grads[k], v, 2e-5, k))
    # the adjacency from an ops.Topology (its source-grouped CSR) instead of a sort of edge_index
    topo = ops.Topology(ei.to(dev), N)
    loss_t, stats_t, grads_t = _run_device(m, head, H, Hn, ei, centers, target, dev, topology=topo)
    assert rel_err(loss_t, want["loss"]) < 1e-5 and float(stats_t["sp_mtp/pairs"]) == want["stats"]["sp_mtp/pairs"]
    for k, v in want["g"].items():
        assert_close3(grads_t[k], v, 2e-5, k + " (topology)")


# ------------------------------------------------------------------------------- the Engine
def _cfg(**training):
    cfg = gp.cylinder_config(2, 32)
    cfg["training"] = dict(cfg["training"], **training)
    return cfg


def _batch(seed=3):
    g = gp.collate([gp.cylinder_mesh(70, seed), gp.cylinder_mesh(90, seed + 1)])
    rng = np.random.default_rng(seed)
    g.y = g.x[:, :2] + torch.from_numpy(0.1 * rng.standard_normal((g.x.shape[0], 2)).astype(np.float32))
    return g


def _engine(dev, cfg, seed=5):
    torch.manual_seed(seed)
    return harness.Engine(cfg, dev, learning_rate=1e-3, warmup=1, grad_clip=1e9)


def _step(eng, batch, centers):
    """one eager step; (loss, stats, gradients by name) -- the gradients as the backward left them (grad_clip 1e9: the clip is the identity)"""
    loss = eng.train_step(batch, mtp_centers=centers)
    named = dict(eng.sim.named_parameters())
    if eng.spatial_mtp is not None:
        named.update({"spatial_mtp." + k: p for k, p in eng.spatial_mtp.named_parameters()})
    return loss, eng.last_mtp_stats, {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}


def test_engine_step_against_the_cpu_engine(dev, monkeypatch):
    cfg = _cfg(use_spatial_mtp=True, spatial_mtp_alpha=0.3)
    batch = _batch()
    N = batch.x.shape[0]
    centers = torch.tensor([0, 5, 17, 69, 70, 71, 100, N - 1, 33, 140])
    eng = _engine(dev, cfg)
    state = {k: v.detach().cpu().clone() for k, v in eng.state_dict().items()}
    loss, stats, grads = _step(eng, batch.to(dev), centers.to(dev))
    with monkeypatch.context() as mp:
        mp.setattr(harness, "get_model", lambda param, only_processor=False: MR.TorchEPD(2, 2 + 9, 3, 2, 32))
        cpu = _engine(torch.device("cpu"), cfg)
    cpu.load_state_dict(state)
    loss_c, stats_c, grads_c = _step(cpu, batch, centers)
    print("loss", float(loss), float(loss_c))
    assert rel_err(loss, loss_c) < 1e-5
    assert sorted(stats) == sorted(stats_c) == sorted(list(MR.STAT_NAMES) + ["sp_mtp/aux_loss"])
    for k in stats:
        assert rel_err(stats[k], stats_c[k]) < 1e-5, k
    assert sorted(grads) == sorted(grads_c) and any(k.startswith("spatial_mtp.") for k in grads)
    for k in grads:
        print(k, assert_close3(grads[k], grads_c[k], 2e-5, k))
    # the same step with the node renumbering forced on: the hooks see the engine's numbering, the branch the caller's
    mode = gp.get_node_renumbering()
    try:
        gp.set_node_renumbering("on")
        ren = _engine(dev, cfg)
        ren.load_state_dict({k: v.to(dev) for k, v in state.items()})
        b2 = _batch().to(dev)
        loss_r, stats_r, grads_r = _step(ren, b2, centers.to(dev))
        topo = ops.get_topology(b2.edge_index, N, pos=b2.pos, renumber=True)
        assert topo.node_order is not None                          # the mesh WAS renumbered
    finally:
        gp.set_node_renumbering(mode)
    assert rel_err(loss_r, loss) < 1e-5 and rel_err(stats_r["sp_mtp/aux_loss"], stats["sp_mtp/aux_loss"]) < 1e-5
    for k in grads:
        assert_close3(grads_r[k], grads[k], 2e-5, k + " (renumbered)")


def _model_cfg(kind):
    """configs whose models number the hooked rows by rules of their own: the sparse-attention Transformer (its attention topology's
    Morton order) and the EPD with the temporal block (rows brought back to the caller's numbering BEFORE the decoder)"""
    cfg = _cfg(use_spatial_mtp=True, spatial_mtp_alpha=0.3)
    if kind == "transformer":
        cfg["model"] = {"type": "transformer", "message_passing_num": 2, "hidden_size": 32, "node_input_size": 2, "output_size": 2,
                        "edge_input_size": 0, "num_heads": 4, "use_rope_embeddings": False, "use_gated_attention": False}
    else:
        cfg["training"]["use_temporal_block"] = True
    return cfg


@pytest.mark.parametrize("kind", ["transformer", "epd_temporal"])
def test_engine_step_under_each_models_own_renumbering(dev, kind):
    cfg = _model_cfg(kind)
    N = _batch().x.shape[0]
    centers = torch.tensor([0, 5, 17, 69, 70, 71, 100, N - 1, 33, 140]).to(dev)
    mode = gp.get_node_renumbering()
    out = {}
    try:
        for m in ("off", "on"):
            gp.set_node_renumbering(m)
            eng = _engine(dev, cfg)                                 # the same seed: the same weights
            b = _batch().to(dev)
            out[m] = _step(eng, b, centers)
            ranks = eng.model.last_node_rank
            # "on": the encoder's rows WERE renumbered; the temporal block hands the decoder the caller's numbering again
            assert (ranks["nodes_encoder"] is not None) == (m == "on")
            assert (ranks["decode_module"] is not None) == (m == "on" and kind == "transformer")
    finally:
        gp.set_node_renumbering(mode)
    (loss, stats, grads), (loss_r, stats_r, grads_r) = out["off"], out["on"]
    assert float(stats["sp_mtp/pairs"]) > 0 and any(k.startswith("spatial_mtp.") for k in grads)
    assert rel_err(loss_r, loss) < 1e-5 and rel_err(stats_r["sp_mtp/aux_loss"], stats["sp_mtp/aux_loss"]) < 1e-5
    assert sorted(grads) == sorted(grads_r)
    for k in grads:
        if k.endswith("k_proj.bias"):
            # a key bias shifts every score of a row alike, which the softmax ignores: this gradient is zero in exact arithmetic, and
            # what is stored is rounding residue (1e-12 here).  It has no scale of its own: held against the key weight's gradient
            scale = float(grads[k[:-4] + "weight"].abs().max())
            assert float(grads_r[k].abs().max()) < 2e-5 * scale and float(grads[k].abs().max()) < 2e-5 * scale, k
            continue
        assert_close3(grads_r[k], grads[k], 2e-5, k + " (renumbered)")


def test_engine_without_the_key_is_bit_identical(dev):
    off = _cfg(use_spatial_mtp=False)
    absent = _cfg()
    del absent["training"]["use_spatial_mtp"]
    batch = _batch().to(dev)
    a, b = _engine(dev, off), _engine(dev, absent)
    assert a.spatial_mtp is None and b.spatial_mtp is None
    for _ in range(2):
        assert torch.equal(a.train_step(batch), b.train_step(batch))
