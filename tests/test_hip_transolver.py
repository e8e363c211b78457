"""GPU: the slice-attention launches of include/mgn_hip_slice.h (csrc/mgn_slice.inc) against the fp64 restatement
(tests/transolver_reference.py), their noise stream and run-to-run bit identity, the module and the Engine against the reference's arrays
(tests/golden/transolver.npz) and the CPU torch-ops path.

Bounds: per compared tensor the larger of the project's convention (1e-5 of the fp64 tensor's largest entry forward, 2e-5 for gradients)
and 4 x the error of an fp32 evaluation on the CPU against fp64 for that tensor -- the golden's fp32 run where there is one; for the
kernel shapes the restatement's functions evaluated with fp32 operands (`_restate(P, torch.float32, ...)`: the matrix products, GELUs,
reductions and the token part run in fp32, but `transolver_reference.gumbel32` hands back fp64 noise, so the logit sum, the division by
the temperature and the softmax of that evaluation are promoted to fp64 -- it is NOT a pure fp32 run, its error is the smaller one and
the bound the tighter for it); for the Engine step the CPU Engine in fp32 against the CPU Engine in fp64.  Never a figure of the code
under test.  Every test prints the ratio it observes."""
import numpy as np
import pytest
import torch

import graph_physics_amd as gp
import transolver_reference as TR
from conftest import rel_err
from graph_physics_amd import _capi, harness, transolver as TS
from graph_physics_amd.mesh import Graph
from test_transolver_host import CASES, _config, build, compare, run

pytestmark = pytest.mark.gpu


def _pass_rows(launch, G):
    return int(_capi.lib().mgn_slice_pass_rows(launch, G))


def _inputs(N, H, G, C, scale=0.5, bias=0.5, seed=0):
    """random operands (fp32, CPU) with u = 0 and u = 1 - 2^-24 planted; the seed advances until no row's pre-clamp temperature (fp64)
    lies within 1e-3 of the clamp point, where the gradient has a kink"""
    while True:
        g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * G + C + 7919 * seed)
        r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        P = dict(xm=r(N, H * C), Ws=scale * r(G, C), bs=0.1 * r(G), W1=0.5 * r(G, C), b1=0.1 * r(G), w2=0.5 * r(1, G), b2=0.1 * r(1),
                 bias=torch.full((1, H, 1, 1), 0.5) if bias is None else torch.as_tensor(bias, dtype=torch.float32).expand(H).reshape(1, H, 1, 1).clone(),
                 Wq=0.5 * r(C, C), Wk=0.5 * r(C, C), Wv=0.5 * r(C, C), dOut=r(N, H * C), u=torch.rand(N, H, G, generator=g))
        P["u"][0, 0, 0] = 0.0
        P["u"][N - 1, H - 1, G - 1] = 1.0 - 2.0 ** -24
        _, _, tpre = TR.weights(P["xm"].double().view(N, H, C), *(P[k].double() for k in ("Ws", "bs", "W1", "b1", "w2", "b2", "bias")), P["u"])
        if float((tpre - TR.CLAMP).abs().min()) > 1e-3:
            return P, tpre
        seed += 1


NAMES = ("xm", "Ws", "bs", "W1", "b1", "w2", "b2", "bias", "Wq", "Wk", "Wv")


def _restate(P, dtype, N, H, G, C):
    """(out, w, S, norm, grads in the order of NAMES) of the restatement's functions evaluated in `dtype` on the CPU"""
    t = {k: P[k].to(dtype).clone().requires_grad_(True) for k in NAMES}
    xm = t["xm"].view(N, H, C)
    w, _, _ = TR.weights(xm, t["Ws"], t["bs"], t["W1"], t["b1"], t["w2"], t["b2"], t["bias"], P["u"])
    w = w.to(dtype)
    S, norm = TR.aggregate(w, xm)
    out = TR.expand(w, TR.tokens(S, norm, t["Wq"], t["Wk"], t["Wv"])).reshape(N, H * C)
    grads = torch.autograd.grad(out, [t[k] for k in NAMES], P["dOut"].to(dtype))
    return [out.detach(), w.detach(), S.detach(), norm.detach()] + list(grads)


def _hip(P, dev, N, H, G, C, u_given=True, seed=0, step=None, layer=0):
    t = {k: P[k].to(dev).clone().requires_grad_(True) for k in NAMES}
    step = torch.zeros(1, dtype=torch.int64, device=dev) if step is None else step

    def tokens(S, norm):
        return TR.tokens(S, norm, t["Wq"], t["Wk"], t["Wv"])

    out = TS._SliceAttnFn.apply(t["xm"], t["Ws"], t["bs"], t["W1"], t["b1"], t["w2"], t["b2"], t["bias"], P["u"].to(dev) if u_given else None, step,
                                (seed, layer, H, G, C), tokens, t["Wq"], t["Wk"], t["Wv"])
    w = out.grad_fn.saved_tensors[1].clone()
    S, norm = TS.slice_aggregate(w, t["xm"].detach(), H, G, C)
    grads = torch.autograd.grad(out, [t[k] for k in NAMES], P["dOut"].to(dev))
    return [out.detach().clone(), w, S, norm] + [g.clone() for g in grads]


def _check(tag, got, r64, r32):
    labels = ["out", "w", "S", "norm"] + ["d" + k for k in NAMES]
    worst = ("", 0.0)
    for i, name in enumerate(labels):
        conv = 1e-5 if i < 4 else 2e-5
        bd = TR.bound(conv, rel_err(r32[i], r64[i]))
        e = rel_err(got[i].reshape(r64[i].shape), r64[i])
        if e / bd > worst[1]:
            worst = (name, e / bd)
        assert e < bd, f"{tag} {name}: {e:.3e} >= {bd:.3e}"
    print(f"{tag}: worst error / bound = {worst[1]:.3f} ({worst[0]})")


# (N, H, G, C, logit scale, bias): odd sizes, tile edges, several workgroups, every lane-group width P in {1, 8, 32, 64}
SHAPES = [(1, 1, 1, 2, 0.5, None), (63, 2, 8, 8, 0.5, None), (64, 8, 24, 2, 0.5, None), (65, 1, 32, 16, 0.5, None), (257, 2, 64, 64, 0.5, None),
          (65, 2, 8, 16, 0.5, None), (257, 8, 32, 16, 0.5, None), (64, 1, 64, 8, 0.5, None), (63, 8, 1, 16, 0.5, None),
          (257, 2, 8, 8, 30.0, None),                  # logits of +-30
          (257, 2, 8, 16, 0.5, [-0.1, 0.5])]           # head 0: clamped and unclamped rows mixed


@pytest.mark.parametrize("N,H,G,C,scale,bias", SHAPES)
def test_launches_against_the_restatement(dev, N, H, G, C, scale, bias):
    """Measured on an MI355X, worst error / bound: 0.004 .. 0.33 over the nine plain shapes, 0.24 with logits of +-30, 0.48 with clamped
    and unclamped rows mixed.  (With the temperature's gradient formed as -sum_g dz_g y_g / t^2, a sum that cancels at the size of y,
    the last two sat at 1.4 and 2.0; the kernels take the row maximum off y first.)"""
    P, tpre = _inputs(N, H, G, C, scale, bias)
    if bias is not None:
        frac = float((tpre[:, 0] < TR.CLAMP).double().mean())
        assert 0.1 < frac < 0.9, frac
    r64, r32 = _restate(P, torch.float64, N, H, G, C), _restate(P, torch.float32, N, H, G, C)
    a, b = _hip(P, dev, N, H, G, C), _hip(P, dev, N, H, G, C)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                    # bit-identical from run to run, every launch
    _check(f"N={N} H={H} G={G} C={C}", a, r64, r32)


def test_more_than_two_grid_passes(dev):
    """one row count just above twice what ONE pass of each launch's grid covers (mgn_slice_pass_rows: the launches' own constants)"""
    H, G, C = 1, 64, 2
    per_pass = {l: _pass_rows(l, G) for l in (2, 3, 4, 5)}
    assert all(v > 0 for v in per_pass.values())
    N = 2 * max(per_pass[2] // H, per_pass[3], per_pass[4], per_pass[5]) + 1
    print("rows per grid pass", per_pass, "N", N)
    P, _ = _inputs(N, H, G, C)
    r64, r32 = _restate(P, torch.float64, N, H, G, C), _restate(P, torch.float32, N, H, G, C)
    a, b = _hip(P, dev, N, H, G, C), _hip(P, dev, N, H, G, C)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _check(f"N={N}", a, r64, r32)


def test_leading_dimension_and_the_single_launches(dev):
    N, H, G, C, ld = 65, 2, 8, 8, 48
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(N, ld, generator=g)
    w = torch.softmax(torch.randn(N, H, G, generator=g), dim=-1)
    tok = torch.randn(H, G, C, generator=g)
    xs = wide.to(dev)[:, 16:16 + H * C]                                    # a column slab: leading dimension 48 > H * C
    S, norm = TS.slice_aggregate(w.to(dev), xs, H, G, C)
    S64, n64 = TR.aggregate(w.double(), wide[:, 16:16 + H * C].double().reshape(N, H, C))
    out = TS.slice_expand(w.to(dev), tok.to(dev), H, G, C)
    e = [rel_err(S, S64), rel_err(norm, n64), rel_err(out, TR.expand(w.double(), tok.double()).reshape(N, H * C))]
    print("S, norm, out:", e)
    assert max(e) < 1e-5


def _abi_chain(dev, P, N, H, G, C, ld, at):
    """launches 2, 3, 4 and 5 straight through the C ABI with every row matrix (x_mid, the expanded output, dOut, dx) as the column slab
    [at, at + H * C) of an [N, ld] buffer filled with 7: (results by name, the two written wide buffers)"""
    from graph_physics_amd._launch import call, workspace
    f = dict(dtype=torch.float32, device=dev)
    L = _capi.lib()

    def wide(src=None):
        t = torch.full((N, ld), 7.0, **f)
        if src is not None:
            t[:, at:at + H * C] = src.to(dev)
        return t

    p = lambda t: t.data_ptr()   # noqa: E731
    d = {k: P[k].to(dev).contiguous() for k in ("Ws", "bs", "W1", "b1", "w2", "b2", "u")}
    bias = P["bias"].to(dev).reshape(-1).contiguous()
    tok, dS, dnorm = (P[k].to(dev).contiguous() for k in ("tok", "dS", "dnorm"))
    xw, dow, outw, dxw = wide(P["xm"]), wide(P["dOut"]), wide(), wide()
    xs, dos, outs, dxs = (t[:, at:] for t in (xw, dow, outw, dxw))
    w, rowsc = torch.empty(N, H, G, **f), torch.empty(N * H, 2, **f)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    call("mgn_slice_weights_fwd", dev, p(xs), ld, p(d["Ws"]), p(d["bs"]), p(d["W1"]), p(d["b1"]), p(d["w2"]), p(d["b2"]), p(bias), p(d["u"]), 0,
         p(step), 0, N, H, G, C, p(w), p(rowsc))
    S, norm = torch.empty(H, G, C, **f), torch.empty(H, G, **f)
    ws = workspace(L.mgn_slice_aggregate_workspace_bytes(N, H, G, C), dev)
    call("mgn_slice_aggregate", dev, p(w), p(xs), ld, N, H, G, C, p(S), p(norm), p(ws), ws.numel())
    call("mgn_slice_expand", dev, p(w), p(tok), N, H, G, C, p(outs), ld)
    da, dh1, dt2 = torch.empty(N * H, G, **f), torch.empty(N * H, G, **f), torch.empty(N * H, **f)
    dw2, db2, dbias = torch.empty(G, **f), torch.empty(1, **f), torch.empty(H, **f)
    ws = workspace(L.mgn_slice_rows_bwd_workspace_bytes(N, H, G), dev)
    call("mgn_slice_rows_bwd", dev, p(dos), ld, p(tok), p(dS), p(dnorm), p(xs), ld, p(w), p(rowsc), p(d["Ws"]), p(d["bs"]), p(d["W1"]), p(d["b1"]),
         p(d["w2"]), p(d["u"]), 0, p(step), 0, N, H, G, C, p(dxs), ld, p(da), p(dh1), p(dt2), p(dw2), p(db2), p(dbias), p(ws), ws.numel())
    torch.cuda.synchronize()
    res = dict(w=w, rowsc=rowsc, S=S, norm=norm, out=outw[:, at:at + H * C].clone(), dx=dxw[:, at:at + H * C].clone(), da=da, dh1=dh1, dt2=dt2,
               dw2=dw2, db2=db2, dbias=dbias)
    return res, (outw, dxw)


def test_leading_dimensions_of_the_row_launches(dev):
    """every launch that takes a leading dimension (ldx of 2, 3 and 5, ldo of 4, lddo and lddx of 5) fed a column slab of a wider matrix:
    the same bits as with dense rows, and not one element written outside the slab"""
    N, H, G, C = 65, 2, 8, 8
    P, _ = _inputs(N, H, G, C)
    g = torch.Generator().manual_seed(11)
    P.update(tok=torch.randn(H, G, C, generator=g), dS=torch.randn(H, G, C, generator=g), dnorm=torch.randn(H, G, generator=g))
    dense, _ = _abi_chain(dev, P, N, H, G, C, H * C, 0)
    slab, wides = _abi_chain(dev, P, N, H, G, C, 48, 20)
    for k in dense:
        assert torch.equal(dense[k], slab[k]), k
    for t in wides:
        assert bool((t[:, :20] == 7.0).all()) and bool((t[:, 20 + H * C:] == 7.0).all())
    # and the dense chain is the chain the restatement describes (launch 5's dx against autograd through the same fixed tokens)
    xm = P["xm"].double().view(N, H, C).requires_grad_(True)
    w64, _, _ = TR.weights(xm, *(P[k].double() for k in ("Ws", "bs", "W1", "b1", "w2", "b2", "bias")), P["u"])
    S64, n64 = TR.aggregate(w64, xm)
    out64 = TR.expand(w64, P["tok"].double()).reshape(N, H * C)
    obj = (out64 * P["dOut"].double()).sum() + (S64 * P["dS"].double()).sum() + (n64 * P["dnorm"].double()).sum()
    (dx64,) = torch.autograd.grad(obj, xm)
    e = [rel_err(dense["out"], out64), rel_err(dense["S"], S64), rel_err(dense["dx"], dx64.reshape(N, H * C))]
    print("out, S, dx:", e)
    assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 2e-5


# ------------------------------------------------------------------------------------------- the noise stream
def test_noise_stream(dev):
    N, H, G, C = 257, 2, 24, 8
    P, _ = _inputs(N, H, G, C)
    step = torch.tensor([5], dtype=torch.int64, device=dev)
    u = TS.slice_uniforms(11, step, 3, N, H, G)
    Pu = dict(P, u=u.cpu())
    drawn = _hip(P, dev, N, H, G, C, u_given=False, seed=11, step=step, layer=3)
    fed = _hip(Pu, dev, N, H, G, C, u_given=True)
    assert all(torch.equal(x, y) for x, y in zip(drawn, fed))              # null u == fed the stream's values, bit for bit (backward too)
    assert torch.equal(u, TS.slice_uniforms(11, step, 3, N, H, G))
    assert not torch.equal(u, TS.slice_uniforms(11, step + 1, 3, N, H, G))
    assert not torch.equal(u, TS.slice_uniforms(11, step, 4, N, H, G))
    assert not torch.equal(u, TS.slice_uniforms(12, step, 3, N, H, G))
    assert torch.equal(u[:100], TS.slice_uniforms(11, step, 3, 100, H, G))  # a function of the index, not of the launch geometry
    big = TS.slice_uniforms(11, step, 0, 15625, 2, 32).double().flatten()  # 10^6 draws
    n = big.numel()
    assert n == 10 ** 6 and float(big.min()) >= 0.0 and float(big.max()) < 1.0
    m, v = float(big.mean()), float(big.var())
    se_m, se_v = (1 / 12 / n) ** 0.5, (1 / 180 / n) ** 0.5                 # var of (u - 1/2)^2 is 1/180
    print("mean", m, "var", v)
    assert abs(m - 0.5) < 5 * se_m and abs(v - 1 / 12) < 5 * se_v


def test_refused_sizes():
    L = _capi.lib()
    assert L.mgn_slice_uniforms(0, None, 0, 10, 2, 65, None, None) == 1
    assert b"mgn_slice_uniforms" in L.mgn_attn_last_error()
    assert L.mgn_slice_weights_fwd(None, 0, *([None] * 8), 0, None, 0, 10, 2, 65, 8, None, None, None) == 1
    assert b"mgn_slice_weights_fwd" in L.mgn_attn_last_error()
    assert L.mgn_slice_aggregate(None, None, 0, 10, 2, 8, 0, None, None, None, 0, None) == 1
    assert b"mgn_slice_aggregate" in L.mgn_attn_last_error()
    assert L.mgn_slice_expand(None, None, 10, 2, 65, 8, None, 0, None) == 1
    assert b"mgn_slice_expand" in L.mgn_attn_last_error()
    assert L.mgn_slice_rows_bwd(None, 0, *([None] * 4), 0, *([None] * 8), 0, None, 0, 10, 2, 8, 0, None, 0, *([None] * 7), 0, None) == 1
    assert b"mgn_slice_rows_bwd" in L.mgn_attn_last_error()


def test_no_rows_is_no_error(dev):
    """N = 0: an empty tensor has no address, so the row-sized pointers are null; every launch returns 0 and the reductions write zeros"""
    L = _capi.lib()
    H, G, C = 2, 8, 8
    f = dict(dtype=torch.float32, device=dev)
    small = [torch.ones(n, **f) for n in (G * C, G, G * C, G, G, 1, H)]          # Ws, bs, W1, b1, w2, b2, bias
    sp = [t.data_ptr() for t in small]
    tok, dS, dnorm = torch.ones(H, G, C, **f), torch.ones(H, G, C, **f), torch.ones(H, G, **f)
    S, norm = torch.ones(H, G, C, **f), torch.ones(H, G, **f)
    dw2, db2, dbias = torch.ones(G, **f), torch.ones(1, **f), torch.ones(H, **f)
    assert L.mgn_slice_uniforms(0, None, 0, 0, H, G, None, None) == 0
    assert L.mgn_slice_weights_fwd(None, H * C, *sp, None, 0, None, 0, 0, H, G, C, None, None, None) == 0
    assert L.mgn_slice_aggregate(None, None, H * C, 0, H, G, C, S.data_ptr(), norm.data_ptr(), None, 0, None) == 0
    assert L.mgn_slice_expand(None, tok.data_ptr(), 0, H, G, C, None, H * C, None) == 0
    assert L.mgn_slice_rows_bwd(None, H * C, tok.data_ptr(), dS.data_ptr(), dnorm.data_ptr(), None, H * C, None, None, *sp[:5], None, 0, None, 0,
                                0, H, G, C, None, H * C, None, None, None, dw2.data_ptr(), db2.data_ptr(), dbias.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in (S, norm, dw2, db2, dbias))


# ------------------------------------------------------------------------------------------- module and Engine
@pytest.fixture(scope="module")
def Z():
    return TR.load_golden()


@pytest.mark.parametrize("case", CASES)
def test_module_matches_the_reference(dev, Z, case):
    """Measured on an MI355X, worst error / bound: rope_gate 0.224, narrow 0.106, temporal 0.084, unified 0.295, clamp 0.599."""
    meta, T, state, g64, err = TR.unpack_case(Z, case)
    got = run(build(meta, state).to(dev), T, torch.float32, dev)
    compare(case + " HIP", got, T, g64, err)


def _mesh_graph(dev, n=300, seed=0):
    g = torch.Generator().manual_seed(seed)
    side = 20
    idx = torch.arange(n)
    e = torch.stack([idx[:-1], idx[1:]])
    e = torch.cat([e, e.flip(0)], dim=1)
    x = torch.randn(n, 3, generator=g)
    x[:, 2] = (torch.arange(n) % side == 0).float() * float(gp.NodeType.WALL_BOUNDARY)
    pos = torch.rand(n, 2, generator=g)
    return Graph(x=x.to(dev), y=torch.randn(n, 2, generator=g).to(dev), pos=pos.to(dev), edge_index=e.to(dev),
                 edge_attr=torch.randn(e.shape[1], 3, generator=g).to(dev))


def _as(batch, dev, dtype=torch.float32):
    cast = lambda t: t.to(dev, dtype) if t.is_floating_point() else t.to(dev)   # noqa: E731
    return Graph(**{k: cast(getattr(batch, k)) for k in ("x", "y", "pos", "edge_index", "edge_attr")})


def _step_grads(eng, batch):
    """(loss, gradients by name) of one training step's forward, loss and backward, BEFORE any clip or optimiser touches them"""
    eng.sim.train()
    node_type = batch.x[:, eng.sim.node_type_index]
    net_out, target, _ = eng.sim(batch)
    loss = eng._loss(batch, net_out, target, node_type)
    for p in eng.sim.parameters():
        p.grad = None
    loss.backward()
    return loss.detach(), {k: p.grad.detach().clone() for k, p in eng.sim.named_parameters() if p.grad is not None}


def test_engine_step_matches_the_cpu_torch_ops_path(dev):
    """300-node mesh.  The Engine's forward, loss and backward on the HIP kernels against the same Engine on the CPU torch-ops path fed
    mgn_slice_uniforms' values, PER TENSOR and before the clip: the reference of every tensor is the CPU Engine in fp64, its bound the
    larger of the convention (1e-5 for the loss, 2e-5 for a gradient) and 4 x the distance of the fp32 CPU Engine to that fp64 run.
    Then one whole train_step on both (clip and optimiser included): the same loss."""
    cfg = _config(slice_num=8)
    cpu = torch.device("cpu")
    torch.manual_seed(3)
    eng = harness.Engine(cfg, dev, seed=9)
    state = {k: v.cpu() for k, v in eng.sim.state_dict().items()}
    ref, ref64 = harness.Engine(cfg, cpu, seed=9), harness.Engine(cfg, cpu, seed=9)
    ref.sim.load_state_dict(state), ref64.sim.load_state_dict(state)
    ref64.sim.double()
    batch = _mesh_graph(dev)
    N, H, G = 300, 4, 8
    step0 = torch.zeros(1, dtype=torch.int64, device=dev)
    ref.model.noise_u = ref64.model.noise_u = [TS.slice_uniforms(9, step0, l, N, H, G).cpu() for l in range(2)]
    l_hip, g_hip = _step_grads(eng, batch)
    l_32, g_32 = _step_grads(ref, _as(batch, cpu))
    l_64, g_64 = _step_grads(ref64, _as(batch, cpu, torch.float64))
    assert l_64.dtype == torch.float64 and set(g_hip) == set(g_32) == set(g_64)
    worst = ("loss", rel_err(l_hip, l_64) / TR.bound(1e-5, rel_err(l_32, l_64)))
    assert worst[1] < 1
    for k in g_64:
        bd = TR.bound(2e-5, rel_err(g_32[k], g_64[k]))
        e = rel_err(g_hip[k], g_64[k])
        if e / bd > worst[1]:
            worst = (k, e / bd)
        assert e < bd, f"{k}: {e:.3e} >= {bd:.3e}"
    print(f"Engine gradients, {len(g_64)} tensors: worst error / bound = {worst[1]:.3f} ({worst[0]})")
    eng.model.model._noise_step.zero_()                                     # the same noise again for the whole step
    la, lb = eng.train_step(batch), ref.train_step(_as(batch, cpu))
    print("loss", float(la), float(lb))
    assert abs(float(la) - float(lb)) < 1e-5 * abs(float(lb))


def test_rollout_replay_equals_eager(dev):
    eng = harness.Engine(_config(slice_num=8), dev, seed=1)
    frames = [_mesh_graph(dev, seed=s) for s in range(3)]
    for f in frames[1:]:
        f.edge_index, f.edge_attr, f.pos = frames[0].edge_index, frames[0].edge_attr, frames[0].pos
    eng.train_step(frames[0])
    eng.model.model._noise_step.fill_(100)
    eager = eng.rollout(frames, graph="off")
    eng.rollout(frames, graph="on")                                         # (captures; the warm-up and capture advance the counter)
    eng.model.model._noise_step.fill_(100)
    replay = eng.rollout(frames, graph="on")
    assert int(eng.model.model._noise_step) == 103
    assert all(torch.equal(a, b) for a, b in zip(eager, replay))
    again = eng.rollout(frames, graph="on")                                  # the counter went on: other noise, other frames
    assert not torch.equal(again[0], replay[0])
