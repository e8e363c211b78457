"""GPU: the training tail of csrc/mgn_prep.hip against float64 references built on the CPU from the fp32 inputs the kernels get.

  * ``mgn_clip_adamw_t`` / ``mgn_clip_adamw`` (harness.FusedClipAdamW): ONE step from a chosen state (moments and step counter
    written before the step, so an fp32 and an fp64 trajectory cannot drift apart) against ``clip_grad_norm_`` +
    ``torch.optim.AdamW`` in float64 -- six regimes, both forms, tensor sizes at the edges of OPT_CHUNK = 4096 and of the
    256-thread stride; more than 96 and more than 480 tensors; parameters without a gradient; a non-contiguous gradient;
  * ``k_gate_fwd`` / ``k_gate_bwd``, ``k_rope_gather`` / ``k_rope_scatter``, ``k_gather_rows`` / ``k_halo_unpack_add`` called
    directly through ``ops``.

Every bound is derived from the roundings the quantity takes (u = 2^-24, one fp32 rounding), never from what the kernel gave.
Hyper-parameters reach the kernels as C floats, so the references use the fp32-rounded lr, betas, eps, weight decay and max_norm
(1 - 0.9f differs from 0.1 by 2.4e-7, four roundings by itself).  Each test prints ``PREPTAIL <what> <largest error / bound>``
(``pytest -s`` shows them)."""
import numpy as np
import pytest
import torch

import recipe as R
from graph_physics_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # one fp32 rounding, relative
TINY = 2.0 ** -126      # smallest normal fp32


def _f32(x: float) -> float:
    """the value a C ``float`` argument holds"""
    return float(np.float32(x))


def _report(what: str, frac: float) -> float:
    print(f"PREPTAIL {what} {frac:.3f}")
    return frac


def _frac(err: torch.Tensor, bound: torch.Tensor) -> float:
    """largest err / bound; an element with bound 0 must have err 0 (reported as inf otherwise)"""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _ulp32(p: torch.Tensor) -> torch.Tensor:
    """spacing of fp32 at |p| (float64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(p.detach().cpu().numpy().astype(np.float32))).astype(np.float64))


# ====================================================================== fused clip + AdamW
BETAS, EPS = (0.9, 0.95), 1e-8
SIZES = [(1,), (255,), (257,), (4095,), (4096,), (4097,), (8193,), (128, 384)]

# grad scale, prior moments, step counter before, lr, weight decay, max_norm.
# ``noclip``: the sizes above hold 70 146 elements, so elements of scale 0.01 have norm 2.65 and WOULD be clipped at max_norm 1;
# the case exists for coefficient == 1 (asserted below), which needs the scale 1e-3 (norm 0.265).
CASES = {
    "noclip": dict(g=1e-3, prior=None, step0=0, lr=1e-3, wd=1e-4, max_norm=1.0),
    "clip": dict(g=10.0, prior=None, step0=0, lr=1e-3, wd=1e-4, max_norm=1.0),
    "decay": dict(g=0.01, prior=0.01, step0=9, lr=1e-2, wd=0.1, max_norm=1.0),
    "eps": dict(g=1e-8, prior=None, step0=0, lr=1e-3, wd=1e-4, max_norm=1.0),
    "late": dict(g=1.0, prior=1.0, step0=999, lr=1e-3, wd=1e-4, max_norm=0.0),
    "mixed": dict(g="mixed", prior="mixed", step0=4, lr=1e-3, wd=1e-4, max_norm=1.0),
}


def _draw(shape, scale, gen):
    z = torch.randn(*shape, generator=gen)
    if scale == "mixed":                                     # randn * 10^U(-6, 2): eight decades inside one tensor
        return z * torch.pow(10.0, torch.rand(*shape, generator=gen) * 8.0 - 6.0)
    return z * float(scale)


def _set_form(monkeypatch, form):
    if form == "chunked":
        monkeypatch.setenv("MGN_OPT_NO_TABLE", "1")
    else:
        monkeypatch.delenv("MGN_OPT_NO_TABLE", raising=False)


def _ref_step(p0, g0, m0, v0, step0, lr, wd, max_norm):
    """clip_grad_norm_ + torch.optim.AdamW in float64 over the tensors that have a gradient, state preloaded; every tensor gets the
    SAME step count (FusedClipAdamW keeps one counter).  Returns (norm, coef, {index: (p, g, m, v)})."""
    live = [i for i, g in enumerate(g0) if g is not None]
    q = {i: torch.nn.Parameter(p0[i].detach().cpu().double().clone()) for i in live}
    for i in live:
        q[i].grad = g0[i].detach().cpu().double().clone()
    mx = _f32(max_norm)
    if mx > 0:
        norm = float(torch.nn.utils.clip_grad_norm_([q[i] for i in live], mx, norm_type=2.0, foreach=False))
        coef = min(mx / (norm + 1e-6), 1.0)
    else:
        norm = float(torch.sqrt(sum((q[i].grad ** 2).sum() for i in live)))
        coef = 1.0
    ref = torch.optim.AdamW([q[i] for i in live], lr=_f32(lr), betas=(_f32(BETAS[0]), _f32(BETAS[1])), eps=_f32(EPS),
                            weight_decay=_f32(wd), foreach=False)
    for i in live:
        ref.state[q[i]] = {"step": torch.tensor(float(step0)), "exp_avg": m0[i].detach().cpu().double().clone(),
                           "exp_avg_sq": v0[i].detach().cpu().double().clone()}
    ref.step()
    out = {i: (q[i].detach(), q[i].grad, ref.state[q[i]]["exp_avg"], ref.state[q[i]]["exp_avg_sq"]) for i in live}
    assert all(float(ref.state[q[i]]["step"]) == step0 + 1 for i in live)
    return norm, coef, out


def _check_step(tag, params, opt, p0, g0, m0, v0, step0, lr, wd, max_norm):
    """the assertions of one optimiser step.  p0 / g0 / m0 / v0: fp32 CPU tensors as they were BEFORE the step (g0[i] None: no
    gradient).  Returns (norm, coef) of the reference."""
    norm, coef, ref = _ref_step(p0, g0, m0, v0, step0, lr, wd, max_norm)
    assert float(opt.step_t) == step0 + 1
    # norm: non-negative terms; longest chain 16 fmas + 8 tree levels + ceil(parts / 256) + 8 levels ~ 40 roundings; sqrt halves
    norm_gpu = float(opt.norm_t)
    f_norm = _report(f"{tag} norm", abs(norm_gpu - norm) / norm / 2e-6)
    assert f_norm < 1.0, f"{tag}: norm {norm_gpu!r} vs {norm!r}"
    b1, b2 = _f32(BETAS[0]), _f32(BETAS[1])
    fr = dict(g=0.0, m=0.0, v=0.0, p=0.0)
    changed = False
    for i, (p_r, g_r, m_r, v_r) in ref.items():
        g_gpu = params[i].grad.detach().cpu()
        changed = changed or not torch.equal(g_gpu, g0[i])
        g_gpu, m_gpu, v_gpu = g_gpu.double(), opt.exp_avg[i].cpu().double(), opt.exp_avg_sq[i].cpu().double()
        p_gpu = params[i].detach().cpu().double()
        fr["g"] = max(fr["g"], _frac((g_gpu - g_r).abs(), 4 * U * g_r.abs()))
        # the two summands cancel: absolute against their magnitudes
        fr["m"] = max(fr["m"], _frac((m_gpu - m_r).abs(), 4 * U * (b1 * m0[i].double().abs() + (1 - b1) * g_r.abs())))
        fr["v"] = max(fr["v"], _frac((v_gpu - v_r).abs(), 8 * U * v_r.abs()))
        # p is rounded twice (decay product, subtraction); the step itself carries a handful of fp32 roundings
        delta = p_r - p0[i].double()
        fr["p"] = max(fr["p"], _frac((p_gpu - p_r).abs(), 2 * _ulp32(p0[i]).reshape(p_r.shape) + 8e-6 * delta.abs()))
    for k in ("g", "m", "v", "p"):
        _report(f"{tag} {k}", fr[k])
    assert changed == (coef < 1.0), f"{tag}: gradients {'changed' if changed else 'unchanged'} but the reference coefficient is {coef}"
    assert fr["g"] <= 1.0, f"{tag}: clipped gradients {fr['g']:.3f} of the bound"
    assert fr["m"] <= 1.0, f"{tag}: exp_avg {fr['m']:.3f} of the bound"
    assert fr["v"] < 1.0, f"{tag}: exp_avg_sq {fr['v']:.3f} of the bound"
    assert fr["p"] <= 1.0, f"{tag}: parameters {fr['p']:.3f} of the bound"
    return norm, coef


def _make(dev, shapes, gen, lr, wd, max_norm, g_scale, prior=None, step0=0):
    """parameters ~ N(0,1), gradients and prior state on the CPU (fp32) and a FusedClipAdamW holding that state on ``dev``"""
    from graph_physics_amd import harness

    p0 = [torch.randn(*s, generator=gen) for s in shapes]
    g0 = [_draw(s, g_scale, gen) for s in shapes]
    if prior is None:
        m0, v0 = [torch.zeros(*s) for s in shapes], [torch.zeros(*s) for s in shapes]
    else:
        m0, v0 = [_draw(s, prior, gen) for s in shapes], [_draw(s, prior, gen) ** 2 for s in shapes]
    params = [torch.nn.Parameter(p.clone().to(dev)) for p in p0]
    opt = harness.FusedClipAdamW(params, lr, betas=BETAS, eps=EPS, weight_decay=wd, max_norm=max_norm)
    for i in range(len(shapes)):
        opt.exp_avg[i].copy_(m0[i])
        opt.exp_avg_sq[i].copy_(v0[i])
    opt.step_t.fill_(float(step0))
    for p, g in zip(params, g0):
        p.grad = g.clone().to(dev)
    return params, opt, p0, g0, m0, v0


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("form", ["table", "chunked"])
def test_one_adamw_step_from_a_chosen_state(dev, monkeypatch, form, case):
    """one step of either form against float64 clip_grad_norm_ + AdamW preloaded with the same moments and step count: norm,
    clipped gradients, both moments, parameters, step counter; and the case is in the regime it is named after"""
    c = CASES[case]
    _set_form(monkeypatch, form)
    gen = torch.Generator().manual_seed(11 + list(CASES).index(case))
    params, opt, p0, g0, m0, v0 = _make(dev, SIZES, gen, c["lr"], c["wd"], c["max_norm"], c["g"], c["prior"], c["step0"])
    opt.step()
    assert (opt._table is not None) == (form == "table")
    norm, coef = _check_step(f"{case}/{form}", params, opt, p0, g0, m0, v0, c["step0"], c["lr"], c["wd"], c["max_norm"])
    if case == "clip":
        assert coef < 0.1
    if case == "noclip":
        assert coef == 1.0
    if case == "decay":
        allp = torch.cat([p.reshape(-1) for p in p0])
        assert float((_f32(c["lr"]) * _f32(c["wd"]) * allp.double().abs() / _ulp32(allp)).median()) > 1000
    if case == "eps":
        r = float(torch.cat([g.reshape(-1) for g in g0]).double().abs().median()) / _f32(EPS)
        assert 0.1 < r < 10


@pytest.mark.parametrize("n,form", [(500, "chunked"), (200, "table")])
def test_adamw_step_over_more_tensors_than_one_launch_holds(dev, monkeypatch, n, form):
    """500 tensors: over the table form's 480, so FusedClipAdamW itself falls back to the chunked form (six launches of each kernel);
    200 tensors: table form, more than one chunked launch would hold.  Clipping is active, so a partial dropped at a launch
    boundary shows in the norm and in every clipped gradient."""
    monkeypatch.delenv("MGN_OPT_NO_TABLE", raising=False)
    shapes = [[(1,), (3, 5), (128,), (4097,)][i % 4] for i in range(n)]
    gen = torch.Generator().manual_seed(n)
    params, opt, p0, g0, m0, v0 = _make(dev, shapes, gen, 1e-3, 1e-4, 1.0, 10.0)
    opt.step()
    assert (opt._table is None) == (form == "chunked")
    norm, coef = _check_step(f"{n}-tensors/{form}", params, opt, p0, g0, m0, v0, 0, 1e-3, 1e-4, 1.0)
    assert coef < 0.1
    want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g0)))        # over all n tensors
    assert abs(float(opt.norm_t) - want) / want < 2e-6


@pytest.mark.parametrize("form", ["table", "chunked"])
def test_adamw_parameters_without_a_gradient(dev, monkeypatch, form):
    """three steps over 12 parameters: two have no gradient on step 2 only, one never has.  A parameter without a gradient keeps p,
    m and v bit for bit; the norm is over the live gradients; the device table is rebuilt when the live set changes; the live
    parameters meet the one-step bounds (the float64 reference is reloaded from the device state before each step).

    PINNED, not endorsed: FusedClipAdamW keeps ONE step counter.  A parameter that skipped a step (or joins late) takes the global
    count in its bias corrections, where torch.optim.AdamW would use the parameter's own count; the reference below is therefore
    given the global count for every live parameter.

    Parameter 0's gradient is a column slice of a wider tensor (non-contiguous): after the step ``.grad`` is contiguous and holds
    the clipped values."""
    from graph_physics_amd import harness

    _set_form(monkeypatch, form)
    shapes = [(16, 24), (5,), (300,), (4097,)] * 3
    gen = torch.Generator().manual_seed(5)
    p_init = [torch.randn(*s, generator=gen) for s in shapes]
    params = [torch.nn.Parameter(p.clone().to(dev)) for p in p_init]
    lr, wd, mx = 1e-3, 1e-4, 1.0
    opt = harness.FusedClipAdamW(params, lr, betas=BETAS, eps=EPS, weight_decay=wd, max_norm=mx)
    never, skip2 = 11, (3, 7)
    keys = []
    for step in (1, 2, 3):
        dead = {never} | (set(skip2) if step == 2 else set())
        p0 = [p.detach().cpu().clone() for p in params]
        m0, v0 = [m.cpu().clone() for m in opt.exp_avg], [v.cpu().clone() for v in opt.exp_avg_sq]
        g0 = [None if i in dead else torch.randn(*s, generator=gen) for i, s in enumerate(shapes)]
        for i, p in enumerate(params):
            p.grad = None if g0[i] is None else g0[i].clone().to(dev)
        wide = torch.zeros(16, 32)
        wide[:, :24] = g0[0]
        params[0].grad = wide.to(dev)[:, :24]
        assert not params[0].grad.is_contiguous()
        opt.step()
        assert params[0].grad.is_contiguous()
        keys.append(opt._table_key)
        norm, coef = _check_step(f"nograd/{form}/step{step}", params, opt, p0, g0, m0, v0, step - 1, lr, wd, mx)
        assert coef < 0.1          # clipping is active: .grad holds clipped values, checked against the reference above
        for i in dead:
            assert params[i].grad is None
            assert torch.equal(params[i].detach().cpu(), p0[i]) and torch.equal(opt.exp_avg[i].cpu(), m0[i])
            assert torch.equal(opt.exp_avg_sq[i].cpu(), v0[i])
    assert torch.equal(opt.exp_avg[never].cpu(), torch.zeros(shapes[never])) and torch.equal(params[never].detach().cpu(), p_init[never])
    if form == "table":
        assert keys[0] != keys[1] and keys[1] != keys[2]
        assert len(keys[0]) == 11 and len(keys[1]) == 9 and len(keys[2]) == 11
    else:
        assert opt._table is None


# ====================================================================== gate
def _gate_inputs(N, H, seed):
    gen = torch.Generator().manual_seed(seed)
    G = torch.randn(N, H, generator=gen)
    flat = G.view(-1)
    k = torch.arange(flat.numel())
    for r, val in enumerate((100.0, -100.0, 20.0, -20.0)):       # a quarter of the logits, a sixteenth each
        flat[k % 16 == r] = val
    phi = torch.randn(N, generator=gen)
    gate_pos = torch.randn(H, generator=gen)
    agg = torch.randn(N, H, generator=gen)
    d = torch.randn(N, H, generator=gen)
    return G, phi, gate_pos, agg, d


@pytest.mark.parametrize("with_phi", [False, True])
@pytest.mark.parametrize("N,H", [(1, 1), (37, 6), (257, 128), (1000, 33)])
def test_gate_kernels_vs_fp64(dev, N, H, with_phi):
    """k_gate_fwd (training and inference form) and k_gate_bwd against float64, logits of +-100 and +-20 among unit-scale ones.

    Bounds.  gate: 4u relative below 0.5 (expf within an ulp = 2u, the addition, the division), the same absolute on 1 - gate
    elsewhere.  Two things the fp32 formats add to that, both worked out before any run:
      * with phi the LOGIT is computed, fl(G + phi * gate_pos): one rounding of the product and one of the sum, at most
        u * (|phi * gate_pos| + |logit|) on the logit, and d gate = gate (1 - gate) d logit -- at a logit of -20 that alone is
        20u relative.  Without phi the logit is an input and the term is absent.
      * below the smallest normal fp32 (2^-126) a relative bound has no meaning: expf(100) is inf, so the gate at -100 is exactly 0
        (asserted) where float64 has 3.7e-44.  The bounds carry that floor.
    agg_out, dAgg: 6u relative (plus the two terms above for agg_out).  dG: 8u |d agg| max(gate (1 - gate), 2^-24) absolute.
    The backward kernel's reference is formed from the fp32 gate it is given (the forward kernel's output)."""
    assert (N * H) % 256 != 0                                        # a partial last block in every shape
    G, phi, gate_pos, agg, d = _gate_inputs(N, H, 100 * N + H)
    Gd, aggd, dd = G.to(dev), agg.to(dev), d.to(dev)
    phid, gpd = (phi.to(dev), gate_pos.to(dev)) if with_phi else (None, None)
    gate, agg_out = torch.full((N, H), float("nan"), device=dev), torch.full((N, H), float("nan"), device=dev)
    ops.gate_fwd(Gd, phid, gpd, aggd, gate, agg_out)
    agg_inf = torch.full((N, H), float("nan"), device=dev)
    ops.gate_fwd(Gd, phid, gpd, aggd, None, agg_inf)                 # the inference form: no gate stored
    assert torch.equal(agg_inf, agg_out)
    dAgg, dG = torch.full((N, H), float("nan"), device=dev), torch.full((N, H), float("nan"), device=dev)
    ops.gate_bwd(dd, aggd, gate, dAgg, dG)
    alias, dG2 = dd.clone(), torch.full((N, H), float("nan"), device=dev)
    ops.gate_bwd(alias, aggd, gate, alias, dG2)                      # dAgg may alias dAggG (mgn_hip.h)
    assert torch.equal(alias, dAgg) and torch.equal(dG2, dG)
    gate, agg_out, dAgg, dG = gate.cpu(), agg_out.cpu(), dAgg.cpu(), dG.cpu()
    for t in (gate, agg_out, dAgg, dG):
        assert bool(torch.isfinite(t).all())

    extra = (phi.double()[:, None] * gate_pos.double()[None, :]) if with_phi else torch.zeros(N, H, dtype=torch.float64)
    logit = G.double() + extra
    g_ref = torch.sigmoid(logit)
    one_m = torch.sigmoid(-logit)                                    # 1 - gate without cancellation
    dlogit = U * (extra.abs() + logit.abs()) if with_phi else torch.zeros_like(logit)
    low = g_ref < 0.5
    err_g = (gate.double() - g_ref).abs()
    b_low = 4 * U * g_ref + dlogit * g_ref * one_m + TINY
    b_high = 4 * U + dlogit * g_ref * one_m                          # |(1 - gate) - (1 - gate_ref)| = |gate - gate_ref|
    tag = f"gate N={N} H={H} phi={int(with_phi)}"
    f_gate = _report(f"{tag} gate", _frac(err_g, torch.where(low, b_low, b_high)))
    a64 = agg.double()
    f_agg = _report(f"{tag} agg_out", _frac((agg_out.double() - a64 * g_ref).abs(),
                                            a64.abs() * (6 * U * g_ref + dlogit * g_ref * one_m + TINY) + TINY))
    gt = gate.double()                                               # what the backward kernel was given
    f_dagg = _report(f"{tag} dAgg", _frac((dAgg.double() - d.double() * gt).abs(), 6 * U * (d.double() * gt).abs() + TINY))
    f_dg = _report(f"{tag} dG", _frac((dG.double() - d.double() * a64 * gt * (1 - gt)).abs(),
                                      8 * U * (d.double() * a64).abs() * torch.clamp(gt * (1 - gt), min=U)))
    assert f_gate <= 1.0 and f_agg <= 1.0 and f_dagg <= 1.0 and f_dg <= 1.0, (f_gate, f_agg, f_dagg, f_dg)
    hi, lo = G == 100.0, G == -100.0
    if N * H >= 2:
        assert bool(hi.any()) and bool(lo.any())
    assert bool((gate[hi] == 1.0).all()) and bool((gate[lo] == 0.0).all())
    assert bool((dG[hi] == 0.0).all()) and bool((dG[lo] == 0.0).all())


# ====================================================================== RoPE
ROPE_N, ROPE_E, ROPE_HUB = 300, 2500, 7
_rope_cache = {}


def _rope_topology(dev):
    """300 nodes, 2500 edges with duplicates and self loops; node 7 is a hub of out-degree >= 300; nodes 10..12 and 299 have no
    outgoing edge.  Built once and left unchanged."""
    if "topo" not in _rope_cache:
        ei = R.random_graph(ROPE_N, ROPE_E, 17).clone()
        ei[0, 100:400] = ROPE_HUB
        for n in (10, 11, 12):
            ei[0][ei[0] == n] = 13
        topo = ops.Topology(ei.to(dev), ROPE_N)
        src, dst = topo.src_s.cpu().long(), topo.dst_s.cpu().long()
        key = lambda s, t: torch.sort(s * ROPE_N + t).values
        assert torch.equal(key(src, dst), key(ei[0], ei[1]))         # the kernel's edge list is the input's, reordered
        deg = torch.bincount(src, minlength=ROPE_N)
        assert int(deg[ROPE_HUB]) >= 300 and int((deg == 0).sum()) >= 4 and bool((src == dst).any())
        _rope_cache["topo"] = (topo, src, dst, deg)
    return _rope_cache["topo"]


def _rope_rotate(v, theta, pc, axes, sign):
    """float64: rotate the first 2 * pc * axes channels of v [E, H] pairwise by sign * theta [E, axes * pc]; the rest pass through"""
    out = v.clone()
    nrot = 2 * pc * axes
    ev, od = v[:, 0:nrot:2], v[:, 1:nrot:2]
    cs, sn = torch.cos(theta), sign * torch.sin(theta)
    out[:, 0:nrot:2] = ev * cs - od * sn
    out[:, 1:nrot:2] = ev * sn + od * cs
    return out


def _pair_norm(t):
    """[R, H] -> [R, H / 2]: 2-norm of each channel pair"""
    return torch.sqrt(t[:, 0::2] ** 2 + t[:, 1::2] ** 2)


@pytest.mark.parametrize("scale", [1.0, 500.0])
@pytest.mark.parametrize("base", [100.0, 10000.0])
@pytest.mark.parametrize("H,axes,pos_w", [(128, 3, 3), (16, 3, 3), (64, 2, 3), (32, 1, 2)])
def test_rope_kernels_vs_fp64(dev, H, axes, pos_w, base, scale):
    """k_rope_gather and k_rope_scatter against a float64 rotation by theta = (pos[src] - pos[dst])[axis] * inv_freq[i] formed in
    float64 from the fp32 inputs.  The kernel rounds the difference and the product once each, so its angle is off by at most
    2u |theta|; sinf / cosf and the two products and the sum of each output add a few roundings:
        per pair  ||out_gpu - out_ref|| <= (2u |theta| + 6u) ||(v.x, v.y)||.
    Scatter: the sum of the per-edge bounds plus deg * u * (||resid|| + sum ||T_k||) for the accumulation (every partial sum,
    which starts from the residual row, is bounded by that sum).  Pass-through channels bit for bit; rows without an outgoing edge
    equal the residual (or zero) exactly; two runs identical; <gather(x), T> == <x, scatter(T)> on the device results."""
    topo, src, dst, deg = _rope_topology(dev)
    pc = H // (2 * axes)
    nrot = 2 * pc * axes
    gen = torch.Generator().manual_seed(H + axes + int(base) + int(scale))
    pos = torch.rand(ROPE_N, pos_w, generator=gen) * scale
    inv_freq = torch.pow(torch.tensor(base), -torch.arange(pc, dtype=torch.float32) / float(pc))
    x = torch.randn(ROPE_N, H, generator=gen)
    T = torch.randn(ROPE_E, H, generator=gen)
    resid = torch.randn(ROPE_N, H, generator=gen)
    posd, invd, xd, Td, residd = pos.to(dev), inv_freq.to(dev), x.to(dev), T.to(dev), resid.to(dev)

    delta = pos.double()[src][:, :axes] - pos.double()[dst][:, :axes]                       # [E, axes]
    theta = (delta[:, :, None] * inv_freq.double()[None, None, :]).reshape(ROPE_E, axes * pc)
    per_pair = torch.cat([2 * U * theta.abs() + 6 * U, torch.zeros(ROPE_E, H // 2 - axes * pc, dtype=torch.float64)], dim=1)
    tag = f"rope H={H} axes={axes} base={int(base)} scale={int(scale)}"
    if scale > 1:
        assert float(theta.abs().max()) > 300
    else:
        assert float(theta.abs().max()) < 2

    # ---- gather
    out = torch.full((ROPE_E, H), float("nan"), device=dev)
    ops.rope_gather(xd, posd, invd, topo, axes, out)
    out = out.cpu()
    xs = x[src]
    assert torch.equal(out[:, nrot:], xs[:, nrot:])
    ref = _rope_rotate(xs.double(), theta, pc, axes, 1.0)
    f_g = _report(f"{tag} gather", _frac(_pair_norm(out.double() - ref)[:, : axes * pc], (per_pair * _pair_norm(xs.double()))[:, : axes * pc]))
    assert f_g <= 1.0

    # ---- scatter, with and without the residual
    edge_bound = per_pair * _pair_norm(T.double())                                           # [E, H/2]
    refT = _rope_rotate(T.double(), theta, pc, axes, -1.0)
    sum_ref = torch.zeros(ROPE_N, H, dtype=torch.float64).index_add_(0, src, refT)
    sum_bound = torch.zeros(ROPE_N, H // 2, dtype=torch.float64).index_add_(0, src, edge_bound)
    sum_norm = torch.zeros(ROPE_N, H // 2, dtype=torch.float64).index_add_(0, src, _pair_norm(T.double()))
    res = {}
    for with_resid in (False, True):
        o1, o2 = torch.full((ROPE_N, H), float("nan"), device=dev), torch.full((ROPE_N, H), float("nan"), device=dev)
        ops.rope_scatter(Td, posd, invd, topo, axes, residd if with_resid else None, o1)
        ops.rope_scatter(Td, posd, invd, topo, axes, residd if with_resid else None, o2)
        assert torch.equal(o1, o2)
        o1 = o1.cpu()
        r0 = resid if with_resid else torch.zeros(ROPE_N, H)
        assert torch.equal(o1[deg == 0], r0[deg == 0])
        bound = sum_bound + deg.double()[:, None] * U * (sum_norm + _pair_norm(r0.double()))
        f_s = _report(f"{tag} scatter resid={int(with_resid)}", _frac(_pair_norm(o1.double() - (r0.double() + sum_ref))[deg > 0], bound[deg > 0]))
        assert f_s <= 1.0
        res[with_resid] = o1
    a = float((out.double() * T.double()).sum())
    b = float((x.double() * res[False].double()).sum())
    _report(f"{tag} adjoint", abs(a - b) / max(abs(a), abs(b)) / 1e-5)
    assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (a, b)


# ====================================================================== halo rows
@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("H", [4, 128, 132])
def test_gather_rows_is_an_exact_row_copy(dev, H, n):
    """16-byte lanes, H / 4 per row: lane counts below, across and (1000 x 128) exactly filling 256-thread blocks"""
    gen = torch.Generator().manual_seed(n + H)
    src = torch.randn(400, H, generator=gen)
    idx = torch.randint(0, 400, (n,), generator=gen, dtype=torch.int32)       # repeated (1000 of 400) and out of order
    idx[-1] = idx[0]
    if n > 2:
        idx[1], idx[2] = 399, 0
    out = torch.full((n + 1, H), float("nan"), device=dev)
    got = ops.gather_rows(src.to(dev), idx.to(dev), out[:n])
    assert torch.equal(got.cpu(), src[idx.long()])
    assert bool(torch.isnan(out[n]).all())                                       # nothing written past the last row


@pytest.mark.parametrize("H", [4, 132])
def test_halo_unpack_add_sums_in_ascending_order(dev, H):
    """200 destination nodes among 500 rows, ragged groups (empty ones, groups of one, one of 50), a random permutation of the packed
    rows.  The kernel does plain fp32 adds in ascending k from the old dst row, so the sequential fp32 sum on the CPU is exact; it
    is also within deg * u * sum |terms| of the float64 sum.  Rows not listed are untouched."""
    rng = np.random.default_rng(H)
    n_nodes, n_rows = 200, 500
    degs = rng.integers(0, 7, size=n_nodes)
    degs[[0, 5, 199]] = 0
    degs[[1, 6, 198]] = 1
    degs[100] = 50
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    total = int(rowptr[-1])
    perm = rng.permutation(total).astype(np.int32)
    nodes = rng.permutation(n_rows)[:n_nodes].astype(np.int32)                   # distinct, out of order
    gen = torch.Generator().manual_seed(H)
    rows = torch.randn(total, H, generator=gen)
    dst0 = torch.randn(n_rows, H, generator=gen)
    dst = dst0.clone().to(dev)
    ops.halo_unpack_add(rows.to(dev), torch.from_numpy(nodes).to(dev), torch.from_numpy(rowptr).to(dev), torch.from_numpy(perm).to(dev), dst)
    dst = dst.cpu()
    listed = torch.zeros(n_rows, dtype=torch.bool)
    listed[torch.from_numpy(nodes).long()] = True
    assert torch.equal(dst[~listed], dst0[~listed])
    nd = torch.from_numpy(nodes).long()
    acc32, acc64, mag = dst0[nd].clone(), dst0[nd].double(), dst0[nd].double().abs()
    rp, pm, dg = torch.from_numpy(rowptr).long(), torch.from_numpy(perm).long(), torch.from_numpy(degs).long()
    for t in range(int(degs.max())):                                              # the t-th term of every group that has one
        has = dg > t
        term = rows[pm[rp[:-1][has] + t]]
        acc32[has] = acc32[has] + term
        acc64[has] = acc64[has] + term.double()
        mag[has] = mag[has] + term.double().abs()
    assert torch.equal(dst[nd], acc32)
    f = _report(f"halo_unpack_add H={H} vs fp64", _frac((dst[nd].double() - acc64).abs(), dg.double()[:, None] * U * mag))
    assert f <= 1.0
