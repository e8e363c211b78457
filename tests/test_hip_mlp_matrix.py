"""GPU: the generic MLP kernels (k_mlp_fwd / k_mlp_bwd<HB, MT, RAGGED>) and the routes of ops.MlpFunction against the
fp32 and fp64 oracles over the table of tests/mlp_cases.py: widths next to a multiple of 16, rows next to the tile edges,
2 .. 8 layers, ReLU / SiLU / GELU, processor blocks off the packed path, the two-tiles-per-wave instances, the bf16 matrix
mode, and the host-side behaviour around them.  tests/test_mlp_cases_host.py shows on the CPU that the references alone
sit inside half of every bar used here.

Bars: forward FWD_TOL in the three readings of conftest.assert_close3 against the fp64 oracle; SiLU / GELU gradients
GRAD_TOL against the fp64 oracle; ReLU gradients by the rule of test_hip_parity.py::test_mlp_forward_backward -- within
GRAD_TOL of the fp32 oracle, or as close to the fp64 oracle as the fp32 oracle is (x 1.25 + 1e-6), which only a flipped
mask can make necessary: at most one ReLU case in ten may need it and none with 65 rows or fewer (the last test counts)."""
import time

import pytest
import torch

import graph_physics_amd as gp
import mlp_cases as MC
from conftest import assert_close3, rel_err, rms_err
from graph_physics_amd import ops

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = MC.FWD_TOL, MC.GRAD_TOL

_t0 = [None]
_relu_cases, _second_branch = set(), set()
_worst, _routes = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _t0[0] = time.time()
    yield


def _note(fam, act, what, v):
    _worst[(fam, act, what)] = max(_worst.get((fam, act, what), 0.0), v)


def _check_grad(fam, c, what, hip, g32, g64):
    assert hip is not None and hip.shape == g64.shape, (c.name, what, None if hip is None else tuple(hip.shape))
    assert bool(torch.isfinite(hip).all()), (c.name, what)
    e64 = rel_err(hip, g64)
    _note(fam, c.act, "gradients", e64)
    if c.act != "relu":
        assert e64 < GRAD_TOL, (c.name, what, e64)
        return
    e32 = rel_err(hip, g32)
    if e32 < GRAD_TOL:
        return
    own = rel_err(g32, g64)
    print(f"second branch: {c.name} {what}: vs fp32 {e32:.2e}, vs fp64 {e64:.2e}, fp32 oracle vs fp64 {own:.2e}")
    _second_branch.add(c.name)
    assert e64 < 1.25 * own + 1e-6, (c.name, what, e32, e64, own)


def _check(fam, c, outs, grads, dins):
    """forward, every parameter gradient and the input gradient(s) of one run against the references"""
    r32, r64 = MC.reference(c.name, torch.float32), MC.reference(c.name, torch.float64)
    if c.act == "relu":
        _relu_cases.add(c.name)
    for i, (o, want) in enumerate(zip(outs, r64.out)):
        assert o.shape == want.shape
        r, _, _ = assert_close3(o, want, FWD_TOL, f"{c.name} forward[{i}]")
        _note(fam, c.act, "forward", r)
    assert set(grads) == set(r64.grads)
    for k in grads:
        _check_grad(fam, c, k, grads[k], r32.grads[k], r64.grads[k])
    for i, (d, d32, d64) in enumerate(zip(dins, r32.dins, r64.dins)):
        if d64 is None:
            assert d is None
        else:
            _check_grad(fam, c, f"input[{i}]", d, d32, d64)


def _same(a, b):
    outs_a, grads_a, dins_a = a
    outs_b, grads_b, dins_b = b
    ok = all(torch.equal(x, y) for x, y in zip(outs_a, outs_b)) and all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    return ok and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(dins_a, dins_b))


# ---------------------------------------------------------------------------------- A: stand-alone build_mlp
def _mlp_net(c, dev):
    p, x, cot = MC.mlp_inputs(c)
    net = gp.build_mlp(c.fin, c.H, c.fout, nb_of_layers=c.NL, layer_norm=c.norm, act=c.act).to(dev)
    net.load_state_dict(p)
    return net, x, cot


def _mlp_pass(net, c, x, cot, dev):
    """one forward + backward.  Input and cotangent are the leading rows of NaN-filled buffers; the cotangent goes to the
    kernel as the very tensor (``backward(gradient=)``)."""
    for q in net.parameters():
        q.grad = None
    xd = MC.padded(x.to(dev)).requires_grad_(c.wants_dx)
    out = net(xd)
    route = out.grad_fn.meta[8]
    out.backward(gradient=MC.padded(cot.to(dev)))
    grads = {k: v.grad for k, v in net.state_dict(keep_vars=True).items()}
    for k, v in net.state_dict(keep_vars=True).items():   # (a padded last layer included: its exact [fout, H] / [fout] shape)
        assert v.grad.shape == v.shape and v.grad.is_contiguous(), k
    return (out.detach(),), grads, (xd.grad,), route


@pytest.mark.parametrize("name", list(MC.FAMILY_A))
def test_build_mlp_vs_fp64(dev, name):
    c = MC.FAMILY_A[name]
    net, x, cot = _mlp_net(c, dev)
    *first, route = _mlp_pass(net, c, x, cot, dev)
    want = c.route if ops.X6_ENABLED else "generic"   # (MGN_FP32_MFMA: nothing is packed)
    assert route == want, (name, route, want)
    if c.H == 128:
        _routes[name] = route
    _check("A", c, *first)
    *second, _ = _mlp_pass(net, c, x, cot, dev)
    assert _same(first, second), name + ": a second forward + backward is not bit-identical"


# ------------------------------------------------------------------- B, C: processor blocks off the packed path
def _block(c, dev):
    p, ei, x, e, cx, ce = MC.block_inputs(c)
    gp.layers.set_use_silu_activation(c.act == "silu")
    try:
        blk = gp.GraphNetBlock(c.H, nb_of_layers=c.NL).to(dev)
    finally:
        gp.layers.set_use_silu_activation(False)
    blk.load_state_dict(p)
    return blk, ei.to(dev), [t.to(dev) for t in (x, e, cx, ce)]


def _block_pass(blk, eid, ts):
    for q in blk.parameters():
        q.grad = None
    x, e, cx, ce = ts
    xd, ed = MC.padded(x).requires_grad_(True), MC.padded(e).requires_grad_(True)
    x2, e2 = blk(xd, eid, ed)
    torch.autograd.backward([x2, e2], [MC.padded(cx), MC.padded(ce)])
    return (x2.detach(), e2.detach()), {k: v.grad for k, v in blk.state_dict(keep_vars=True).items()}, (xd.grad, ed.grad)


@pytest.mark.parametrize("name", list(MC.FAMILY_B))
def test_block_off_the_packed_path_vs_fp64(dev, name):
    c = MC.FAMILY_B[name]
    blk, eid, ts = _block(c, dev)
    first = _block_pass(blk, eid, ts)
    _check("B", c, *first)
    assert _same(first, _block_pass(blk, eid, ts)), name + ": a second forward + backward is not bit-identical"


@pytest.mark.parametrize("name", list(MC.FAMILY_C))
def test_block_two_tiles_per_wave_vs_fp64(dev, name):
    """E and N above 131072: the edge and the node launches take the MT = 2 instances of the full-width generic kernels
    (forward with three / two gathered phases; backward with the dOut2 / idx2 add and din_resid), last tile ragged in rows"""
    c = MC.FAMILY_C[name]
    blk, eid, ts = _block(c, dev)
    first = _block_pass(blk, eid, ts)
    _check("C", c, *first)
    assert _same(first, _block_pass(blk, eid, ts)), name + ": a second forward + backward is not bit-identical"


# ------------------------------------------------------------------------------------------ D: bf16 matrix mode
@pytest.mark.parametrize("name", list(MC.FAMILY_D))
def test_build_mlp_bf16_mode(dev, name):
    """Forward against the explicit fp64 restatement of the mode (mlp_cases.bf16_explicit_forward); the distance between
    that and O.bf16_mixed() is what rounding decisions cost, and the engine gets twice it (on rel_err no less than one bf16
    ulp at the tensor's scale, 4e-3).  Gradients by the rule of test_hip_configs.py, against the mixed oracle."""
    c = MC.FAMILY_D[name]
    net, x, cot = _mlp_net(c, dev)
    ops.set_matrix_precision("bf16")
    try:
        (out,), grads, (dx,), route = _mlp_pass(net, c, x, cot, dev)
        torch.cuda.synchronize()
    finally:
        ops.set_matrix_precision("fp32")
    assert route == "generic"
    explicit = MC.bf16_explicit_forward(name)
    mixed, r32 = MC.reference(name, torch.float32, True), MC.reference(name, torch.float32)
    d_rel, d_rms = rel_err(mixed.out[0], explicit), rms_err(mixed.out[0], explicit)
    e_rel, e_rms = rel_err(out, explicit), rms_err(out, explicit)
    print(f"bf16 {name}: references apart rel {d_rel:.2e} rms {d_rms:.2e}; engine from the explicit one rel {e_rel:.2e} rms {e_rms:.2e}")
    assert rel_err(out, r32.out[0]) > 1e-5, "the bf16 mode was not taken"
    assert e_rel <= max(2.0 * d_rel, 4e-3), (name, e_rel, d_rel)
    assert e_rms <= 2.0 * d_rms, (name, e_rms, d_rms)
    worst = 0.0
    for k, g in grads.items():
        a, b, f32 = g.detach().double().cpu(), mixed.grads[k].double(), r32.grads[k].double()
        gap = float((b - f32).norm() / f32.norm())
        err = float((a - b).norm() / b.norm())
        worst = max(worst, err)
        assert err < max(1.5 * gap, 0.03), (name, k, err, gap)
    if c.wants_dx:
        b, f32 = mixed.dins[0].double(), r32.dins[0].double()
        gap, err = float((b - f32).norm() / f32.norm()), float((dx.double().cpu() - b).norm() / b.norm())
        assert err < max(1.5 * gap, 0.03), (name, "input", err, gap)
    _note("D", c.act, "forward (vs explicit, rel)", e_rel)
    _note("D", c.act, "gradients (vs mixed, norm-relative)", worst)


# ------------------------------------------------------------------------------------- host side, on the device
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("fin,H,fout,norm", [(11, 32, 3, False), (128, 128, 128, True)], ids=["generic", "packed"])
def test_no_rows(dev, fin, H, fout, norm, act):
    """M = 0: an empty result, zero gradients of the parameters' shapes, an empty input gradient"""
    net = gp.build_mlp(fin, H, fout, layer_norm=norm, act=act).to(dev)
    x = torch.empty(0, fin, device=dev).requires_grad_(fin == H)
    out = net(x)
    assert out.shape == (0, fout)
    out.backward(gradient=torch.empty(0, fout, device=dev))
    for k, v in net.state_dict(keep_vars=True).items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().max()) == 0.0, k
    if fin == H:
        assert x.grad.shape == (0, H)


def test_input_gradient_of_a_narrow_input_is_refused(dev):
    net = gp.build_mlp(11, 32, 32).to(dev)
    x = torch.randn(20, 11, device=dev).requires_grad_(True)
    out = net(x)
    with pytest.raises(NotImplementedError, match="ragged-width MLP input"):
        out.sum().backward()


@pytest.mark.parametrize("fin,H", [(32, 32), (128, 128)], ids=["generic", "packed"])
def test_second_backward_is_refused(dev, fin, H):
    net = gp.build_mlp(fin, H, H).to(dev)
    out = net(torch.randn(20, fin, device=dev))
    cot = torch.ones_like(out)
    out.backward(gradient=cot, retain_graph=True)
    with pytest.raises(RuntimeError, match="no saved activations"):
        out.backward(gradient=cot)


def test_depth_above_eight_is_refused(dev):
    x = torch.randn(20, 32, device=dev)
    y = gp.build_mlp(32, 32, 32, nb_of_layers=8).to(dev)(x)
    assert y.shape == (20, 32) and bool(torch.isfinite(y).all())
    with pytest.raises(AssertionError, match="at most 8 layers"):
        gp.build_mlp(32, 32, 32, nb_of_layers=9).to(dev)(x)


def test_report_and_relu_second_branch_budget():
    """the figures of this file (pytest -s) and the budget of ReLU cases that needed the fp64 branch; last in file order"""
    for (fam, act, what), v in sorted(_worst.items()):
        print(f"worst engine error  family {fam}  {act:4s}  {what:36s} {v:.2e}")
    for name, route in _routes.items():
        print(f"route {route:8s} {name}")
    print(f"ReLU cases on the second branch: {len(_second_branch)} of {len(_relu_cases)} {sorted(_second_branch)}")
    print(f"wall time of this file so far: {time.time() - _t0[0]:.1f} s")
    small = [n for n in _second_branch if n in MC.FAMILY_A and MC.FAMILY_A[n].M <= 65]
    assert not small, small
    assert 10 * len(_second_branch) <= len(_relu_cases), (sorted(_second_branch), len(_relu_cases))
