"""GPU: ``Engine.validate``, ``make_prediction`` and ``rollout`` with ``use_previous_data`` on the trajectory and the golden
normaliser state of ``test_rollout_vs_golden`` (3 rounds of latent 128, 96 nodes, 5 frames).

Bounds.  Predictions of the validation loop against ``rollout`` and of the captured step against the eager one: equality of
bits.  Metrics against fp64 sums over the predictions the loop returned: relative 1e-5 (summation rounding only, see
test_hip_rollout_tail.py).  Predictions with previous data against the fp64 restatement (tests/rollout_reference.py around the
oracle's model in double precision): the existing rollout bound, ``rel_err < 2e-5`` after 5 steps.  ``val_1step_rmse`` against
the golden first prediction: the golden test allows ``max |pred - pred1| < 2e-5 * max |pred1|``, which moves a root mean
square of ``pred - y`` by at most that much, so the relative bound is ``2e-5 * max |pred1| / rms(pred1 - y)``, formed in the
test and printed.
"""
import numpy as np
import pytest
import torch

import graph_physics_amd as gp
import recipe as R
import rollout_reference as RR
import sim_reference as SR
from conftest import load_golden, rel_err
from graph_physics_amd import harness
from oracle import mgn_oracle as O

pytestmark = pytest.mark.gpu
L, N, SEED, T = 3, 96, 51, 5
SUM_TOL = 1e-5
ROLLOUT_TOL = 2e-5


def _engine(dev, **kw):
    eng = harness.Engine(gp.cylinder_config(L, 128), dev, **kw)
    eng.model.load_state_dict(R.make_params(R.epd_param_shapes(L, 128, 11, 3, 2), SEED))
    g = load_golden("rollout_5steps")
    eng.sim.load_state_dict({k[len("norm."):]: v.to(dev) for k, v in g.items() if k.startswith("norm.")}, strict=False)
    return eng, g


def _frames(dev):
    pos, ei, ea, xs, ys = R.trajectory(N, T, SEED)
    eid, ead, posd = ei.to(dev), ea.to(dev), pos.to(dev)
    mk = lambda t: gp.Graph(x=xs[t].to(dev), y=ys[t].to(dev), pos=posd, edge_attr=ead, edge_index=eid)   # noqa: E731
    return [mk(t) for t in range(T)], [mk(T - 1 - t) for t in range(T - 1)], xs, ys   # two trajectories on ONE mesh


def _metrics64(preds, ys, types, masks=(0.0, 5.0)):
    """the dict of validate() in fp64 from per-trajectory lists of predictions and targets"""
    w = np.isin(types.astype(np.float64), masks)
    per, first, s_all, rows = [], [], 0.0, 0
    for tp, ty in zip(preds, ys):
        for k, (p, y) in enumerate(zip(tp, ty)):
            d2 = (p.double().cpu().numpy() - y.double().cpu().numpy()) ** 2
            per.append(d2[w].mean())
            s_all, rows = s_all + d2.sum(), rows + d2.size
            if k == 0:
                first.append(np.sqrt(d2.mean()))
    return dict(val_loss=float(np.mean(per)), val_all_rollout_rmse=float(np.sqrt(s_all / rows)), val_1step_rmse=float(np.mean(first)),
                val_loss_per_step=np.array(per))


def _same_bits(a, b):
    assert [len(t) for t in a["predictions"]] == [len(t) for t in b["predictions"]]
    for ta, tb in zip(a["predictions"], b["predictions"]):
        assert all(torch.equal(p, q) for p, q in zip(ta, tb)), "predictions differ"
    assert torch.equal(a["val_loss_per_step"], b["val_loss_per_step"])
    for k in ("val_loss", "val_all_rollout_rmse", "val_1step_rmse"):
        assert a[k] == b[k], k


def test_validate_eager_vs_rollout_fp64_metrics_and_golden(dev):
    eng, g = _engine(dev)
    A, B, xs, ys = _frames(dev)
    want = eng.rollout(A, graph="off")
    v = eng.validate([A], graph="off")
    assert len(v["predictions"]) == 1 and all(torch.equal(p, q) for p, q in zip(v["predictions"][0], want))
    ref = _metrics64(v["predictions"], [[f.y for f in A]], xs[0][:, 2].numpy())
    print("validate", {k: v[k] for k in ref}, "fp64", ref)
    assert v["val_loss_per_step"].dtype == torch.float64 and v["val_loss_per_step"].device.type == "cpu"
    assert np.abs(v["val_loss_per_step"].numpy() / ref["val_loss_per_step"] - 1).max() < SUM_TOL
    for k in ("val_loss", "val_all_rollout_rmse", "val_1step_rmse"):
        assert abs(v[k] / ref[k] - 1) < SUM_TOL, (k, v[k], ref[k])
    # the first step against the golden first prediction of the unmodified reference
    pred1, y0 = g["pred1"].double().numpy(), ys[0].double().numpy()
    rmse1 = np.sqrt(((pred1 - y0) ** 2).mean())
    tol = ROLLOUT_TOL * np.abs(pred1).max() / rmse1
    print(f"val_1step_rmse {v['val_1step_rmse']:.9e} golden {rmse1:.9e} tolerance {tol:.3e}")
    assert abs(v["val_1step_rmse"] / rmse1 - 1) < tol
    # make_prediction is the same frame step; predict_step keeps its result
    batch, pred, target, last, prev = eng.make_prediction(A[0], None, None)
    assert torch.equal(pred, want[0]) and last is pred and prev is None and torch.equal(target, A[0].y)
    assert torch.equal(eng.predict_step(A[1], pred), want[1])
    assert torch.equal(eng.make_prediction(A[1], pred, None)[1], want[1])


def test_validate_graphed_equals_eager_over_two_trajectories(dev):
    eng, _ = _engine(dev)
    A, B, xs, ys = _frames(dev)
    off = eng.validate([A, B], graph="off")
    assert "validate" not in eng._f_steps
    on = eng.validate([A, B], graph="on")
    step = eng._f_steps["validate"]["graph"]
    _same_bits(on, off)
    assert [len(t) for t in on["predictions"]] == [T, T - 1]
    # the second trajectory restarted from its own first frame: it equals that trajectory validated alone
    alone = eng.validate([B], graph="on")
    assert all(torch.equal(p, q) for p, q in zip(alone["predictions"][0], on["predictions"][1]))
    assert torch.equal(alone["val_loss_per_step"], on["val_loss_per_step"][T:])
    assert eng._f_steps["validate"]["graph"] is step, "one capture serves every trajectory on the mesh"
    _same_bits(eng.validate([A, B], graph="auto"), off)      # 5 frames on a small mesh: replayed
    assert eng._f_steps["validate"]["graph"] is step
    # rollout() without previous data is still the captured step it always was, and agrees
    assert all(torch.equal(p, q) for p, q in zip(eng.rollout(A, graph="on"), off["predictions"][0]))
    assert "rollout" not in eng._f_steps
    # loss masks of one type
    one, _ = _engine(dev, loss_masks=(5,))
    v5 = one.validate([A], graph="on")
    ref = _metrics64(v5["predictions"], [[f.y for f in A]], xs[0][:, 2].numpy(), (5.0,))
    assert np.abs(v5["val_loss_per_step"].numpy() / ref["val_loss_per_step"] - 1).max() < SUM_TOL
    assert v5["val_all_rollout_rmse"] == eng.validate([A], graph="on")["val_all_rollout_rmse"]


# ------------------------------------------------------------------------------------------------ previous data
LAY = SR.Layout("P", 6, 0, 4, 4, 0, 2, 2, 3, 3)   # x = [v_x, v_y, previous dv_x, previous dv_y, node_type, t]


def _previous_data_case(dev):
    cfg = gp.cylinder_config(L, 128)
    cfg["model"]["node_input_size"] = 4
    cfg["index"] = {"feature_index_start": 0, "feature_index_end": 4, "output_index_start": 0, "output_index_end": 2, "node_type_index": 4}
    eng = harness.Engine(cfg, dev, use_previous_data=True, previous_data_start=2, previous_data_end=4)
    params = R.make_params(R.epd_param_shapes(L, 128, 13, 3, 2), SEED)
    eng.model.load_state_dict(params)
    pos, ei, ea, xs, ys = R.trajectory(N, T, SEED)
    x6 = []
    for t in range(T):
        dv = xs[t][:, :2] - xs[t - 1][:, :2] if t > 0 else 0.05 * R.randn((N, 2), SEED + 7)
        x6.append(torch.cat([xs[t][:, :2], dv, xs[t][:, 2:4]], dim=1).contiguous())
    eid, ead, posd = ei.to(dev), ea.to(dev), pos.to(dev)
    frames = [gp.Graph(x=x6[t].to(dev), y=ys[t].to(dev), pos=posd, edge_attr=ead, edge_index=eid) for t in range(T)]
    eng.sim.train()                       # normaliser statistics: accumulated over the frames, then read back for the fp64 side
    for f in frames:
        eng.sim._build_input_graph(f, True)
    eng.sim.eval()
    sim = SR.Simulator64(LAY)
    for name, nz in sim.norms().items():
        t_ = getattr(eng.sim, name)
        nz.load(t_._acc_sum.cpu().numpy(), t_._acc_sum_squared.cpu().numpy(), float(t_._acc_count), float(t_._num_accumulations))
    p64 = {k: v.double() for k, v in params.items()}
    net = lambda xn, en: O.epd_forward(torch.from_numpy(xn), torch.from_numpy(en), ei, p64, L).numpy()   # noqa: E731
    ref = RR.Rollout64(sim, net, use_previous_data=True, previous=(2, 4))
    return eng, frames, ref, [(x6[t].numpy(), ys[t].numpy(), ea.numpy()) for t in range(T)]


def test_previous_data_vs_fp64_graphed_equals_eager_and_boundary_rows(dev):
    eng, frames, ref, host = _previous_data_case(dev)
    with torch.no_grad():
        want, seen = ref.rollout(host)
    eager = eng.rollout(frames, graph="off")
    for t in range(T):
        err = rel_err(eager[t], torch.from_numpy(want[t]))
        print(f"step {t + 1}: rel_err {err:.3e}")
        assert err < ROLLOUT_TOL, t
    plain, _ = RR.Rollout64(ref.sim, ref.net).rollout(host)               # the feedback is not a no-op on this model
    assert SR.rel_err(plain[4], want[4]) > 100 * ROLLOUT_TOL
    # the frame steps one by one: what is handed on, and the boundary rows of it
    mask = harness.build_mask(frames[0].x[:, 4])
    last = prev = None
    for t, f in enumerate(frames):
        batch, pred, target, last, prev = eng.make_prediction(f, last, prev)
        assert torch.equal(pred, eager[t])
        assert rel_err(batch.x, torch.from_numpy(seen[t])) < ROLLOUT_TOL
        assert torch.equal(prev, pred - batch.x[:, 0:2])
        assert torch.equal(pred[mask], f.y[mask]) and torch.equal(prev[mask], (f.y - batch.x[:, 0:2])[mask])
        assert bool(mask.any()) and not torch.equal(prev[~mask], (f.y - batch.x[:, 0:2])[~mask])
    # the captured step: same bits, and its feedback state ends where the eager loop's does
    graphed = eng.rollout(frames, graph="on")
    assert all(torch.equal(p, q) for p, q in zip(graphed, eager))
    S = eng._f_steps["rollout"]
    assert torch.equal(S["plast"], prev) and torch.equal(S["last"], last)
    assert all(torch.equal(p, q) for p, q in zip(eng.rollout(frames, graph="on"), eager)) and eng._f_steps["rollout"] is S
    off, on = eng.validate([frames, frames[:3]], graph="off"), eng.validate([frames, frames[:3]], graph="on")
    _same_bits(on, off)
    assert all(torch.equal(p, q) for p, q in zip(on["predictions"][0], eager))
    with torch.no_grad():
        v64 = ref.validate([host, host[:3]])
    # a sum of squared errors moves by dS / S <= 2 |d pred| / rms(pred - y); the smaller of the two root mean squares is taken
    tol = 2 * ROLLOUT_TOL * max(np.abs(p).max() for p in want) / min(v64["val_all_rollout_rmse"], v64["val_1step_rmse"])
    print(f"metrics {on['val_loss']:.9e} {on['val_all_rollout_rmse']:.9e} {on['val_1step_rmse']:.9e} fp64 {v64['val_loss']:.9e} "
          f"{v64['val_all_rollout_rmse']:.9e} {v64['val_1step_rmse']:.9e} tolerance {tol:.3e}")
    for k in ("val_loss", "val_all_rollout_rmse", "val_1step_rmse"):
        assert abs(on[k] / v64[k] - 1) < tol, k
