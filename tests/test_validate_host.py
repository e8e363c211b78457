"""CPU: the validation loops of ``harness.Engine`` (``make_prediction``, ``rollout`` with ``use_previous_data``, ``validate``)
on their torch statement against the fp64 restatement of tests/rollout_reference.py, the restatement itself against a case
worked out by hand, every refusal of the constructor, and the second header include/mgn_hip_ext.h against
``_capi.EXT_SYMBOLS`` (the first header and its 93 functions are test_capi_symbols.py's and stay as they are).

Bounds.  The engine's CPU path evaluates in fp32 what the restatement evaluates in fp64: per frame a normalisation, an affine
map of 13 inputs and the inverse normalisation, about 20 roundings of 6e-8 on numbers of the tensor's scale, and the map
below is a contraction (|A| sums to less than 1 per output), so a frame does not amplify what it inherits: five frames stay
under 5 * 20 * 6e-8 = 6e-6; asserted at the project's rollout bound ``rel_err < 2e-5`` (test_rollout_vs_golden).  A sum of
squared errors S moves by dS / S <= 2 * |d pred| / rms(pred - y), so the metrics are held to ``2 * 2e-5 * max|pred| /
rms(pred - y)``, formed in the test from the fp64 side and printed.
"""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

import capi_layout as CL
import graph_physics_amd as gp
import rollout_reference as RR
import sim_reference as SR
from conftest import REPO
from graph_physics_amd import _capi, harness

ROLLOUT_TOL = 2e-5


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def _hand_case(use_previous_data):
    """x = [v, p, type]: output column v, previous-data column p, both are features; the network is 0.25 * p.  The output
    normaliser holds count 4, sum 2, sum of squares 17 (mean 0.5, std 2), the node normaliser count 1, sum 0, sum of
    squares 1 (mean 0, std 1: the features pass unchanged)."""
    lay = SR.Layout("H", 3, 0, 2, 2, 0, 1, 1, 0, 1)
    sim = SR.Simulator64(lay)
    sim.out.load([2.0], [17.0], 4.0, 1.0)
    sim.node.load(np.zeros(11), np.ones(11), 1.0, 1.0)
    assert sim.out.mean()[0, 0] == 0.5 and sim.out.std()[0, 0] == 2.0
    net = lambda xn, en: 0.25 * xn[:, 1:2]   # noqa: E731
    ro = RR.Rollout64(sim, net, use_previous_data=use_previous_data, previous=(1, 2))
    x1 = np.array([[1, 1, 0], [2, -2, 5], [3, 4, 4], [4, 4, 0.5]], dtype=np.float32)
    y1 = np.array([[1.5], [2], [7], [8]], dtype=np.float32)
    x2 = np.array([[9, 9, 0], [9, 9, 5], [9, 9, 4], [9, 9, 0.5]], dtype=np.float32)
    y2 = np.array([[3], [1], [0], [0]], dtype=np.float32)
    ea = np.zeros((0, 1), dtype=np.float32)
    return ro, [(x1, y1, ea), (x2, y2, ea)]


def test_restatement_on_a_case_worked_out_by_hand():
    ro, frames = _hand_case(True)
    # frame 1: raw = v + 2 * (0.25 p) + 0.5 = [2, 1.5, 5.5, 6.5]; rows 2 (INFLOW) and 3 (type 0.5: the float is compared) take y
    xb, pred, target, last, prev = ro.make_prediction(*frames[0], None, None)
    assert np.array_equal(xb, frames[0][0]) and np.array_equal(target, frames[0][1])
    assert pred[:, 0].tolist() == [2.0, 1.5, 7.0, 8.0] and last is pred
    assert prev[:, 0].tolist() == [1.0, -0.5, 4.0, 4.0]                     # pred - v, after the re-imposition
    m = ro.frame_metrics(xb, pred, target)                                  # pred - y = [0.5, -0.5, 0, 0]
    assert (m["S_all"], m["S_loss"], m["n_loss"], m["N"]) == (0.5, 0.5, 2.0, 4.0)
    assert m["val_loss"] == 0.25 and m["rmse"] == np.sqrt(0.125)
    # frame 2: v <- [2, 1.5, 7, 8], p <- [1, -0.5, 4, 4]; raw = v + 0.5 p + 0.5 = [3, 1.75, 9.5, 10.5]
    xb, pred, target, last, prev2 = ro.make_prediction(*frames[1], last, prev)
    assert xb[:, 0].tolist() == [2.0, 1.5, 7.0, 8.0] and xb[:, 1].tolist() == [1.0, -0.5, 4.0, 4.0]
    assert pred[:, 0].tolist() == [3.0, 1.75, 0.0, 0.0] and prev2[:, 0].tolist() == [1.0, 0.25, -7.0, -8.0]
    m = ro.frame_metrics(xb, pred, target)                                  # pred - y = [0, 0.75, 0, 0]
    assert (m["S_all"], m["S_loss"], m["n_loss"]) == (0.5625, 0.5625, 2.0) and m["val_loss"] == 0.28125
    v = ro.validate([frames, frames[:1]])                                   # the state restarts with the second trajectory
    assert v["val_loss_per_step"].tolist() == [0.25, 0.28125, 0.25] and v["val_loss"] == (0.25 + 0.28125 + 0.25) / 3
    assert v["val_all_rollout_rmse"] == np.sqrt((0.5 + 0.5625 + 0.5) / 12) and v["val_1step_rmse"] == np.sqrt(0.125)
    assert np.array_equal(v["predictions"][1][0], v["predictions"][0][0])
    # without use_previous_data the column keeps the frame's own 9: row 0 is 2 + 2 * 2.25 + 0.5, and nothing is handed on
    ro, frames = _hand_case(False)
    _, pred, _, last, prev = ro.make_prediction(*frames[0], None, None)
    assert prev is None
    xb, pred, _, _, prev = ro.make_prediction(*frames[1], last, "kept")
    assert xb[0].tolist() == [2.0, 9.0, 0.0] and pred[0, 0] == 7.0 and prev == "kept"
    # a loss mask list of one type, and one that selects no row
    one = RR.Rollout64(ro.sim, ro.net, masks=(5.0,)).frame_metrics(frames[0][0], np.array([[2.0], [1.5], [7], [8]]), frames[0][1])
    assert (one["S_loss"], one["n_loss"], one["val_loss"]) == (0.25, 1.0, 0.25)
    none = RR.Rollout64(ro.sim, ro.net, masks=(3.0,)).frame_metrics(frames[0][0], np.array([[2.0], [1.5], [7], [8]]), frames[0][1])
    assert (none["S_loss"], none["n_loss"]) == (0.0, 0.0) and np.isnan(none["val_loss"])


# ------------------------------------------------------------------------------------------------ the engine on the CPU
LAY = SR.Layout("P", 6, 0, 4, 4, 0, 2, 2, 3, 3)   # x = [v_x, v_y, previous v_x, previous v_y, node_type, t]
PREVIOUS = (2, 4)


class _Affine(torch.nn.Module):
    """a fixed contraction of the 13 normalised node features (the edges are not read)"""

    def __init__(self):
        super().__init__()
        rng = np.random.default_rng(5)
        self.A64 = rng.uniform(-1, 1, size=(LAY.Wn, LAY.O)) / LAY.Wn
        self.b64 = np.array([0.125, -0.25])
        self.A, self.b = torch.from_numpy(self.A64.astype(np.float32)), torch.from_numpy(self.b64.astype(np.float32))
        self.A64, self.b64 = self.A.double().numpy(), self.b.double().numpy()   # the fp64 side uses the SAME coefficients

    def forward(self, graph):
        return graph.x @ self.A + self.b


def _config():
    cfg = gp.cylinder_config(2, 32)
    cfg["model"]["node_input_size"] = 4
    cfg["index"] = {"feature_index_start": 0, "feature_index_end": 4, "output_index_start": 0, "output_index_end": 2, "node_type_index": 4}
    return cfg


def _trajectory(N, T, seed):
    rng = np.random.default_rng(seed)
    types = np.array([0, 5, 4, 6, 0, 0, 1, 5, 0, 0, 0][:N], dtype=np.float32)
    frames = []
    for t in range(T):
        x = rng.standard_normal((N, 6)).astype(np.float32)
        x[:, 4], x[:, 5] = types, t
        frames.append((x, rng.standard_normal((N, 2)).astype(np.float32), rng.standard_normal((4, 3)).astype(np.float32)))
    return frames


def _graphs(frames):
    return [gp.Graph(x=torch.from_numpy(x.copy()), y=torch.from_numpy(y.copy()), pos=torch.zeros(x.shape[0], 2),
                     edge_attr=torch.from_numpy(ea.copy()), edge_index=torch.zeros(2, ea.shape[0], dtype=torch.int64))
            for x, y, ea in frames]


def _pair(use_previous_data, masks=None):
    """the engine on the CPU and the restatement, with the same normaliser state (accumulated by the engine over two frames)"""
    kw = dict(use_previous_data=True, previous_data_start=PREVIOUS[0], previous_data_end=PREVIOUS[1]) if use_previous_data else {}
    eng = harness.Engine(_config(), torch.device("cpu"), loss_masks=masks, **kw)
    aff = _Affine()
    eng.sim.model = aff
    eng.sim.train()
    for g in _graphs(_trajectory(11, 2, 99)):
        eng.sim._build_input_graph(g, True)
    eng.sim.eval()
    sim = SR.Simulator64(LAY)
    for name, nz in sim.norms().items():
        t = getattr(eng.sim, name)
        nz.load(t._acc_sum.numpy(), t._acc_sum_squared.numpy(), float(t._acc_count), float(t._num_accumulations))
    ref = RR.Rollout64(sim, lambda xn, en: xn @ aff.A64 + aff.b64, use_previous_data=use_previous_data, previous=PREVIOUS,
                       masks=(SR.NODE_NORMAL, SR.NODE_OUTFLOW) if masks is None else masks)
    return eng, ref


def _metric_tol(preds, frames):
    p = np.concatenate(preds)
    d = p - np.concatenate([y for _, y, _ in frames])
    tol = 2 * ROLLOUT_TOL * np.abs(p).max() / np.sqrt((d ** 2).mean())
    print(f"metric tolerance {tol:.3e}")
    return tol


@pytest.mark.parametrize("use_previous_data", [False, True])
def test_make_prediction_and_rollout_on_the_cpu(use_previous_data):
    eng, ref = _pair(use_previous_data)
    frames = _trajectory(11, 5, 7)
    graphs = _graphs(frames)
    want, seen = ref.rollout(frames)
    last = prev = None
    for t, g in enumerate(graphs):
        x_before = g.x.clone()
        batch, pred, target, last, prev = eng.make_prediction(g, last, prev)
        assert torch.equal(g.x, x_before) and batch is not g               # the caller's frame is left alone (batch.clone())
        assert last is pred and target is batch.y and torch.equal(target, g.y)
        assert SR.rel_err(pred.numpy(), want[t]) < ROLLOUT_TOL, t
        assert SR.rel_err(batch.x.numpy(), seen[t]) < ROLLOUT_TOL, t        # the frame the model saw, feedback columns included
        keep = SR.keep_mask(frames[t][0][:, 4])
        assert torch.equal(pred[~torch.from_numpy(keep)], g.y[~torch.from_numpy(keep)])
        if use_previous_data:
            assert torch.equal(prev, pred - batch.x[:, 0:2])
            assert torch.equal(prev[~torch.from_numpy(keep)], (g.y - batch.x[:, 0:2])[~torch.from_numpy(keep)])
            if t > 0:
                assert torch.equal(batch.x[:, 2:4], handed) and not torch.equal(batch.x[:, 2:4], g.x[:, 2:4])
            handed = prev
        else:
            assert prev is None and torch.equal(batch.x[:, 2:4], g.x[:, 2:4])
    for mode in ("auto", "off"):
        got = eng.rollout(graphs, graph=mode)
        assert len(got) == 5 and torch.equal(got[4], last)
    if use_previous_data:   # the feedback matters: the plain rollout of the same frames differs from the second frame on
        plain, _ = RR.Rollout64(ref.sim, ref.net).rollout(frames)
        assert SR.rel_err(plain[0], want[0]) == 0.0 and SR.rel_err(plain[1], want[1]) > 1e-3
    else:                   # predict_step: its signature and its result
        step = eng.predict_step(graphs[0], None)
        assert torch.equal(step, eng.make_prediction(graphs[0], None, None)[1])
        assert torch.equal(eng.predict_step(graphs[1], step), eng.rollout(graphs[:2], graph="off")[1])


@pytest.mark.parametrize("use_previous_data,masks", [(False, None), (True, None), (True, (5,)), (False, (0, 4, 5, 6))])
def test_validate_on_the_cpu(use_previous_data, masks):
    eng, ref = _pair(use_previous_data, masks)
    trajs = [_trajectory(11, 4, 21), _trajectory(6, 3, 22)]    # two meshes of different size: frames weigh by their rows
    want = ref.validate(trajs)
    got = eng.validate([_graphs(tr) for tr in trajs])
    assert set(got) == {"val_loss", "val_all_rollout_rmse", "val_1step_rmse", "val_loss_per_step", "predictions"}
    assert [len(p) for p in got["predictions"]] == [4, 3]
    for gp_, wp in zip(got["predictions"], want["predictions"]):
        for a, b in zip(gp_, wp):
            assert SR.rel_err(a.numpy(), b) < ROLLOUT_TOL
    tol = _metric_tol([p for tr in want["predictions"] for p in tr], [f for tr in trajs for f in tr])
    per = got["val_loss_per_step"]
    assert per.dtype == torch.float64 and per.device.type == "cpu" and per.shape == (7,)
    assert np.abs(per.numpy() / want["val_loss_per_step"] - 1).max() < tol
    for k in ("val_loss", "val_all_rollout_rmse", "val_1step_rmse"):
        assert isinstance(got[k], float) and abs(got[k] / want[k] - 1) < tol, (k, got[k], want[k])
    again = eng.validate([_graphs(tr) for tr in trajs], graph="off")       # the table is reused: same numbers
    assert torch.equal(again["val_loss_per_step"], per) and again["val_1step_rmse"] == got["val_1step_rmse"]
    # a table with fewer rows than frames: nothing past it is written, the counter runs on, and validate refuses the epoch
    small = (torch.full((3, 4), -7.0, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), 2)
    eng._metrics_table = lambda rows, dev: small
    with pytest.raises(RuntimeError, match="holds 2 rows and its counter reads 7"):
        eng.validate([_graphs(tr) for tr in trajs])
    assert bool((small[0][2] == -7.0).all()) and not bool((small[0][:2] == -7.0).any())
    del eng._metrics_table
    with pytest.raises(ValueError, match="at least one frame"):
        eng.validate([[]])
    with pytest.raises(ValueError, match="graph must be"):
        eng.validate([_graphs(trajs[0])], graph="maybe")


def test_constructor_refuses_bad_previous_data_ranges():
    dev, cfg = torch.device("cpu"), _config()
    ok = harness.Engine(cfg, dev, use_previous_data=True, previous_data_start=2, previous_data_end=4)
    assert (ok.use_previous_data, ok.previous_data_start, ok.previous_data_end) == (True, 2, 4)
    off = harness.Engine(cfg, dev, previous_data_start=0, previous_data_end=1)   # not in use: not checked, as in the reference
    assert not off.use_previous_data and tuple(int(t) for t in off.loss_masks) == (0, 5)
    for kw, text in ((dict(), "needs previous_data_start"), (dict(previous_data_start=2), "needs previous_data_start"),
                     (dict(previous_data_start=-2, previous_data_end=0), "no column range"),
                     (dict(previous_data_start=4, previous_data_end=2), "no column range"),
                     (dict(previous_data_start=2, previous_data_end=3), "hold 1 columns"),
                     (dict(previous_data_start=5, previous_data_end=8), "hold 3 columns"),
                     (dict(previous_data_start=1, previous_data_end=3), "overlap the output columns"),
                     (dict(previous_data_start=0, previous_data_end=2), "overlap the output columns"),
                     (dict(previous_data_start=3, previous_data_end=5), "contain the node-type column"),
                     (dict(previous_data_start=4, previous_data_end=6), "contain the node-type column")):
        with pytest.raises(ValueError, match=text):
            harness.Engine(cfg, dev, use_previous_data=True, **kw)
    # the width of x is known with the first frame: a range past it is refused there
    eng = harness.Engine(cfg, dev, use_previous_data=True, previous_data_start=5, previous_data_end=7)
    eng.sim.model = _Affine()
    with pytest.raises(ValueError, match="outside x"):
        eng.make_prediction(_graphs(_trajectory(11, 1, 3))[0], None, None)


# ------------------------------------------------------------------------------------------------ the second header
def _ext_header():
    with open(os.path.join(REPO, "include", "mgn_hip_ext.h")) as fh:
        return fh.read()


def _ext_prototypes():
    """name -> (return class, [argument classes]) of include/mgn_hip_ext.h, read like ``capi_layout.header_prototypes``"""
    text = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", CL._strip_comments(_ext_header()), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\s*\b(mgn_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        assert name not in out
        out[name] = (CL._c_class(ret.strip(), False), [] if params in (["void"], [""]) else [CL._c_class(p, True) for p in params])
    return out


def test_ext_symbols_match_the_second_header():
    protos = _ext_prototypes()
    assert sorted(protos) == sorted(_capi.EXT_SYMBOLS) == ["mgn_rollout_tail", "mgn_rollout_tail_scratch_floats"]
    assert "struct" not in CL._strip_comments(_ext_header())        # scalar and pointer arguments only
    lib, src = _capi.lib(), CL.unit_source("prep")
    for name, (ret, args) in protos.items():
        res, argtypes = _capi.EXT_SYMBOLS[name]
        assert [CL.ctypes_class(t) for t in argtypes] == args, name
        assert CL.ctypes_class(res) == ret, name
        fn = getattr(lib, name)                                       # exported, prototypes set by lib()
        assert fn.restype is res and list(fn.argtypes) == list(argtypes)
        assert CL.defines(src, name), f"{name} is not defined under mgn_prep.hip"
        assert name not in _capi.SYMBOLS and _capi._UNIT_OF[name] == "prep"
    # the first header is untouched: 93 functions, ABI 136, nine units
    first = CL.header_prototypes()
    assert len(first) == 93 and sorted(first) == sorted(_capi.SYMBOLS) and not set(first) & set(protos)
    assert lib.mgn_version() == 136 == _capi.EXPECTED_VERSION and len(_capi.UNITS) == 9 == len(_capi.SOURCES)
    assert lib.mgn_rollout_tail_scratch_floats() == 3 * 256


def test_new_sources_enter_the_source_hash(tmp_path, monkeypatch):
    inc = os.path.join(CL.CSRC, "mgn_rollout.inc")
    assert inc in _capi.DEPS and '#include "mgn_rollout.inc"' in open(os.path.join(CL.CSRC, "mgn_prep.hip")).read()
    rule = open(os.path.join(CL.CSRC, "Makefile")).read()
    assert "csrc/mgn_rollout.inc" in rule and "include/mgn_hip_ext.h" in rule
    before = _capi.source_hash()
    for attr, path in (("EXT_HEADER", _capi.EXT_HEADER), ("DEPS", inc)):
        copy = tmp_path / os.path.basename(path)
        shutil.copy(path, copy)
        with open(copy, "a") as fh:
            fh.write("\n")
        monkeypatch.setattr(_capi, attr, str(copy) if attr == "EXT_HEADER" else [d for d in _capi.DEPS if d != inc] + [str(copy)])
        assert _capi.source_hash() != before, attr
        monkeypatch.undo()
    assert _capi.source_hash() == before


def test_rollout_tail_refuses_bad_arguments_before_any_launch():
    lib = _capi.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)                  # a non-null pointer that is never dereferenced: every call is refused
    types = (ctypes.c_float * 4)(0.0, 5.0, 0.0, 0.0)

    def tail(O=2, y=p, pred=p, part=p, n_types=2, metrics=None, slot=None, cap=0, loss_types=types):
        return lib.mgn_rollout_tail(p, 6, 0, 4, y, 2, p, O, p, p, p, 1e-8, loss_types, n_types, 4, pred, None, part, metrics, slot, cap, None)

    cases = {"O = 0": dict(O=0), "O = 33": dict(O=33), "y null": dict(y=None), "pred null": dict(pred=None), "part null": dict(part=None),
             "no loss types": dict(metrics=p, slot=p, cap=4, n_types=0), "five loss types": dict(metrics=p, slot=p, cap=4, n_types=5),
             "metrics without a slot": dict(metrics=p, cap=4), "metrics with capacity 0": dict(metrics=p, slot=p, cap=0),
             "output window outside x": dict(O=7)}
    for what, kw in cases.items():
        assert lib.mgn_edge_features(None, 5, None, None, 0, None, None) == 1   # another refusal of the unit overwrites the text
        assert b"mgn_edge_features" in lib.mgn_prep_last_error()
        assert tail(**kw) == 1, what
        text = lib.mgn_prep_last_error().decode()
        assert text.startswith("mgn_rollout_tail: "), (what, text)
        with pytest.raises(RuntimeError) as e:
            _capi.check(1, "mgn_rollout_tail")              # the channel is found from the symbol: the prep unit's
        assert str(e.value) == f"mgn_rollout_tail failed (code 1): {text}"
