"""GPU: ``mgn_sim_pre`` / ``mgn_sim_post`` (csrc/mgn_prep.hip) through ``Simulator`` against the fp64 restatement of
tests/sim_reference.py (anchored to the reference by tests/golden/simulator_io.npz, test_sim_reference_host.py), at the
shapes where the kernels can go wrong: four column layouts, the 8 row lanes and the 2048-row stride of ``k_stats_partial``
plus and minus one, two strides, each of N*Wn, N*O and E*We sizing the normalising launch, E = 0, one row, a fresh
normaliser, the accumulation cut-off read from the device counter (also under a graph replay), the type-error flag, the
33-column refusal, and non-integral node types.

Bounds.  Inputs are multiples of 1/8 in [-2, 2] (``sim_reference.make_inputs``), so every partial sum and sum of
squares is an fp32 number in any summation order: the four buffers of every normaliser must EQUAL the fp64 values after
every call -- a dropped or doubled row cannot hide.  Normalised outputs, targets and predictions: rel_err < 1e-6 against
fp64; the restatement asserts |mean| <= std per varying column, so the bound is not spent on cancellation.  The
reference's own fp32 evaluation of the formula is within 1.3e-7 of fp64 on these inputs (measured and asserted < 5e-7
in test_sim_reference_host.py).

Before ``k_sim_post`` compared the float node type (it truncated with ``(int)(long)t`` first), all nine cases of
``test_masked_prediction_with_non_integral_types`` failed on an MI355X ("a non-integral type kept the prediction":
rows of type 0.5 and -0.5, truncated to NORMAL, and 5.5, to OUTFLOW, kept the prediction where the reference and the
module's torch fallback write the ground truth); the other 42 tests of this file passed on that library as well.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import graph_physics_amd as gp
import sim_reference as SR
from graph_physics_amd import _capi
from graph_physics_amd._launch import call

pytestmark = pytest.mark.gpu
TOL = 1e-6
NORMS = ("_node_normalizer", "_output_normalizer", "_edge_normalizer")
BUFFERS = ("_acc_sum", "_acc_sum_squared", "_acc_count", "_num_accumulations")


def _sim(lay, dev, limit=None, fused=True):
    sim = gp.Simulator(model=torch.nn.Identity(), device=dev, **lay.sim_kwargs())
    sim.fused = fused
    if limit is not None:
        for k in NORMS:
            if getattr(sim, k) is not None:
                getattr(sim, k)._max_accumulations = limit
    return sim


def _graph(x, y, ea, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return gp.Graph(x=t(x), y=t(y), pos=torch.zeros(x.shape[0], 2, device=dev), edge_attr=t(ea),
                    edge_index=torch.zeros(2, ea.shape[0], dtype=torch.int64, device=dev))


def _packed(sim):
    """the buffers in the order of ``Simulator64.packed_buffers``, as fp64 (exact: they are fp32 numbers)"""
    return np.concatenate([getattr(getattr(sim, k), b).detach().double().cpu().numpy().reshape(-1)
                           for k in NORMS if getattr(sim, k) is not None for b in BUFFERS])


def _close(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.isfinite(got).all(), what
    err = SR.rel_err(got, want)
    assert err < TOL, f"{what}: rel_err {err:.3e}"


@functools.lru_cache(maxsize=None)
def _reference(lname, N, E, limit):
    """the fp64 side of a case, computed once: per call the inputs, the normalised outputs and the packed buffers"""
    lay = SR.LAYOUTS[lname]
    ref = SR.Simulator64(lay, limit if limit is not None else 10 ** 5)
    calls = []
    for c in range(4):
        x, y, ea = SR.make_inputs(lay, N, E, c, SR.case_seed(lname, N))
        xn, tgt, en = ref.build_input(x, y, ea, training=(c < 3))
        assert ref.well_conditioned(), (lname, N, E, c)   # |mean| <= std: the bound below is not spent on cancellation
        calls.append((x, y, ea, xn, tgt, en, ref.packed_buffers()))
    net = SR.eighths(N, lay.O, 1000 * SR.case_seed(lname, N) + 90)
    x, y = calls[3][0], calls[3][1]
    fresh = SR.Simulator64(lay)
    return dict(calls=calls, net=net, pred=ref.build_outputs(x, net), pred_masked=ref.predict(x, y, net, True),
                keep=SR.keep_mask(x[:, lay.type_idx]), pred_fresh=fresh.build_outputs(x, net))


def _check_input_graph(sim, lay, g, ea_in, xn, tgt, en, what):
    graph, target = sim._build_input_graph(g, sim.training)
    _close(graph.x, xn, what + " node features")
    _close(target, tgt, what + " target")
    if lay.edge_w > 0:
        _close(graph.edge_attr, en, what + " edge features")
    else:
        assert graph.edge_attr is g.edge_attr   # no edge normaliser: the same object, untouched
        assert np.array_equal(graph.edge_attr.cpu().numpy(), ea_in)
    return graph, target


@pytest.mark.parametrize("N,E", SR.ROWS)
@pytest.mark.parametrize("lname", ["A", "B", "C", "E"])
def test_simulator_pre_post_vs_fp64(dev, lname, N, E):
    lay = SR.LAYOUTS[lname]
    assert SR.exactly_summable(max(N, E), 3)
    R = _reference(lname, N, E, None)
    sim, twin = _sim(lay, dev), _sim(lay, dev, fused=False)
    assert sim.fused and not twin.fused
    graphs = [_graph(x, y, ea, dev) for (x, y, ea, *_rest) in R["calls"]]
    assert sim._can_fuse(graphs[0])
    # a fresh normaliser: count 0 is clamped to 1, mean 0, std eps
    _close(sim.predict(graphs[3], torch.from_numpy(R["net"]).to(dev)), R["pred_fresh"], "fresh predict")
    for s in (sim, twin):
        s.train()
        for c in range(3):   # three training calls: statistics accumulate BEFORE normalising
            x, y, ea, xn, tgt, en, packed = R["calls"][c]
            _check_input_graph(s, lay, graphs[c], ea, xn, tgt, en, f"{'fused' if s.fused else 'torch'} call {c}")
            assert np.array_equal(_packed(s), packed), f"{'fused' if s.fused else 'torch'} buffers after call {c}"
            if N == 1 and c == 0:   # one row: variance 0, (v - mean) exactly 0
                graph, target = s._build_input_graph(graphs[c], False)
                assert not graph.x.any() and not target.any()
        s.eval()
        x, y, ea, xn, tgt, en, packed = R["calls"][3]
        before = {k: {b: getattr(getattr(s, k), b).clone() for b in BUFFERS} for k in NORMS if getattr(s, k) is not None}
        _check_input_graph(s, lay, graphs[3], ea, xn, tgt, en, "eval call")
        for k in before:   # eval: bitwise unchanged
            for b in BUFFERS:
                assert torch.equal(before[k][b], getattr(getattr(s, k), b)), (k, b)
        assert np.array_equal(_packed(s), R["calls"][2][6])
        net = torch.from_numpy(R["net"]).to(dev)
        _close(s.predict(graphs[3], net), R["pred"], "predict")
        _close(s.build_outputs(graphs[3], net), R["pred"], "build_outputs")
        got = s.predict(graphs[3], net, mask_truth=True)
        _close(got, R["pred_masked"], "masked predict")
        keep = torch.from_numpy(R["keep"])
        assert torch.equal(got.cpu()[~keep], torch.from_numpy(y[:, :lay.O])[~keep])   # re-imposed rows are y itself
    sim.check_node_types()   # all codes valid: the flag stayed clear


@pytest.mark.parametrize("lname,N,E", [("A", 2049, 2047), ("C", 9, 7), ("B", 300, 4099)])
def test_accumulation_cut_off(dev, lname, N, E):
    """max_accumulations = 2 on all three normalisers: the third training call leaves buffers and counter bitwise alone
    and still normalises; a module loaded from a state dict whose counter is already at the limit does the same."""
    lay = SR.LAYOUTS[lname]
    R = _reference(lname, N, E, 2)
    sim = _sim(lay, dev, limit=2)
    sim.train()
    graphs = [_graph(x, y, ea, dev) for (x, y, ea, *_rest) in R["calls"]]
    for c in range(3):
        x, y, ea, xn, tgt, en, packed = R["calls"][c]
        _check_input_graph(sim, lay, graphs[c], ea, xn, tgt, en, f"call {c}")
        assert np.array_equal(_packed(sim), packed), c
    assert np.array_equal(R["calls"][2][6], R["calls"][1][6]) and float(sim._node_normalizer._num_accumulations) == 2.0
    loaded = _sim(lay, dev, limit=2)
    loaded.load_state_dict(sim.state_dict())
    loaded.train()
    x, y, ea, xn, tgt, en, packed = R["calls"][2]
    _check_input_graph(loaded, lay, graphs[2], ea, xn, tgt, en, "loaded at the limit")
    assert np.array_equal(_packed(loaded), packed)
    # the same state without the limit goes on accumulating
    free = _sim(lay, dev)
    free.load_state_dict(sim.state_dict())
    free.train()
    free._build_input_graph(graphs[2], True)
    assert float(free._node_normalizer._num_accumulations) == 3.0 and float(free._output_normalizer._acc_count) == 3.0 * N


def test_graph_replay_stops_at_the_cut_off(dev):
    """One captured training call (single stream, no parallel branches), limit 2: after a warm-up call and three replays
    the counter is 2 and the sums are those of two calls -- the kernels read the device counter at replay time."""
    lname, N, E = "A", 2049, 2047
    lay = SR.LAYOUTS[lname]
    x, y, ea = SR.make_inputs(lay, N, E, 0, SR.case_seed(lname, N))
    ref = SR.Simulator64(lay, 2)
    for _ in range(3):
        xn, tgt, en = ref.build_input(x, y, ea, True)
    assert ref.node.num_accumulations == 2 and ref.well_conditioned()
    sim = _sim(lay, dev, limit=2)
    sim.train()
    g = _graph(x, y, ea, dev)
    sim._build_input_graph(g, True)   # warm-up: workspace and flag allocated, node types checked, counter 1
    torch.cuda.synchronize(dev)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        graph, target = sim._build_input_graph(g, True)
    torch.cuda.synchronize(dev)
    assert float(sim._node_normalizer._num_accumulations) == 1.0   # capturing ran nothing
    for _ in range(3):
        cg.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(_packed(sim), ref.packed_buffers())
    _close(graph.x, xn, "replayed node features")
    _close(target, tgt, "replayed target")
    _close(graph.edge_attr, en, "replayed edge features")


def test_type_codes(dev):
    """9 and -1 raise (F.one_hot does); 2.75 and -0.5 truncate toward zero to one-hot columns 2 and 0 (``.long()``)."""
    lay = SR.LAYOUTS["C"]
    x, y, ea = SR.make_inputs(lay, 9, 7, 0)
    for bad in (9.0, -1.0):
        xb = x.copy()
        xb[4, lay.type_idx] = bad
        with pytest.raises(RuntimeError, match="node type codes"):
            _sim(lay, dev)._build_input_graph(_graph(xb, y, ea, dev), False)   # the first fused call checks itself
        sim = _sim(lay, dev)
        sim._build_input_graph(_graph(x, y, ea, dev), False)
        sim.check_node_types()
        sim._build_input_graph(_graph(xb, y, ea, dev), False)                  # later calls only raise the flag
        with pytest.raises(RuntimeError, match="node type codes"):
            sim.check_node_types()
        with pytest.raises(RuntimeError):
            SR.Simulator64(lay).build_input(xb, y, ea, False)
    xt = x.copy()
    xt[0, lay.type_idx], xt[1, lay.type_idx] = 2.75, -0.5
    sim, ref = _sim(lay, dev), SR.Simulator64(lay)
    graph, _ = sim._build_input_graph(_graph(xt, y, ea, dev), False)   # fresh statistics: mean 0, std eps
    sim.check_node_types()
    hot = graph.x[:2, 2:].cpu().numpy() != 0
    assert hot.sum(axis=1).tolist() == [1, 1] and hot.argmax(axis=1).tolist() == [2, 0]
    _close(graph.x, ref.build_input(xt, y, ea, False)[0], "truncated one-hot")


def test_33_columns_are_not_fused_and_refused_by_the_kernel(dev):
    lay = SR.LAYOUTS["W33"]
    assert lay.Wn == 33
    N, E = 300, 40
    sim, ref = _sim(lay, dev), SR.Simulator64(lay)
    sim.train()
    for c in range(2):
        x, y, ea = SR.make_inputs(lay, N, E, c, SR.case_seed("W33", N))
        g = _graph(x, y, ea, dev)
        assert not sim._can_fuse(g)
        xn, tgt, en = ref.build_input(x, y, ea, True)
        assert ref.well_conditioned()
        _check_input_graph(sim, lay, g, ea, xn, tgt, en, f"33 columns, call {c}")
        assert np.array_equal(_packed(sim), ref.packed_buffers())
    d, keep, (xd, yd, ead) = sim._desc(g, False)
    xn_out, tg_out, en_out = torch.empty(N, 33, device=dev), torch.empty(N, 3, device=dev), torch.empty_like(ead)
    d.node_out, d.target_out, d.edge_out = xn_out.data_ptr(), tg_out.data_ptr(), en_out.data_ptr()
    ws = torch.empty(_capi.lib().mgn_sim_workspace_bytes(), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="feature widths"):
        call("mgn_sim_pre", dev, C.byref(d), ws.data_ptr(), ws.numel())


@pytest.mark.parametrize("O", [1, 3, 32])
@pytest.mark.parametrize("N", [255, 256, 257])
def test_masked_prediction_with_non_integral_types(dev, N, O):
    """Rows of type -0.5, 0.5 and 5.5 receive y (the reference compares the float); rows of type 0 and 5 keep the
    prediction.  Fused kernel and torch fallback of the same module agree."""
    lay = SR.Layout("M", 40, 4, 4, 1, 8, 8 + O, O, 0, 1)
    x, y, ea = SR.make_inputs(lay, N, 0, 0, 5)
    x[:, lay.type_idx] = SR.mask_types(x[:, lay.type_idx])
    t = x[:, lay.type_idx]
    assert all((t == v).sum() >= 30 for v in (-0.5, 0.5, 5.5, 0.0, 5.0))
    ref = SR.Simulator64(lay)
    ref.build_input(x, y, ea, True)
    assert ref.well_conditioned()
    net = SR.eighths(N, O, 4242)
    want, plain = ref.predict(x, y, net, True), ref.build_outputs(x, net)
    sim = _sim(lay, dev)
    sim.train()
    g = _graph(x, y, ea, dev)
    sim._build_input_graph(g, True)
    sim.eval()
    imposed = torch.from_numpy((t == -0.5) | (t == 0.5) | (t == 5.5))
    kept = torch.from_numpy((t == 0.0) | (t == 5.0))
    y_t = torch.from_numpy(y[:, :O])
    for fused in (True, False):
        sim.fused = fused
        free = sim.predict(g, torch.from_numpy(net).to(dev), mask_truth=False).cpu()
        got = sim.predict(g, torch.from_numpy(net).to(dev), mask_truth=True).cpu()
        _close(free, plain, "prediction")
        assert torch.equal(got[imposed], y_t[imposed]), f"fused={fused}: a non-integral type kept the prediction"
        assert torch.equal(got[kept], free[kept]) and not torch.equal(got[kept], y_t[kept])
        _close(got, want, "masked prediction")
