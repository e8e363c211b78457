"""GPU: ``mgn_rollout_tail`` (csrc/mgn_rollout.inc) through ``call``, without a model: the prediction against
``mgn_sim_post(mask_truth=1)`` bit for bit, the feedback delta against the fp32 subtraction, the four metrics against fp64.

Shapes.  The row kernel runs a fixed grid of 256 blocks of 256 threads with a grid-stride loop over the N x O elements, and
reduces per wave of 64, then over the four waves of a block: N is taken around the wave (63, 64, 65) and the block (255, 256,
257), at 0 and 1, at 4099, and at 65800 > 256 * 256 + 257, where the loop takes a second pass whatever O; O is 1, 2, 3 and the
limit 32.  The output window starts at column 8, the node type sits in column 1, y is three columns wider than O.

Bounds.
  * pred and prev: equality of bits.
  * Dyadic inputs (``sim_reference.eighths``; output normaliser count 4, sum 2, sum of squares 17: mean 0.5, std 2): the
    prediction is a multiple of 1/8, and y is set to it minus an error of -2/8 .. 2/8, so every squared error is a multiple of
    2^-6 and their total stays below 2^18 even at 65800 x 32 elements (checked on the host): every partial sum, in any order,
    is an fp32 number, and the four metrics must EQUAL the fp64 values.
  * General inputs: pred is held to the project's ``TOL = 1e-6`` by ``rel_err`` against the fp64 restatement
    (test_hip_simulator_io.py); the sums are compared against fp64 sums over that very fp32 pred and y, so only summation
    rounding is left: under 3 ulp per term plus a tree of at most about 30 additions at these sizes, less than 2e-6; asserted
    at a relative 1e-5.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sim_reference as SR
from graph_physics_amd._launch import call

pytestmark = pytest.mark.gpu
TOL = 1e-6
SUM_TOL = 1e-5
NS = (0, 1, 63, 64, 65, 255, 256, 257, 4099, 65800)
OS = (1, 2, 3, 32)
LOSS_LISTS = ((0.0, 5.0), (5.0,), (0.0, 4.0, 5.0, 6.0))
SENTINEL = -777.0
assert NS[-1] > 256 * 256 + 257


def _layout(O):
    return SR.Layout(f"T{O}", 40, 4, 4, 1, 8, 8 + O, O + 3, 0, 1)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _tail(dev, lay, x, y, net, acc, N, loss=None, prev=True, table=None, cap=0):
    """one call; x, y, net, acc = (sum, sumsq, count): device tensors (one spare row at N = 0: no null pointers);
    table = (metrics, slot).  Returns pred, prev."""
    pred = torch.full((max(N, 1), lay.O), SENTINEL, dtype=torch.float32, device=dev)
    pv = torch.full((max(N, 1), lay.O), SENTINEL, dtype=torch.float32, device=dev) if prev else None
    part = torch.empty(3 * 256, dtype=torch.float32, device=dev)
    types = (C.c_float * len(loss))(*loss) if loss else None
    m, slot = table if table is not None else (None, None)
    rc = call("mgn_rollout_tail", dev, x.data_ptr(), lay.x_w, lay.out_start, lay.type_idx, y.data_ptr(), lay.y_w, net.data_ptr(), lay.O,
              acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), SR.STD_EPS, types, len(loss) if loss else 0, N, pred.data_ptr(),
              pv.data_ptr() if prev else None, part.data_ptr(), m.data_ptr() if m is not None else None,
              slot.data_ptr() if slot is not None else None, cap)
    assert rc == 0
    return pred[:N], (pv[:N] if prev else None)


def _sim_post(dev, lay, x, y, net, acc, N):
    pred = torch.empty(max(N, 1), lay.O, dtype=torch.float32, device=dev)
    call("mgn_sim_post", dev, x.data_ptr(), lay.x_w, lay.out_start, lay.type_idx, y.data_ptr(), lay.y_w, net.data_ptr(), lay.O,
         acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr(), SR.STD_EPS, 1, N, pred.data_ptr())
    return pred[:N]


def _metrics64(pred, y, types, O, loss):
    d2 = (pred.astype(np.float64) - y[:, :O].astype(np.float64)) ** 2
    w = np.isin(types.astype(np.float64), loss)
    return np.array([d2.sum(), d2[w].sum(), float(w.sum()), float(pred.shape[0])])


@functools.lru_cache(maxsize=None)
def _dyadic(N, O, types="mixed"):
    """host side of a dyadic case, computed once: inputs (one spare row at N = 0), the fp64 prediction and the error planted in y"""
    lay, rows = _layout(O), max(N, 1)
    x, net = SR.eighths(rows, lay.x_w, 11 + O), SR.eighths(rows, O, 23 + O)
    t = SR.mask_types(SR.type_codes(rows, 3)) if types == "mixed" else np.full(rows, 4.0 if types == "all masked" else 0.0, np.float32)
    x[:, lay.type_idx] = t
    raw = x[:, lay.out_start:lay.out_end].astype(np.float64) + (net.astype(np.float64) * 2.0 + 0.5)
    e = ((SR.eighths(rows, O, 37 + O) * 8).astype(np.int64) % 5 - 2) / 8.0          # -2/8 .. 2/8
    y = SR.eighths(rows, lay.y_w, 41 + O)
    y[:, :O] = (raw - e).astype(np.float32)
    assert np.array_equal(y[:, :O].astype(np.float64), raw - e)                      # multiples of 1/8 below 16: fp32 numbers
    keep = SR.keep_mask(t)
    pred = np.where(keep[:, None], raw, y[:, :O].astype(np.float64))[:N]
    d2 = (pred - y[:N, :O]) ** 2
    # every squared error a multiple of 2^-6, their total below 2^18: every partial sum is an fp32 number
    assert np.array_equal(d2 * 64, np.round(d2 * 64)) and d2.sum() < 2 ** 18
    return lay, x, y, net, t, pred


def _dyadic_acc(dev, O):
    return (torch.full((1, O), 2.0, device=dev), torch.full((1, O), 17.0, device=dev), torch.tensor(4.0, device=dev))


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("N", NS)
def test_dyadic_inputs_bits_and_exact_metrics(dev, N, O):
    lay, x, y, net, t, pred64 = _dyadic(N, O)
    xd, yd, nd, acc = _dev(x, dev), _dev(y, dev), _dev(net, dev), _dyadic_acc(dev, O)
    want = _sim_post(dev, lay, xd, yd, nd, acc, N) if N > 0 else torch.empty(0, O, device=dev)
    cap = 3
    m = torch.full((cap + 2, 4), SENTINEL, dtype=torch.float64, device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    for k, loss in enumerate(LOSS_LISTS):                     # three calls fill rows 0..2 (lists of 2, 1 and 4 types)
        pred, prev = _tail(dev, lay, xd, yd, nd, acc, N, loss, True, (m, slot), cap)
        assert torch.equal(pred, want), "pred differs from mgn_sim_post(mask_truth=1)"
        assert np.array_equal(pred.cpu().numpy().astype(np.float64), pred64)
        assert np.array_equal(prev.cpu().numpy(), pred.cpu().numpy() - x[:N, lay.out_start:lay.out_end])
        assert int(slot) == k + 1
    got = m.cpu().numpy()
    for k, loss in enumerate(LOSS_LISTS):
        assert np.array_equal(got[k], _metrics64(pred64, y[:N], t[:N], O, loss)), (k, got[k])
    if N >= 9:   # every node type occurs: the three lists select different rows
        assert got[0][2] > got[1][2] > 0 and got[2][2] > got[0][2] and got[0][1] > 0
    # a fourth call at capacity 3: accepted, nothing stored, the counter still advances (the host sees slot > cap)
    _tail(dev, lay, xd, yd, nd, acc, N, LOSS_LISTS[0], False, (m, slot), cap)
    assert int(slot) == 4 and np.array_equal(m.cpu().numpy()[:cap], got[:cap]) and bool((m[cap:] == SENTINEL).all())


@pytest.mark.parametrize("O", [1, 32])
@pytest.mark.parametrize("types", ["all masked", "none masked"])
def test_every_row_masked_and_no_row_masked(dev, types, O):
    N = 257
    lay, x, y, net, t, pred64 = _dyadic(N, O, types)
    xd, yd, nd, acc = _dev(x, dev), _dev(y, dev), _dev(net, dev), _dyadic_acc(dev, O)
    m = torch.full((2, 4), SENTINEL, dtype=torch.float64, device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    pred, prev = _tail(dev, lay, xd, yd, nd, acc, N, (0.0, 5.0), True, (m, slot), 2)
    assert torch.equal(pred, _sim_post(dev, lay, xd, yd, nd, acc, N))
    row = m.cpu().numpy()[0]
    assert np.array_equal(row, _metrics64(pred64, y, t, O, (0.0, 5.0)))
    if types == "all masked":     # the ground truth everywhere: no error, and no loss row: S_loss is exactly 0
        assert torch.equal(pred, yd[:, :O]) and row.tolist() == [0.0, 0.0, 0.0, float(N)]
        assert torch.equal(prev, yd[:, :O] - xd[:, lay.out_start:lay.out_end])
    else:
        assert row[2] == N and row[0] == row[1] > 0 and not torch.equal(pred, yd[:, :O])


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("N", [257, 4099])
def test_general_inputs_vs_fp64_and_determinism(dev, N, O):
    lay = _layout(O)
    rng = np.random.default_rng(100 * O + N)
    x = rng.standard_normal((N, lay.x_w)).astype(np.float32)
    y = rng.standard_normal((N, lay.y_w)).astype(np.float32)
    net = rng.standard_normal((N, O)).astype(np.float32)
    t = SR.mask_types(SR.type_codes(N, 5))
    x[:, lay.type_idx] = t
    ref = SR.Simulator64(lay)
    ref.out(ref.target_delta(x, y).astype(np.float32), True)   # the statistics of this frame's own delta: |mean| <= std
    assert ref.out.well_conditioned()
    acc32 = (ref.out.acc_sum.astype(np.float32), ref.out.acc_sum_squared.astype(np.float32), np.float32(ref.out.acc_count))
    ref.out.load(acc32[0], acc32[1], acc32[2], 1.0)              # the fp64 side reads the buffers the kernel reads
    acc = (_dev(acc32[0], dev), _dev(acc32[1], dev), torch.tensor(float(acc32[2]), device=dev))
    xd, yd, nd = _dev(x, dev), _dev(y, dev), _dev(net, dev)
    runs = []
    for _ in range(2):
        m = torch.zeros(1, 4, dtype=torch.float64, device=dev)
        slot = torch.zeros(1, dtype=torch.int32, device=dev)
        pred, prev = _tail(dev, lay, xd, yd, nd, acc, N, (0.0, 5.0), True, (m, slot), 1)
        runs.append((pred, prev, m))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"
    pred, prev, m = runs[0]
    assert torch.equal(pred, _sim_post(dev, lay, xd, yd, nd, acc, N))
    p = pred.cpu().numpy()
    err = SR.rel_err(p, ref.predict(x, y, net, True))
    assert err < TOL, f"pred: rel_err {err:.3e}"
    assert np.array_equal(prev.cpu().numpy(), p - x[:, lay.out_start:lay.out_end])
    want, got = _metrics64(p, y, t, O, (0.0, 5.0)), m.cpu().numpy()[0]
    print("metrics", got, "fp64 over the fp32 pred", want)
    assert got[2] == want[2] > 0 and got[3] == N
    assert abs(got[0] / want[0] - 1) < SUM_TOL and abs(got[1] / want[1] - 1) < SUM_TOL
    # without a table the call writes pred and prev only (null metrics, slot, no loss types)
    pred2, prev2 = _tail(dev, lay, xd, yd, nd, acc, N)
    assert torch.equal(pred2, pred) and torch.equal(prev2, prev)
    pred3, none = _tail(dev, lay, xd, yd, nd, acc, N, prev=False)
    assert torch.equal(pred3, pred) and none is None
