"""CPU: the fp64 restatement of the Simulator boundary (tests/sim_reference.py) against the golden file minted from the
unmodified reference (tests/golden/simulator_io.npz, make_golden_simulator_io.py), and the error of the reference's OWN
fp32 arithmetic against fp64 on the inputs the GPU tests use.

Bounds:
  * restatement vs golden outputs: rel_err < 1e-6 (the golden is an fp32 evaluation of the same formula);
  * restatement vs golden normaliser buffers: EQUAL -- every input is a multiple of 1/8 in [-2, 2], so the reference's
    fp32 sums are exact (sim_reference.exactly_summable) and an fp64 sum is the same number;
  * the reference's fp32 formula vs fp64 on those inputs: measured here <= 1.5e-7 at every row count of
    sim_reference.ROWS and widths 1, 4 and 32; asserted < 5e-7, so the 1e-6 the GPU tests ask of the kernels leaves the
    reference's own rounding at least a factor 2.
"""
import os

import numpy as np
import pytest

import sim_reference as SR
from scipy.spatial import cKDTree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulator_io.npz")
TOL = 1e-6
GOLDEN_CASES = [(lay, n, e) for lay in ("A", "B", "E") for (n, e) in ((9, 7), (2049, 2047))]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_golden_file_is_small_data():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "meshmask.npz"))
    z = np.load(GOLDEN, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiu" for k in z.files)
    assert {k.split(".")[0] for k in z.files} == {f"{lay}_{n}_{e}" for lay, n, e in GOLDEN_CASES}


@pytest.mark.parametrize("lname,N,E", GOLDEN_CASES)
def test_restatement_reproduces_the_reference(golden, lname, N, E):
    lay, case = SR.LAYOUTS[lname], f"{lname}_{N}_{E}"
    limit = int(golden[f"{case}.max_accumulations"])
    assert limit == (2 if case == "A_2049_2047" else 10 ** 5)
    sim = SR.Simulator64(lay, limit)
    rn, re = golden[f"{case}.rows_n"], golden[f"{case}.rows_e"]
    assert np.array_equal(rn, SR.sample_rows(N)) and np.array_equal(re, SR.sample_rows(E))
    packed = []
    for c in range(4):
        x, y, ea = SR.make_inputs(lay, N, E, c, SR.case_seed(lname, N))
        # the regenerated inputs are the minted ones: the kept rows, and the integer column sums over all rows
        assert np.array_equal(np.concatenate([x, y], axis=1)[rn] * 8, golden[f"{case}.c{c}.xy8"].astype(np.float32))
        assert np.array_equal(ea[re] * 8, golden[f"{case}.c{c}.ea8"].astype(np.float32))
        sums = np.concatenate([v.astype(np.float64).sum(axis=0) * 8 for v in (x, y, ea)])
        assert np.array_equal(sums, golden[f"{case}.c{c}.colsum8"].astype(np.float64))
        xn, tgt, en = sim.build_input(x, y, ea, training=(c != 3))
        nodes = golden[f"{case}.c{c}.nodes"]
        assert nodes.shape == (len(rn), lay.Wn + lay.O)
        assert SR.rel_err(nodes[:, :lay.Wn], xn[rn]) < TOL and SR.rel_err(nodes[:, lay.Wn:], tgt[rn]) < TOL
        if lay.edge_w > 0:
            assert SR.rel_err(golden[f"{case}.c{c}.edges"], en[re]) < TOL
        else:
            assert en is ea and f"{case}.c{c}.edges" not in golden
        packed.append(sim.packed_buffers())
        assert np.array_equal(packed[-1], golden[f"{case}.c{c}.norm"].astype(np.float64)), (case, c)
        assert sim.well_conditioned()
    assert np.array_equal(packed[3], packed[2])                      # eval accumulates nothing
    assert np.array_equal(packed[2], packed[1]) == (limit == 2)      # the cut-off, and only there
    assert sim.node.num_accumulations == min(3, limit)
    post, O = golden[f"{case}.post"], lay.O
    net_out = SR.eighths(N, O, 1000 * SR.case_seed(lname, N) + 90)
    mt = SR.mask_types(x[:, lay.type_idx])
    assert np.array_equal(post[:, :O], net_out[rn]) and np.array_equal(post[:, 3 * O], mt[rn])
    assert SR.rel_err(post[:, O:2 * O], sim.build_outputs(x, net_out)[rn]) < TOL
    masked = sim.predict(x, y, net_out, True, types=mt)
    assert SR.rel_err(post[:, 2 * O:3 * O], masked[rn]) < TOL
    keep = SR.keep_mask(mt)
    # a re-imposed row is y itself, bit for bit -- in the reference and in the restatement, also at types 0.5, -0.5, 5.5
    assert np.array_equal(post[:, 2 * O:3 * O][~keep[rn]], y[rn][:, :O][~keep[rn]])
    assert np.array_equal(masked[~keep], y[:, :O][~keep].astype(np.float64))
    assert not keep[mt == 0.5].any() and not keep[mt == -0.5].any() and not keep[mt == 5.5].any()
    assert keep[mt == 0.0].all() and keep[mt == 5.0].all()


def _normalize_fp32(v, s1, s2, count, eps=np.float32(1e-8)):
    """Normalizer.forward after the accumulation, operation by operation in fp32 as torch evaluates it on the CPU"""
    f = np.float32
    safe = max(f(count), f(1.0))
    mean = (s1 / safe).astype(f)
    var = ((s2 / safe).astype(f) - (mean * mean).astype(f)).astype(f)
    sd = np.maximum(np.sqrt(np.maximum(var, f(0.0))).astype(f), eps)
    return ((v - mean).astype(f) / sd).astype(f), ((v * sd).astype(f) + mean).astype(f)


def test_fp32_formula_against_fp64_on_the_exactly_summable_inputs():
    """The figure the GPU bound rests on: how far the reference's own fp32 evaluation is from fp64 on these inputs.
    Also that the inputs are what they claim: the fp32 sums, accumulated over three calls in forward and in reversed row
    order, are the fp64 sums."""
    assert SR.exactly_summable(max(n for n, _ in SR.ROWS), 3) and SR.exactly_summable(max(e for _, e in SR.ROWS), 3)
    worst = 0.0
    for N in sorted({n for n, _ in SR.ROWS} | {e for _, e in SR.ROWS} - {0}):
        for W in (1, 4, 32):
            nz = SR.Normalizer64(W)
            s1, s2, s1r = np.zeros((1, W), np.float32), np.zeros((1, W), np.float32), np.zeros((1, W), np.float32)
            for c in range(3):
                v = SR.balanced(N, W, 77, c) - (SR.balanced(N, W, 177, c) if W == 4 else 0)   # W = 4: a delta y - x, up to +-4
                v = v.astype(np.float32)
                ref = nz(v, True)
                s1 += np.add.reduce(v, axis=0, dtype=np.float32, keepdims=True)
                s1r += np.add.reduce(v[::-1], axis=0, dtype=np.float32, keepdims=True)
                s2 += np.add.reduce(v * v, axis=0, dtype=np.float32, keepdims=True)
                assert np.array_equal(s1, nz.acc_sum) and np.array_equal(s1r, nz.acc_sum) and np.array_equal(s2, nz.acc_sum_squared)
                got, inv = _normalize_fp32(v, s1, s2, nz.acc_count)
                assert nz.well_conditioned()
                worst = max(worst, SR.rel_err(got, ref), SR.rel_err(inv, nz.inverse(v)))
    print(f"fp32 Normalizer formula vs fp64 on the exactly-summable inputs: worst rel_err {worst:.3e}")
    assert 0.0 < worst < 5e-7


def test_one_hot_truncates_and_mask_compares_the_float():
    oh = SR.one_hot(np.array([2.75, -0.5, 8.0, 0.0], dtype=np.float32))
    assert oh.argmax(axis=1).tolist() == [2, 0, 8, 0] and oh.sum() == 4
    for bad in (9.0, -1.0):
        with pytest.raises(RuntimeError):
            SR.one_hot(np.array([0.0, bad], dtype=np.float32))
    assert SR.keep_mask(np.array([0.0, -0.0, 5.0, 0.5, -0.5, 5.5, 1.0], dtype=np.float32)).tolist() == [True, True, True, False, False, False, False]


def test_fresh_normaliser_and_single_row():
    """count 0: the clamp makes mean 0 / 1 and std eps, so build_outputs is x + net_out * eps; one row: variance 0, output 0"""
    lay = SR.LAYOUTS["C"]
    x, y, ea = SR.make_inputs(lay, 1, 0, 0)
    sim = SR.Simulator64(lay)
    net = np.array([[1.0, -2.0]])
    assert np.array_equal(sim.build_outputs(x, net), x[:, :2].astype(np.float64) + net * SR.STD_EPS)
    xn, tgt, en = sim.build_input(x, y, ea, True)
    assert not xn.any() and not tgt.any() and en.shape == (0, 3)
    assert sim.edge.num_accumulations == 1 and sim.edge.acc_count == 0


@pytest.mark.parametrize("lname", list(SR.LAYOUTS))
def test_every_gpu_case_is_well_conditioned(lname):
    """what test_hip_simulator_io.py asserts again next to its bounds: on these inputs no column's |mean| exceeds its std"""
    lay = SR.LAYOUTS[lname]
    for N, E in SR.ROWS:
        sim = SR.Simulator64(lay)
        for c in range(3):
            sim.build_input(*SR.make_inputs(lay, N, E, c, SR.case_seed(lname, N)), True)
            assert sim.well_conditioned(), (lname, N, E, c)


def test_query_pairs_is_the_double_compare():
    """what makes ``query_pairs`` a reference for the kernel's ``s <= r * r`` in double: boundary pairs, coincident points, r = 0"""
    for D in (2, 3):
        grid = np.stack(np.meshgrid(*[np.arange(5)] * D, indexing="ij"), axis=-1).reshape(-1, D).astype(np.float32) * np.float32(0.25)
        pts = np.concatenate([grid, grid[:7]])   # coincident points too
        for r in (0.25, 0.0, 0.3):
            got = {tuple(p) for p in cKDTree(pts).query_pairs(r, output_type="ndarray").reshape(-1, 2).tolist()}
            p64 = pts.astype(np.float64)
            s = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
            i, j = np.nonzero(s <= r * r)
            assert got == {(a, b) for a, b in zip(i.tolist(), j.tolist()) if a < b}, (D, r)
            assert len(got) >= 7
