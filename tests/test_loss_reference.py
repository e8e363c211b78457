"""CPU: (1) tests/loss_reference.py, the independent fp64 statement of the ``loss`` section, anchored on the values minted from the
reference (tests/golden/physics_losses.npz); (2) the plain-torch path of ``graph_physics_amd.losses`` -- what CPU tensors and
``MGN_TORCH_LOSS`` take -- held to it in float64 at every shape tests/test_hip_loss_kernels.py runs on the device kernels."""
import pytest
import torch

from conftest import rel_err

import loss_cases as LC
import loss_fixture as LF
import loss_reference as REF

FWD_TOL = 1e-5
CPU = torch.device("cpu")
F64 = torch.float64
METHODS = LC.METHODS


# ------------------------------------------------------------------------------- 1. the reference against the fixture
def _fixture_inputs(c, method):
    """the fixture case as fp64 tensors, ``net`` a leaf and the physical field built from it as make_golden_losses.py does"""
    geom = REF.Geometry(c.graph.pos, method, edge_index=c.graph.edge_index, face=c.graph.face)
    d = lambda t: t.double()  # noqa: E731
    net = d(c.net).requires_grad_(True)
    u_out, u_tgt = d(c.pre) + (net * d(c.std) + d(c.mean)), d(c.pre) + (d(c.tgt) * d(c.std) + d(c.mean))
    return geom, net, d(c.tgt), d(c.node_type), u_out, u_tgt


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_reference_values_and_gradient_field_vs_fixture(case, method):
    c = LF.Case(case, CPU)
    geom, net, tgt, nt, u_out, u_tgt = _fixture_inputs(c, method)
    want = c.ref(f"{method}.values")
    for k in REF.ALL_KINDS:
        total = REF.evaluate((k,), (1.0,), geom, net, tgt, nt, LF.MASKS, u_out, u_tgt)[0].detach()
        r = rel_err(total, want[k])
        print(f"{case} {method} {REF.KIND_NAMES[k]}: {float(total):.8e} vs {float(want[k]):.8e}  rel {r:.2e}")
        assert r < FWD_TOL
    r = rel_err(geom.gradient(u_out), c.ref(f"{method}.G"))
    print(f"{case} {method} G: rel {r:.2e}")
    assert r < FWD_TOL


@pytest.mark.parametrize("sec", sorted(LF.SECTIONS))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_reference_sections_vs_fixture_fp64(case, method, sec):
    """d total / d net of both shipped sections against the reference's own float64 evaluation: both sides are fp64 evaluations of
    the same fp32 positions, so 1e-7 -- two orders under the tightest bar a kernel is held to -- is generous"""
    c = LF.Case(case, CPU)
    geom, net, tgt, nt, u_out, u_tgt = _fixture_inputs(c, method)
    kinds = [LF.LOSS_ORDER.index(t.upper()) for t in LF.SECTIONS[sec]["type"]]
    total, terms, _ = REF.evaluate(kinds, LF.SECTIONS[sec]["weights"], geom, net, tgt, nt, LF.MASKS, u_out, u_tgt)
    total.backward()
    rt, rs = rel_err(total, c.ref(f"{method}.{sec}.total")), rel_err(torch.stack(terms), c.ref(f"{method}.{sec}.terms"))
    d = rel_err(net.grad, c.dnet64(method, sec))
    print(f"{case} {method} {sec}: total {rt:.2e} terms {rs:.2e}  d net vs the reference's fp64 {d:.2e}")
    assert rt < FWD_TOL and rs < FWD_TOL
    assert d < 1e-7


def test_pair_rule_on_a_messy_edge_list():
    """duplicates, both directions and self pairs collapse to unique undirected pairs; a self pair is reported, not paired"""
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 0], [1, 0, 0, 2, 1, 3, 3, 2]])
    i, j, loops = REF.unique_pairs(ei, 4)
    assert sorted(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 2), (1, 2)] and loops.tolist() == [2, 3]


# ------------------------------------------------------------------------------- 2. the torch path at the new shapes, float64
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(LC.MEDIUM))
def test_torch_every_kind_alone(name, method):
    LC.case_single_kinds(name, method, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("which", sorted(LC.POINTWISE_LISTS))
def test_torch_several_pointwise_terms(which, method):
    LC.case_several_pointwise(which, method, CPU, F64, own_sum=False)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("F", (1, 2, 3, 4))
@pytest.mark.parametrize("name", sorted(LC.SMALL))
def test_torch_shape_matrix(name, F, method):
    LC.case_shape(name, F, method, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("O", (1, 5, 11))
def test_torch_output_width(O, method):
    LC.case_output_width(O, method, CPU, F64)


@pytest.mark.parametrize("F", (1, 2))
def test_torch_path_graph(F):
    LC.case_path_graph(F, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(LC.SMALL))
def test_torch_compute_gradient(name, method):
    LC.case_compute_gradient(name, method, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("masks", LC.MASK_SETS + (LC.FIVE_MASKS,), ids=lambda m: "-".join(map(str, m)))
def test_torch_layout_and_masks(masks, method):
    LC.case_layout(masks, method, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nx, ny", [(5, 6), (4, 8), (3, 11), (3, 2731), (181, 182)])
def test_torch_row_counts(nx, ny, method):
    LC.case_rows(nx, ny, method, CPU, F64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ("tri2d", "tri3d", "tets"))
def test_torch_degenerate_geometry(name, method):
    LC.case_degenerate(name, method, CPU, F64)
    LC.case_geometry(name, method, CPU)


@pytest.mark.parametrize("method", METHODS)
def test_torch_zero_selected_rows(method):
    LC.case_zero_selected(method, CPU, F64)
