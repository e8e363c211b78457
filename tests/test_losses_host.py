"""CPU: the config's ``loss`` section -- the JSON factory (names, refusals), and the plain-torch statement of every loss against
values minted from the reference (tests/golden/physics_losses.npz).  The device kernels are held to the same fixture in
tests/test_hip_losses.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close3, rel_err

import graph_physics_amd as gp
from graph_physics_amd import losses as LS
import capi_layout
import loss_fixture as LF

FWD_TOL = 1e-5
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------- factory
@pytest.mark.parametrize("sec", sorted(LF.SECTIONS))
def test_get_loss_on_the_shipped_sections(sec):
    z = LF.fixture()
    loss, names = gp.get_loss({"loss": LF.SECTIONS[sec]})
    assert isinstance(loss, gp.MultiLoss) and loss.__name__ == "MultiLoss"
    assert names == [str(n) for n in z[f"names.{sec}"]]
    assert [type(l) for l in loss.losses] == [gp.LossType[n].value for n in names]
    assert list(loss.weights) == list(LF.SECTIONS[sec]["weights"])
    assert gp.get_gradient_method({"loss": LF.SECTIONS[sec]}) == str(z[f"method.{sec}"]) == LF.SECTIONS[sec]["gradient_method"]


def test_get_loss_without_a_section_is_l2():
    loss, name = gp.get_loss({"model": {}})
    assert isinstance(loss, gp.L2Loss) and name == "L2LOSS" == str(LF.fixture()["names.none"])
    assert gp.get_gradient_method({}) is None
    assert gp.get_gradient_method({"loss": {"type": ["l2loss"]}}) is None
    loss, name = gp.get_loss({"loss": {"type": ["L1SmoothLoss"]}})   # names are case-insensitive, as LossType[t.upper()]
    assert isinstance(loss, gp.L1SmoothLoss) and name == "L1SMOOTHLOSS"


def test_loss_names_are_the_references():
    want = {"L2LOSS": "MSE", "COSINEL2LOSS": "Cosine", "L1SMOOTHLOSS": "L1Smooth", "GRADIENTL2LOSS": "GradientL2Loss",
            "CONVECTIONL2LOSS": "ConvectionL2Loss", "DIVERGENCEL2LOSS": "DivergenceL2Loss", "DIVERGENCEL1LOSS": "DivergenceL1Loss",
            "DIVERGENCEL1SMOOTHLOSS": "DivergenceL1Smooth"}
    assert [m.name for m in gp.LossType] == list(LF.LOSS_ORDER)
    for k, v in want.items():
        assert gp.LossType[k].value().__name__ == v


@pytest.mark.parametrize("section, key", [
    ({"type": ["l2loss", "gradientl2loss"], "weights": [1, 1]}, "gradient_method"),                        # several types, no method
    ({"type": ["gradientl2loss"], "gradient_method": "finite_diff"}, "loss.type"),                        # one physics loss alone
    ({"type": ["divergencel1loss"]}, "loss.type"),
    ({"type": ["l2loss", "huberloss"], "weights": [1, 1], "gradient_method": "finite_diff"}, "loss.type"),   # unknown type
    ({"type": ["l2loss", "gradientl2loss"], "weights": [1, 1], "gradient_method": "spectral"}, "gradient_method"),   # unknown method
    ({"type": ["l2loss", "gradientl2loss"], "weights": [1], "gradient_method": "finite_diff"}, "loss.weights"),
    ({"type": ["l2loss", "gradientl2loss"], "gradient_method": "finite_diff"}, "loss.weights"),
])
def test_get_loss_refusals_name_the_key(section, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        gp.get_loss({"loss": section})


def test_multiloss_refuses_a_weight_count_mismatch():
    with pytest.raises(ValueError, match=r"loss\.weights"):
        gp.MultiLoss([gp.L2Loss(), gp.GradientL2Loss()], [1.0])


def test_least_squares_needs_faces():
    c = LF.Case("messy", CPU)
    g = gp.Graph(pos=c.graph.pos, edge_index=c.graph.edge_index)
    with pytest.raises(ValueError, match="face"):
        gp.LossGeometry(g, "least_squares")
    with pytest.raises(ValueError, match="gradient_method"):
        gp.LossGeometry(g, "central")


# ------------------------------------------------------------------------------- the torch formulas against the reference
@pytest.mark.parametrize("method", LF.METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_torch_values_and_gradient_field_vs_reference(case, method):
    c = LF.Case(case, CPU)
    want = c.ref(f"{method}.values")
    for i, name in enumerate(LF.LOSS_ORDER):
        got = float(LF.single_loss(c, name, method))
        err = abs(got - float(want[i])) / abs(float(want[i]))
        print(f"{case} {method} {name}: {got:.8e} vs {float(want[i]):.8e}  rel {err:.2e}")
        assert err < FWD_TOL, (name, got, float(want[i]))
    G = gp.compute_gradient(c.graph, c.physical(c.net), method=method)
    r = rel_err(G, c.ref(f"{method}.G"))
    print(f"{case} {method} G: rel {r:.2e}")
    assert r < FWD_TOL


@pytest.mark.parametrize("sec", sorted(LF.SECTIONS))
@pytest.mark.parametrize("method", LF.METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_torch_sections_vs_reference(case, method, sec):
    c = LF.Case(case, CPU)
    total, terms, dnet = LF.section_loss(c, sec, method)
    assert abs(float(total) - float(c.ref(f"{method}.{sec}.total"))) < FWD_TOL * abs(float(c.ref(f"{method}.{sec}.total")))
    assert rel_err(terms, c.ref(f"{method}.{sec}.terms")) < FWD_TOL
    assert abs(float(terms.sum()) - float(total)) < 1e-6 * abs(float(total))   # the list holds the WEIGHTED terms
    bar = c.grad_bar(method, sec)
    r, q, e = assert_close3(dnet, c.dnet64(method, sec), bar, f"{case} {method} {sec} d net")
    print(f"{case} {method} {sec}: d net vs fp64  max-rel {r:.2e} rms {q:.2e} elem {e:.2e}  (bar {bar:.1e}, "
          f"fp32 reference {float(c.ref(f'{method}.{sec}.dnet_ref_dist')):.2e})")


def test_geometry_is_pinned_on_the_graph_and_built_once():
    c = LF.Case("cyl", CPU)
    n0 = gp.LossGeometry.builds
    a = gp.compute_gradient(c.graph, c.physical(c.net), method="finite_diff")
    geom = c.graph.mgn_loss_geometry
    assert isinstance(geom, gp.LossGeometry) and gp.LossGeometry.builds == n0 + 1
    b = gp.compute_gradient(c.graph, c.physical(c.net), method="finite_diff")
    assert c.graph.mgn_loss_geometry is geom and gp.LossGeometry.builds == n0 + 1 and torch.equal(a, b)
    # a geometry pinned ahead of time is the one used
    c2 = LF.Case("cyl", CPU)
    c2.graph.mgn_loss_geometry = geom
    gp.compute_gradient(c2.graph, c2.physical(c2.net), method="finite_diff")
    assert c2.graph.mgn_loss_geometry is geom and gp.LossGeometry.builds == n0 + 1
    # another method on the same graph is another geometry
    gp.compute_gradient(c.graph, c.physical(c.net), method="least_squares")
    assert c.graph.mgn_loss_geometry is not geom and gp.LossGeometry.builds == n0 + 2


def test_a_self_pair_only_weighs():
    """vectorial_operators.py:97-127 on a three-node path with a self loop on node 0: the pair (0, 0) adds 2 / 1e-8 to node 0's
    weight sum and nothing to its numerator"""
    g = gp.Graph(pos=torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 2.0]]), edge_index=torch.tensor([[0, 0, 2], [0, 1, 1]]))
    u = torch.tensor([[1.0], [3.0], [-1.0]])
    G = gp.compute_gradient(g, u, method="finite_diff")
    w01, w12 = 1.0 / (1.0 + 1e-8), 1.0 / (4.0 + 1e-8)
    want0 = (2.0 * 1.0 * w01 * w01) / (w01 + 2e8 + 1e-8)
    assert abs(float(G[0, 0, 0]) - want0) < 1e-6 * want0 and float(G[0, 0, 1]) == 0.0
    want2 = (4.0 * 2.0 * w12 * w12) / (w12 + 1e-8)    # (U[1] - U[2]) * (pos[1] - pos[2]) = 4 * (0, -2) -> sign: same at both ends
    assert abs(float(G[2, 0, 1]) - (-want2)) < 1e-5 * want2


# ------------------------------------------------------------------------------- C ABI
def test_loss_args_layout_matches_header(tmp_path):
    from graph_physics_amd import _capi as c

    got = capi_layout.gcc_layout(tmp_path, {"mgn_loss_args": c.LossArgs}, macros=["MGN_LOSS_MAX_TERMS"])
    capi_layout.assert_layout(got, "mgn_loss_args", c.LossArgs)
    assert got["MGN_LOSS_MAX_TERMS"] == c.MAX_LOSS_TERMS
    assert (LS._L2, LS._COSINE, LS._L1SMOOTH, LS._GRADIENT, LS._CONVECTION, LS._DIV_L2, LS._DIV_L1, LS._DIV_L1SMOOTH) == tuple(range(8))


def test_loss_entry_points_validate_before_any_launch():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    assert lib.mgn_loss_workspace_bytes() >= (_capi.MAX_LOSS_TERMS + 1) * 4
    a = _capi.LossArgs()
    assert lib.mgn_loss_fwd(ctypes.byref(a), None) == 1
    assert b"mgn_loss_fwd" in lib.mgn_loss_last_error()
    assert lib.mgn_loss_bwd(ctypes.byref(a), None, None, None, None, None) == 1
    assert lib.mgn_loss_fd_geometry(None, None, None, None, 2, 10, None, None, None) == 1
    assert lib.mgn_loss_ls_geometry(None, 0, 5, None, 2, 10, None, None, None, None, None, None) == 1


def test_partitioned_step_refuses_a_physics_loss():
    """the nodal gradient of a partition needs halo rows of the fields: not built, so the partitioned step says so"""
    from graph_physics_amd import distributed

    with pytest.raises(NotImplementedError, match="loss"):
        distributed.check_partitioned_loss({"loss": LF.SECTIONS["pinn"]})
    distributed.check_partitioned_loss({})
    distributed.check_partitioned_loss({"loss": {"type": ["l2loss"]}})
