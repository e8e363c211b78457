"""GPU: the config's ``loss`` section on the engine's kernels (csrc/mgn_loss.hip through the C ABI) against values minted from
the reference (tests/golden/physics_losses.npz), and ``Engine`` trained with it."""
import numpy as np
import pytest
import torch

from conftest import assert_close3, rel_err

import graph_physics_amd as gp
from graph_physics_amd import harness
import loss_fixture as LF
import recipe as R

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5    # north_star: forward parity
GRAD_TOL = 1e-4   # parameter gradients through the whole model (tests/test_hip_parity.py)


@pytest.fixture(autouse=True)
def _kernels_only(monkeypatch):
    monkeypatch.delenv("MGN_TORCH_LOSS", raising=False)


# ------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("method", LF.METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_each_loss_alone_vs_reference(dev, case, method):
    c = LF.Case(case, dev)
    want = c.ref(f"{method}.values")
    for i, name in enumerate(LF.LOSS_ORDER):
        got = LF.single_loss(c, name, method)
        assert got.is_cuda
        r = rel_err(got, want[i])
        print(f"{case} {method} {name}: {float(got):.8e} vs {float(want[i]):.8e}  rel {r:.2e}")
        assert r < FWD_TOL, (name, float(got), float(want[i]))
    G = gp.compute_gradient(c.graph, c.physical(c.net), method=method)
    r = rel_err(G, c.ref(f"{method}.G"))
    print(f"{case} {method} G: rel {r:.2e}")
    assert r < FWD_TOL


# ------------------------------------------------------------------------------- 1 + 2. the shipped sections, values and gradient
@pytest.mark.parametrize("sec", sorted(LF.SECTIONS))
@pytest.mark.parametrize("method", LF.METHODS)
@pytest.mark.parametrize("case", LF.CASES)
def test_shipped_sections_vs_reference(dev, case, method, sec):
    c = LF.Case(case, dev)
    total, terms, dnet = LF.section_loss(c, sec, method)
    rt, rs = rel_err(total, c.ref(f"{method}.{sec}.total")), rel_err(terms, c.ref(f"{method}.{sec}.terms"))
    print(f"{case} {method} {sec}: total rel {rt:.2e}, terms rel {rs:.2e}")
    assert rt < FWD_TOL and rs < FWD_TOL
    # against the float64 evaluation of the reference, at least as close as the float32 reference itself is
    bar = c.grad_bar(method, sec)
    d = rel_err(dnet, c.dnet64(method, sec))
    print(f"{case} {method} {sec}: d net vs fp64 max-rel {d:.2e}  (bar {bar:.1e}, fp32 reference "
          f"{float(c.ref(f'{method}.{sec}.dnet_ref_dist')):.2e})")
    r, q, e = assert_close3(dnet, c.dnet64(method, sec), bar, f"{case} {method} {sec} d net")
    print(f"   rms {q:.2e} element-wise {e:.2e}")


# ------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("method", LF.METHODS)
def test_two_runs_are_bit_identical(dev, method):
    for case in ("cyl", "tet"):
        c = LF.Case(case, dev)
        a = LF.section_loss(c, "panels", method)
        b = LF.section_loss(c, "panels", method)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------- 4. Engine
def _engine(dev, L=3, seed=41, lr=1e-3, warmup=4, num_steps=100):
    cfg = dict(gp.cylinder_config(L, 128), loss=LF.SECTIONS["pinn"])
    eng = harness.Engine(cfg, dev, learning_rate=lr, num_steps=num_steps, warmup=warmup)
    eng.model.load_state_dict(R.make_params(R.epd_param_shapes(L, 128, 11, 3, 2), seed))
    return eng


def test_engine_train_steps_vs_reference(dev):
    """two eager steps with the pinn-aneurysm section against two steps of the reference's training step, at the bars of
    test_hip_parity.test_train_steps_vs_golden"""
    L, N, seed = 3, 96, 41
    z = {k[len("train."):]: torch.from_numpy(np.asarray(v)) for k, v in LF.fixture().items() if k.startswith("train.")}
    pos, ei, ea, xs, ys = R.trajectory(N, 3, seed)
    eng = _engine(dev, L, seed)
    assert eng.loss_name == ["L2LOSS", "GRADIENTL2LOSS", "DIVERGENCEL2LOSS"] and eng.gradient_method == "finite_diff"
    eid = ei.to(dev)
    for t in range(2):
        batch = gp.Graph(x=xs[t].to(dev), y=ys[t].to(dev), pos=pos.to(dev), edge_attr=ea.to(dev), edge_index=eid)
        loss = eng.train_step(batch)
        print(f"step {t}: loss {float(loss):.6f} vs {float(z['loss'][t]):.6f}, grad norm {float(eng.last_grad_norm):.4f} vs "
              f"{float(z['grad_norm'][t]):.4f}, terms {[float(x) for x in eng.last_losses]} vs {z['terms'][t].tolist()}")
        assert abs(float(loss) - float(z["loss"][t])) < 2e-5 * float(z["loss"][t])
        assert abs(float(eng.last_grad_norm) - float(z["grad_norm"][t])) < GRAD_TOL * float(z["grad_norm"][t])
        assert len(eng.last_losses) == 3
        for got, want in zip(eng.last_losses, z["terms"][t]):
            assert got.is_cuda and abs(float(got) - float(want)) < 2e-5 * abs(float(want))
    sd = eng.model.state_dict()
    assert torch.allclose(sd["decode_module.6.weight"].cpu(), z["w_last"], rtol=1e-4, atol=5e-6)
    assert torch.allclose(sd["nodes_encoder.0.bias"].cpu(), z["b_first"], rtol=1e-4, atol=5e-6)
    sums = np.array([sd[k].double().sum().item() for k in sd])
    assert np.allclose(sums, z["param_sum"].numpy(), rtol=1e-5, atol=2e-3)
    assert torch.allclose(eng.sim._node_normalizer._acc_sum.cpu(), z["node_norm_sum"], rtol=1e-6)


def test_engine_graphed_step_equals_eager(dev):
    """hipGraph replay of the whole training step with the loss section == the eagerly launched step"""
    L, N, seed = 3, 96, 41
    pos, ei, ea, xs, ys = R.trajectory(N, 3, seed)
    eid = ei.to(dev)
    mk = lambda t: gp.Graph(x=xs[t].to(dev), y=ys[t].to(dev), pos=pos.to(dev), edge_attr=ea.to(dev), edge_index=eid)  # noqa: E731
    eager = _engine(dev, L, seed)
    losses_e, terms_e = [], []
    for t in range(5):
        losses_e.append(float(eager.train_step(mk(t % 3))))
        terms_e.append([float(x) for x in eager.last_losses])
    graphed = _engine(dev, L, seed)
    n0 = gp.LossGeometry.builds
    graphed.capture_train_step(mk(0), warmup=1)   # one eager step on frame 0 (= step 0), then capture
    assert gp.LossGeometry.builds == n0 + 1       # built by the eager warm-up step, not again by the capture
    for t in range(1, 5):
        lg = float(graphed.train_step_graphed(mk(t % 3)))
        assert abs(losses_e[t] - lg) < 2e-5 * abs(losses_e[t]), (t, losses_e, lg)
        for a, b in zip(terms_e[t], graphed.last_losses):
            assert abs(a - float(b)) < 2e-5 * abs(a)
    assert gp.LossGeometry.builds == n0 + 1
    for (k, v), (_, w) in zip(eager.model.state_dict().items(), graphed.model.state_dict().items()):
        assert torch.allclose(v, w, rtol=1e-4, atol=2e-6), k


# ------------------------------------------------------------------------------- 5. the Transformer config the section ships with
def test_engine_transformer_with_pinn_section(dev):
    """training_config/pinn-aneurysm.json's model and loss keys (Transformer: hidden 64, 4 heads, 14 + 9 inputs, 3 outputs, no edge
    features) through ``Engine`` on a 3-D tetrahedral mesh"""
    from scipy.spatial import Delaunay

    N = 500
    rng = np.random.default_rng(5)
    pts = rng.random((N, 3)).astype(np.float32)
    cells = Delaunay(pts.astype(np.float64)).simplices
    ei = torch.from_numpy(gp.mesh.faces_to_edges(cells, N))
    nt = rng.choice([0, 0, 0, 4, 5, 6], size=N).astype(np.float32)
    feats = rng.standard_normal((N, 14)).astype(np.float32)
    x = torch.from_numpy(np.concatenate([feats, nt[:, None]], axis=1))
    y = torch.from_numpy((feats[:, :3] + 0.05 * rng.standard_normal((N, 3))).astype(np.float32))
    cfg = {"model": {"type": "transformer", "message_passing_num": 10, "hidden_size": 64, "node_input_size": 14, "output_size": 3,
                     "edge_input_size": 0, "num_heads": 4, "use_silu_activation": False, "use_rope_embeddings": False,
                     "use_gated_attention": False},
           "index": {"feature_index_start": 0, "feature_index_end": 14, "output_index_start": 0, "output_index_end": 3,
                     "node_type_index": 14},
           "loss": LF.SECTIONS["pinn"],
           "training": {"use_spatial_mtp": False, "use_temporal_block": False, "enable_vram_optimizations": False}}
    torch.manual_seed(0)
    eng = harness.Engine(cfg, dev, learning_rate=1e-4, num_steps=100, warmup=4)
    batch = gp.Graph(x=x.to(dev), y=y.to(dev), pos=torch.from_numpy(pts).to(dev), edge_index=ei.to(dev),
                     face=torch.from_numpy(cells.T.astype(np.int64)).to(dev))
    n0 = gp.LossGeometry.builds
    geom = None
    for t in range(2):
        loss = eng.train_step(batch)
        assert torch.isfinite(loss).all(), float(loss)
        assert len(eng.last_losses) == 3 and all(torch.isfinite(v).all() for v in eng.last_losses)
        assert abs(float(sum(eng.last_losses)) - float(loss)) < 1e-5 * abs(float(loss))
        for k, p in eng.sim.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if geom is None:
            geom = batch.mgn_loss_geometry
        assert isinstance(geom, gp.LossGeometry) and batch.mgn_loss_geometry is geom
    assert gp.LossGeometry.builds == n0 + 1


# ------------------------------------------------------------------------------- 6. a moved mesh is a new geometry
def test_moved_positions_on_a_new_batch_object(dev):
    a, b = LF.Case("cyl", dev), LF.Case("cyl_moved", dev)
    assert torch.equal(a.graph.edge_index, b.graph.edge_index) and not torch.equal(a.graph.pos, b.graph.pos)
    for method in LF.METHODS:
        ta, _, _ = LF.section_loss(a, "pinn", method)
        tb, terms_b, _ = LF.section_loss(b, "pinn", method)
        assert rel_err(ta, a.ref(f"{method}.pinn.total")) < FWD_TOL
        assert rel_err(tb, b.ref(f"{method}.pinn.total")) < FWD_TOL
        assert rel_err(terms_b, b.ref(f"{method}.pinn.terms")) < FWD_TOL
        assert rel_err(tb, a.ref(f"{method}.pinn.total")) > 100 * FWD_TOL   # the fixture's two meshes do differ
        assert b.graph.mgn_loss_geometry is not a.graph.mgn_loss_geometry
