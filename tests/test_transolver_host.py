"""CPU: the Transolver processor's module tree, its torch-ops path and the fp64 restatement against arrays minted from the reference
(tests/golden/transolver.npz, make_golden_transolver.py); the factory, the Engine's construction and the new refusals."""
import pytest
import torch

import graph_physics_amd as gp
import transolver_reference as TR
from conftest import rel_err
from graph_physics_amd import harness, transolver as TS
from graph_physics_amd.mesh import Graph

CASES = ["rope_gate", "narrow", "temporal", "unified", "clamp"]


@pytest.fixture(scope="module")
def Z():
    return TR.load_golden()


def build(meta, state, dtype=torch.float32):
    mod = gp.TransolverProcessor(message_passing_num=meta["blocks"], node_input_size=meta["n_in"], output_size=meta["n_out"], hidden_size=meta["hidden"],
                                 num_heads=meta["heads"], slice_num=meta["G"], ref=meta["ref"] or 8, unified_pos=bool(meta["ref"]),
                                 use_rope_embeddings=bool(meta["rope"]), use_gated_attention=meta["gate"], rope_pos_dimension=meta["rope"] or 3,
                                 use_temporal_block=meta["temporal"])
    mod.load_state_dict(state, strict=True)
    return mod.to(dtype).train()


def run(mod, T, dtype, dev="cpu"):
    x = T["x"].detach().clone().to(dev, dtype).requires_grad_(True)
    mod.noise_u = [u for u in T["u"]]
    out = mod(Graph(x=x, pos=T["pos"].to(dev, dtype), edge_index=None, edge_attr=None, y=None))
    out.backward(T["dy"].to(dev, dtype))
    return out.detach(), x.grad, {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}


def compare(tag, got, T, g64, err, slack=1.0):
    out, gx, gw = got
    worst = 0.0
    for name, a, b, conv in [("out", out, T["f64.out"], 1e-5), ("g.x", gx, T["f64.g.x"], 2e-5)] + [(k, gw[k], g64[k], 2e-5) for k in g64]:
        e, bd = rel_err(a, b), TR.bound(conv, err[name]) * slack
        worst = max(worst, e / bd)
        assert e < bd, f"{tag} {name}: {e:.3e} >= {bd:.3e}"
    assert set(gw) == set(g64), (set(gw) ^ set(g64))
    print(f"{tag}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_keys_and_shapes_match_the_reference(Z, case):
    meta, T, state, g64, err = TR.unpack_case(Z, case)
    sd = build(meta, state).state_dict()
    assert sorted(sd) == sorted(state)
    assert all(tuple(sd[k].shape) == tuple(state[k].shape) for k in sd)
    assert not any("_noise_step" in k for k in sd)                       # the call counter is not persistent
    assert all("embedding" not in k for k in g64)                        # (the condition is None: no gradient there)


@pytest.mark.parametrize("case", CASES)
def test_no_row_sits_on_the_clamp_point(Z, case):
    _, T, _, _, _ = TR.unpack_case(Z, case)
    assert float((T["tpre"] - TR.CLAMP).abs().min()) > 1e-3
    if case == "clamp":
        frac = (T["tpre"][:, :, 0] < TR.CLAMP).float().mean(dim=1)
        assert bool(((frac > 0.3) & (frac < 0.7)).all())
    u = T["u"]
    assert float(u.min()) == 0.0 and float(u.max()) == 1.0 - 2.0 ** -24   # the planted extremes


@pytest.mark.parametrize("case", CASES)
def test_torch_ops_path_matches_the_reference(Z, case):
    """Measured, worst error / bound: rope_gate 0.184, narrow 0.074, temporal 0.149, unified 0.319, clamp 0.229 (the path takes the row
    maximum off the logits as a constant before the division by the temperature: without that the temperature's gradient is a sum that
    cancels at the size of the logits, and `unified` sat at 1.25 of its bound)."""
    meta, T, state, g64, err = TR.unpack_case(Z, case)
    compare(case + " fp32", run(build(meta, state), T, torch.float32), T, g64, err)


@pytest.mark.parametrize("case", CASES)
def test_torch_ops_path_in_fp64_matches_the_reference(Z, case):
    """the torch-ops path of the module in .double() (its noise formed from the fp32 u in fp32 and widened) must sit on the reference's fp64
    run far inside the fp32 bounds: 1e-3 of the convention"""
    meta, T, state, g64, err = TR.unpack_case(Z, case)
    got = run(build(meta, state, torch.float64), T, torch.float64)
    compare(case + " fp64", got, T, g64, {k: 0.0 for k in err}, slack=1e-3)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_module_pinned_to_the_reference(Z, case):
    """tests/transolver_reference.py itself, on every block's x_mid of a golden case: its slice weights w, its expanded output and its
    gradients for x_mid and every weight of the physics attention against the fp64 module's (which the test above pins to the
    reference's fp64 run).  Two fp64 statements of the same mathematics: 1e-10 of each tensor's largest entry."""
    meta, T, state, _, _ = TR.unpack_case(Z, case)
    mod = build(meta, state, torch.float64)
    for blk in mod.model.blocks:
        blk.Attn.keep_last = True
    mod.noise_u = [u for u in T["u"]]
    mod(Graph(x=T["x"].double(), pos=T["pos"].double(), edge_index=None, edge_attr=None, y=None))   # (forward only: the graph stays)
    N, H, G, C = meta["N"], meta["heads"], meta["G"], meta["hidden"] // meta["heads"]
    worst = 0.0
    for i, blk in enumerate(mod.model.blocks):
        attn = blk.Attn
        xm_m, w_m, out_m = attn.last
        pt, sl = attn.proj_temperature, attn.in_project_slice
        ps = [sl.weight, sl.bias, pt[0].weight, pt[0].bias, pt[2].weight, pt[2].bias, attn.bias, attn.to_q.weight, attn.to_k.weight,
              attn.to_v.weight] + (list(attn.attn_gate.parameters()) if attn.attn_gate is not None else [])
        dOut = torch.randn(N, H * C, dtype=torch.float64, generator=torch.Generator().manual_seed(i))
        g_m = torch.autograd.grad(out_m, [xm_m] + ps, dOut, retain_graph=True)
        xm = xm_m.detach().clone().requires_grad_(True)
        q = [p.detach().clone().requires_grad_(True) for p in ps]
        w, _, tpre = TR.weights(xm.view(N, H, C), q[0], q[1], q[2], q[3], q[4], q[5], q[6], T["u"][i])
        S, norm = TR.aggregate(w, xm.view(N, H, C))
        out = TR.expand(w, TR.tokens(S, norm, q[7], q[8], q[9], gate=tuple(q[10:]) if len(q) > 10 else None)).reshape(N, H * C)
        g_r = torch.autograd.grad(out, [xm] + q, dOut)
        for a, b in [(w, w_m), (out, out_m), (tpre, attn.last_tpre)] + list(zip(g_r, g_m)):
            e = rel_err(a, b)
            worst = max(worst, e)
            assert e < 1e-10, (case, i, e)
        if i == 0:   # the stored fp32 temperatures of the reference's own run belong to the same numbers
            assert rel_err(tpre, T["tpre"][0]) < 1e-5
    print(f"{case}: restatement against the fp64 module, worst {worst:.2e}")


def test_restatement_pieces_agree_with_the_module(Z):
    meta, T, state, _, _ = TR.unpack_case(Z, "clamp")
    mod = build(meta, state, torch.float64)
    attn = mod.model.blocks[0].Attn
    N, H, G, C = 33, meta["heads"], meta["G"], meta["hidden"] // meta["heads"]
    xm = torch.randn(N, H, C, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    u = T["u"][0][:N]
    pt = attn.proj_temperature
    w, t2, tpre = TR.weights(xm, attn.in_project_slice.weight, attn.in_project_slice.bias, pt[0].weight, pt[0].bias, pt[2].weight, pt[2].bias,
                             attn.bias, u)
    S, norm = TR.aggregate(w, xm)
    tok = TR.tokens(S, norm, attn.to_q.weight, attn.to_k.weight, attn.to_v.weight)
    assert rel_err(tok, attn._tokens(S, norm)) < 1e-12
    assert rel_err(tpre, pt(xm).squeeze(-1) + attn.bias.view(1, H)) < 1e-12
    assert rel_err(w.sum(-1), torch.ones(N, H, dtype=torch.float64)) < 1e-12


# ------------------------------------------------------------------------------------------- factory, Engine, refusals
def _config(**model):
    cfg = {"model": {"type": "transolver", "message_passing_num": 2, "hidden_size": 32, "num_heads": 4, "node_input_size": 2, "output_size": 2,
                     "edge_input_size": 3},
           "index": {"feature_index_start": 0, "feature_index_end": 2, "output_index_start": 0, "output_index_end": 2, "node_type_index": 2},
           "training": {}}
    cfg["model"].update(model)
    return cfg


def test_get_transolver_reads_the_reference_defaults():
    m = gp.get_transolver(_config())
    a = m.model.blocks[0].Attn
    assert isinstance(m, gp.TransolverProcessor) and len(m.model.blocks) == 2
    assert (a.slice_num, a.heads, a.dim_head) == (32, 4, 8)
    assert m.model.ref == 8 and not m.model.unified_pos and not m.model.use_rope_embeddings and m.model.temporal_block is None
    assert m.model.preprocess[0].in_features == 2 + gp.NodeType.SIZE
    assert m.model.blocks[0].mlp[0].out_features == 32                                   # mlp_ratio 1
    assert float(a.bias.mean()) == 0.5 and m.noise_seed == 0
    w = a.in_project_slice.weight
    assert torch.allclose(w.t() @ w, torch.eye(8), atol=1e-5)                            # orthogonal initialiser
    assert float(m.model.placeholder.max()) <= 1 / 32
    cfg = _config(slice_num=8, use_rope_embeddings=True, rope_pos_dimension=2, use_gated_attention=True)
    cfg["training"]["use_temporal_block"] = True
    m = gp.get_transolver(cfg)
    assert m.model.temporal_block is not None and m.model.output_proj is not None and m.model.blocks[0].Attn.attn_gate is not None
    with pytest.raises(NotImplementedError, match="transolver"):                         # get_model still refuses, on purpose
        gp.get_model(_config())
    with pytest.raises(ValueError):
        gp.get_transolver({"model": {"type": "epd"}})


def test_construction_refusals():
    with pytest.raises(NotImplementedError, match="dropout"):
        gp.get_transolver(_config(dropout=0.1))
    with pytest.raises(NotImplementedError, match="slice_num"):
        gp.get_transolver(_config(slice_num=65))
    with pytest.raises(NotImplementedError, match="hidden_size"):
        gp.get_transolver(_config(hidden_size=48))
    with pytest.raises(NotImplementedError, match="input columns"):
        gp.get_transolver(_config(unified_pos=True))                                     # 8^3 grid distances: wider than a dense launch
    with pytest.raises(NotImplementedError, match="mlp_ratio"):
        gp.get_transolver(_config(hidden_size=128, mlp_ratio=4))


def test_engine_builds_it_and_refuses_by_name():
    eng = harness.Engine(_config(), torch.device("cpu"), seed=7)
    assert isinstance(eng.model, gp.TransolverProcessor) and eng.model.noise_seed == 7
    assert not any("_noise_step" in k for k in eng.state_dict())
    cfg = _config()
    cfg["training"]["enable_vram_optimizations"] = True
    with pytest.raises(NotImplementedError, match="enable_vram_optimizations"):
        harness.Engine(cfg, torch.device("cpu"))
    gp.set_matrix_precision("fp32")
    cfg = _config()
    cfg["training"]["use_spatial_mtp"] = True
    with pytest.raises(NotImplementedError, match="use_spatial_mtp"):
        harness.Engine(cfg, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="transolver"):
        eng.capture_train_step(None)
    from graph_physics_amd import distributed
    with pytest.raises(NotImplementedError, match="transolver"):
        distributed.check_partitioned_loss(_config())


def test_cpu_noise_counter_and_injection():
    m = gp.get_transolver(_config(slice_num=8)).eval()
    g = Graph(x=torch.randn(20, 2 + gp.NodeType.SIZE), pos=None, edge_index=None, edge_attr=None, y=None)
    with torch.no_grad():
        a, b = m(g), m(g)
        assert int(m.model._noise_step) == 2 and not torch.equal(a, b)                   # noise in eval mode too, new at every call
        u = [torch.rand(20, 4, 8) for _ in range(2)]
        m.noise_u = u
        assert torch.equal(m(g), m(g))
        m.noise_u = u[:1]
        with pytest.raises(ValueError, match="noise_u"):
            m(g)
