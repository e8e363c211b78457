"""CPU: the host side of masked-mesh training -- the numpy restatement (tests/meshmask_reference.py) and the package's CPU path
against arrays minted from the reference (tests/golden/meshmask.npz), the loss identity the GPU tests rest on, the node count
table, the properties of the index draw, the config surface and its refusals, and the C ABI (``exclude`` of ``mgn_loss_args``).
Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_physics_amd as gp
from graph_physics_amd import meshmask as MM, preprocess as PP
import loss_cases
import loss_fixture as LF
import meshmask_reference as MR
from meshmask_fixture import CASES, Case, golden


# ------------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_reference(case):
    c = Case(case)
    a = c.a
    ei, attr, mask = MR.filter_edges_reference(c.edge_index, a["selected"], a["edge_attr"])
    assert ei.dtype == np.int64 and np.array_equal(ei, a["filter.edge_index"]) and np.array_equal(mask, c.mask)
    assert np.array_equal(attr, c.kept_attr) and 0 < mask.sum() < c.E
    fields, mask2 = MR.build_masked_graph_reference(a["x"], a["pos"], c.edge_index, a["edge_attr"], a["selected"])
    assert np.array_equal(mask2, c.mask) and np.array_equal(fields["x"], a["masked.x"]) and np.array_equal(fields["pos"], a["masked.pos"])
    assert np.array_equal(fields["edge_index"], a["filter.edge_index"]) and np.array_equal(fields["edge_attr"], c.kept_attr)
    x, none = MR.reconstruct_reference(c.N, a["lat_x"], a["selected"], a["node_token"])
    assert none is None and np.array_equal(x, a["rec_nodes.x"])
    enc = a["edge_attr"] @ a["enc_w"].T + a["enc_b"]
    x, e = MR.reconstruct_reference(c.N, a["lat_x"], a["selected"], a["node_token"], c.mask, enc, a["lat_e"], a["edge_token"])
    assert np.array_equal(x, a["rec.x"])
    np.testing.assert_allclose(e, a["rec.edge_attr"], rtol=0, atol=4e-6)   # (the Linear's own summation order: a few fp32 ulps of O(1..10) rows)
    assert np.array_equal(e[c.mask], a["lat_e"])
    g = MR.reconstruct_gradients_reference(a["wx"].astype(np.float32), a["selected"], a["we"].astype(np.float32), c.mask)
    assert np.array_equal(g["d_node_token"], a["rec.d_token"]) and np.array_equal(g["d_node_token"], a["rec_nodes.d_token"])
    assert np.array_equal(g["d_edge_token"], a["rec.d_edge_token"])
    assert np.array_equal(g["d_latent_x"], a["wx"][a["selected"]]) and np.array_equal(g["d_latent_edge_attr"], a["we"][c.mask])
    np.testing.assert_allclose(g["d_encoded_edge_attr"].T @ a["edge_attr"], a["rec.d_enc_w"], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------- the package's CPU path against the reference
@pytest.mark.parametrize("case", CASES)
def test_cpu_path_against_the_reference(case):
    c = Case(case)
    sel = c.t("selected")
    ei, attr, mask = gp.filter_edges(torch.from_numpy(c.edge_index), sel, c.t("edge_attr"))
    assert ei.dtype == torch.int64 and torch.equal(ei, c.t("filter.edge_index", torch.int64))
    assert mask.dtype == torch.bool and torch.equal(mask, torch.from_numpy(c.mask)) and torch.equal(attr, torch.from_numpy(c.kept_attr))
    ei2, none, _ = gp.filter_edges(torch.from_numpy(c.edge_index), sel, num_nodes=c.N)
    assert none is None and torch.equal(ei2, ei)

    g = c.graph()
    y = g.y
    mg, edges_mask = gp.build_masked_graph(g, sel)
    assert mg is g and mg.y is y and torch.equal(edges_mask, mask)
    assert torch.equal(mg.x, c.t("masked.x")) and torch.equal(mg.pos, c.t("masked.pos"))
    assert torch.equal(mg.edge_index, ei) and torch.equal(mg.edge_attr, attr)

    wx, we = c.t("wx", torch.float32), c.t("we", torch.float32)
    lat_x = c.t("lat_x").requires_grad_(True)
    tok = torch.nn.Parameter(c.t("node_token").clone())
    full = gp.Graph(x=c.t("full_x"), pos=c.t("pos"), edge_index=torch.from_numpy(c.edge_index))
    rec = gp.reconstruct_graph(full, gp.Graph(x=lat_x), sel, tok, edges_mask)
    assert rec is not full and rec.edge_attr is None and torch.equal(rec.x, c.t("rec_nodes.x")) and torch.equal(full.x, c.t("full_x"))
    (wx * rec.x).sum().backward()
    assert torch.equal(tok.grad, c.t("rec_nodes.d_token")) and torch.equal(lat_x.grad, wx[sel])

    lat_x, lat_e = c.t("lat_x").requires_grad_(True), c.t("lat_e").requires_grad_(True)
    tok, etok = torch.nn.Parameter(c.t("node_token").clone()), torch.nn.Parameter(c.t("edge_token").clone())
    enc = c.encoder()
    full.edge_attr = c.t("edge_attr")
    rec = gp.reconstruct_graph(full, gp.Graph(x=lat_x, edge_attr=lat_e), sel, tok, edges_mask, edge_encoder=enc, edge_mask_token=etok)
    assert torch.equal(rec.x, c.t("rec.x")) and torch.equal(rec.edge_attr, c.t("rec.edge_attr")) and torch.equal(full.edge_attr, c.t("edge_attr"))
    ((wx * rec.x).sum() + (we * rec.edge_attr).sum()).backward()
    assert torch.equal(tok.grad, c.t("rec.d_token")) and torch.equal(etok.grad, c.t("rec.d_edge_token"))
    assert torch.equal(lat_x.grad, wx[sel]) and torch.equal(lat_e.grad, we[edges_mask])
    assert torch.equal(enc.weight.grad, c.t("rec.d_enc_w"))


def _loss_inputs(c):
    graph = gp.Graph(pos=c.t("pos"), face=c.t("face", torch.int64), edge_index=torch.from_numpy(c.edge_index))
    net, tgt, pre, std, mean = (c.t(k) for k in ("net", "tgt", "pre", "std", "mean"))
    return graph, dict(target=tgt, network_output=net, masks=list(LF.MASKS), network_output_physical=pre + (net * std + mean),
                       target_physical=pre + (tgt * std + mean))


@pytest.mark.parametrize("method", LF.METHODS)
@pytest.mark.parametrize("case", CASES)
def test_losses_with_selected_indexes_against_the_reference(case, method):
    c = Case(case)
    graph, kw = _loss_inputs(c)
    want, want9 = c.a[f"{method}.values_selected"], c.a[f"{method}.values_type9"]
    # the identity the GPU tests rest on, on the reference's own numbers: leaving rows S out of the mean IS giving them a type
    # that no mask selects
    assert np.array_equal(want, want9)
    plain = LF.Case("messy", torch.device("cpu")).ref(f"{method}.values").numpy() if case == "messy" else None
    if plain is not None:
        assert not np.any(want == plain)   # ... and it is not the loss without the argument
    left_out = c.t("left_out")
    type9 = c.t("node_type").clone()
    type9[left_out] = 9.0
    assert np.array_equal(MR.loss_row_mask(c.a["node_type"], LF.MASKS, c.a["left_out"]), MR.loss_row_mask(type9.numpy(), LF.MASKS))
    for i, name in enumerate(LF.LOSS_ORDER):
        loss = gp.LossType[name].value()
        got = float(loss(graph=graph, node_type=c.t("node_type"), selected_indexes=left_out, gradient_method=method, **kw))
        got9 = float(loss(graph=graph, node_type=type9, gradient_method=method, **kw))
        err = abs(got - float(want[i])) / abs(float(want[i]))
        print(f"{case} {method} {name}: {got:.8e} vs {float(want[i]):.8e}  rel {err:.2e}")
        assert err < loss_cases.FWD_TOL and abs(got9 - float(want[i])) < loss_cases.FWD_TOL * abs(float(want[i]))
    # MultiLoss hands the argument on; out-of-range and repeated entries change nothing; an empty tensor is no argument
    ml = gp.MultiLoss([gp.L2Loss(), gp.GradientL2Loss(), gp.DivergenceL1Loss()], [0.5, 0.25, 2.0])
    total, terms = ml(graph=graph, node_type=c.t("node_type"), selected_indexes=left_out, gradient_method=method, return_all_losses=True, **kw)
    for t, (i, w) in zip(terms, ((0, 0.5), (3, 0.25), (6, 2.0))):
        assert abs(float(t) - w * float(want[i])) < loss_cases.FWD_TOL * w * abs(float(want[i]))
    noisy = torch.cat([left_out, left_out[:3], torch.tensor([-1, c.N, c.N + 100])])
    assert float(ml(graph=graph, node_type=c.t("node_type"), selected_indexes=noisy, gradient_method=method, **kw)) == float(total)
    none = ml(graph=graph, node_type=c.t("node_type"), gradient_method=method, **kw)
    empty = ml(graph=graph, node_type=c.t("node_type"), selected_indexes=torch.empty(0, dtype=torch.int64), gradient_method=method, **kw)
    assert float(none) == float(empty) != float(total)
    assert float(gp.L2Loss()(node_type=c.t("node_type"), selected_indexes=torch.empty(0, dtype=torch.int64), **kw)) == \
        float(gp.L2Loss()(node_type=c.t("node_type"), **kw))


# ------------------------------------------------------------------------------- the draw
def test_node_count_table_is_the_references():
    z = golden()
    for i, n in enumerate(z["k_table.n"]):
        for j, ratio in enumerate(z["k_table.ratio"]):
            want = int(z["k_table"][i, j])
            assert MM.masked_count(int(n), float(ratio)) == want == MR.masked_count(int(n), float(ratio)), (n, ratio)
            idx = gp.get_masked_indexes(gp.Graph(x=torch.zeros(int(n), 1)), float(ratio))
            assert idx.shape == (want,)
    assert MM.masked_count(20, 0.15) == 17 and MM.masked_count(100, 0.15) == 85 and MM.masked_count(7, 0.85) == 1


def test_masked_indexes_properties():
    g = gp.Graph(x=torch.zeros(1923, 4))
    a = gp.get_masked_indexes(g, 0.15, seed=3, offset=11)
    assert a.dtype == torch.int64 and a.device == g.x.device and a.shape == (MM.masked_count(1923, 0.15),) == (1634,)
    assert int(a.min()) >= 0 and int(a.max()) < 1923 and a.unique().numel() == a.numel()
    assert not torch.equal(a, a.sort()[0])                                         # permutation order, not sorted
    assert torch.equal(a, gp.get_masked_indexes(g, 0.15, seed=3, offset=11))       # a (seed, offset) names its draw
    assert not torch.equal(a, gp.get_masked_indexes(g, 0.15, seed=3, offset=12))   # the next step draws anew
    assert not torch.equal(a, gp.get_masked_indexes(g, 0.15, seed=4, offset=11))
    assert torch.equal(gp.get_masked_indexes(g, 0.0, seed=3, offset=11)[:1634], a)  # the first k of ONE permutation
    assert gp.get_masked_indexes(g, 1.0).numel() == 0
    assert MM.mask_seed(0, 0) == 0x4D41534B and MM.mask_seed(1, 2) == (0x9E3779B97F4A7C15 + 2 + 0x4D41534B) % 2 ** 63
    assert 0 <= MM.mask_seed(-1, -1) < 2 ** 63


# ------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [True, "0.15", -0.01, 1.01, float("nan")])
def test_masking_ratio_refusals(bad):
    with pytest.raises(ValueError, match="masking_ratio"):
        PP.build_preprocessing(masking_ratio=bad)
    with pytest.raises(ValueError, match="masking_ratio"):
        gp.get_preprocessing({"index": {"node_type_index": 2}}, torch.device("cpu"), masking_ratio=bad)
    with pytest.raises(ValueError, match="masking_ratio"):
        gp.get_masked_indexes(gp.Graph(x=torch.zeros(4, 1)), bad)


def test_masking_and_partitioning_do_not_combine():
    with pytest.raises(ValueError, match=r"masking_ratio.*partitioning"):
        PP.build_preprocessing(masking_ratio=0.15, partitioning={"num_partitions": 2})
    with pytest.raises(ValueError, match=r"masking_ratio.*use_partitioning"):
        gp.get_preprocessing({"index": {"node_type_index": 2}}, torch.device("cpu"), masking_ratio=0.15, use_partitioning=True,
                             num_partitions=2)
    f = PP.build_preprocessing(masking_ratio=0.15)
    assert f.masking_ratio == 0.15
    assert not hasattr(PP.build_preprocessing(), "masking_ratio") and not hasattr(PP.build_preprocessing(masking_ratio=None), "masking_ratio")
    assert gp.get_preprocessing({"index": {"node_type_index": 2}}, torch.device("cpu"), masking_ratio=0.5).masking_ratio == 0.5
    assert gp.get_preprocessing({"index": {"node_type_index": 2}}, torch.device("cpu"), masking_ratio=0).masking_ratio == 0


def test_reconstruct_refuses_mismatched_widths():
    full = gp.Graph(x=torch.zeros(6, 4))
    sel, mask = torch.tensor([4, 1, 2]), torch.zeros(0, dtype=torch.bool)
    with pytest.raises(ValueError, match="widths"):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(3, 4)), sel, torch.zeros(5), mask)       # the token
    with pytest.raises(ValueError, match="widths"):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(3, 5)), sel, torch.zeros(4), mask)       # the latent rows
    with pytest.raises(ValueError, match="selected indexes"):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(2, 4)), sel, torch.zeros(4), mask)       # one latent row per index
    full.edge_attr = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="edge_encoder"):
        gp.reconstruct_graph(full, gp.Graph(x=torch.zeros(3, 4)), sel, torch.zeros(4), torch.zeros(5, dtype=torch.bool))


def test_selected_indexes_no_longer_raises():
    c = Case("grid")
    _, kw = _loss_inputs(c)
    every = torch.arange(c.N)
    assert torch.isnan(gp.L2Loss()(node_type=c.t("node_type"), selected_indexes=every, **kw))   # no row left: 0 / 0, as the reference
    assert torch.isnan(gp.MultiLoss([gp.L2Loss(), gp.CosineLoss()], [1, 1])(node_type=c.t("node_type"), selected_indexes=every, **kw))


# ------------------------------------------------------------------------------- C ABI
def test_loss_args_carries_exclude_last(tmp_path):
    import capi_layout
    from graph_physics_amd import _capi

    names = [f for f, _ in _capi.LossArgs._fields_]
    assert names[-1] == "exclude" and names[-2] == "invcount"
    assert capi_layout.header_structs()["mgn_loss_args"][-1] == "exclude"
    got = capi_layout.gcc_layout(tmp_path, {"mgn_loss_args": _capi.LossArgs})
    capi_layout.assert_layout(got, "mgn_loss_args", _capi.LossArgs)
    assert _capi.LossArgs().exclude is None                                    # a fresh struct means "no row excluded"
    lib = _capi.lib()
    assert lib.mgn_version() == _capi.EXPECTED_VERSION == 136                  # additive change: the ABI number stays
    a = _capi.LossArgs()
    a.exclude = C.cast(C.create_string_buffer(16), C.c_void_p)                 # validation still comes first: no launch without a GPU
    assert lib.mgn_loss_fwd(C.byref(a), None) == 1 and b"mgn_loss_fwd" in lib.mgn_loss_last_error()
    # the gather job is as it was: the [MASK] rows ride on its existing "an index outside the source is not followed"
    assert [f for f, _ in _capi.GatherJob._fields_] == ["src", "ld_src", "width", "idx", "rows", "dst", "ld_dst", "src_rows"]
