"""CPU: the host side of ``training.use_spatial_mtp`` -- the module's keys and initial shapes, its CPU path and the fp64 restatement
(tests/mtp_reference.py) against arrays minted from the reference (tests/golden/mtp.npz), the config surface and its refusals, the
Engine wiring on a torch stand-in of the model, and the third header of the C ABI.  Nothing here needs a GPU."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

import capi_layout as CL
import graph_physics_amd as gp
import mtp_reference as MR
from graph_physics_amd import _capi, harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(case):
    m = gp.SpatialMTP1Hop(case.d, num_heads=case.heads, num_layers=case.layers, assume_undirected=case.assume_undirected)
    m.load_state_dict(case.w, strict=True)
    return m


# ------------------------------------------------------------------------------- keys, shapes, weights
def test_state_dict_keys_and_shapes_equal_the_reference():
    g = MR.golden()
    sd = gp.SpatialMTP1Hop(32, num_heads=4, num_layers=2).state_dict()
    assert sorted(sd) == [str(k) for k in g["state_keys"]]
    for k, shape in zip(g["state_keys"], g["state_shapes"]):
        assert list(sd[str(k)].shape) == [int(s) for s in shape if s > 0], k
    assert sd["enc.layers.1.attn.in_proj_weight"].shape == (96, 32)
    # the initialisers are the reference modules': ones for every norm scale, zeros for the attention biases
    assert all(bool((v == 1).all()) for k, v in sd.items() if k.endswith(".scale"))
    assert bool((sd["enc.layers.0.attn.in_proj_bias"] == 0).all()) and bool((sd["enc.layers.0.attn.out_proj.bias"] == 0).all())


@pytest.mark.parametrize("name", ["messy", "directed"])
def test_reference_weights_load_strict(name):
    c = MR.Case(name)
    m = _module(c)
    for k, v in m.state_dict().items():
        assert torch.equal(v, c.w[k]), k


# ------------------------------------------------------------------------------- the CPU path against the reference
@pytest.mark.parametrize("name", MR.CASES)
def test_cpu_path_against_the_reference(name):
    c = MR.Case(name)
    m, head = _module(c), MR.torch_head(c.head)
    H, Hn = c.H.clone().requires_grad_(True), c.H_neigh.clone().requires_grad_(True)
    loss, stats = m(H, c.edge_index, c.centers, head, c.target, H_neigh=Hn if c.has_neigh else None, **c.forward_kwargs())
    grads = {}
    if loss.requires_grad:
        loss.backward()
        grads = {"H": H.grad, "H_neigh": Hn.grad}
        grads.update({"w." + k: p.grad for k, p in m.named_parameters()})
        grads.update({"head." + k: p.grad for k, p in head.named_parameters()})
    seen = MR.check_against_case(c, loss, stats, grads)
    assert (seen > 0) == (name not in ("isolated", "empty"))
    if name == "messy":
        assert float(stats["sp_mtp/pairs"]) == 16 and float(stats["sp_mtp/max_deg"]) == 6 and float(stats["sp_mtp/centers"]) == 5


def test_cpu_cap_keeps_k_distinct_neighbours():
    c = MR.Case("messy")
    m, head = _module(c), MR.torch_head(c.head)
    m.max_neighbors = 3
    loss, stats = m(c.H, c.edge_index, c.centers, head, c.target, H_neigh=c.H_neigh)
    assert float(stats["sp_mtp/pairs"]) == 3 + 3 + 0 + 3 + 2 and float(stats["sp_mtp/max_deg"]) == 3 and bool(torch.isfinite(loss))
    m.max_neighbors = 6   # nothing is cut: the uncapped result, bit for bit
    full = _module(c)(c.H, c.edge_index, c.centers, head, c.target, H_neigh=c.H_neigh)[0]
    assert torch.equal(m(c.H, c.edge_index, c.centers, head, c.target, H_neigh=c.H_neigh)[0], full)


# ------------------------------------------------------------------------------- the fp64 restatement against the reference
@pytest.mark.parametrize("name", MR.CASES)
def test_restatement_against_the_fp64_reference(name):
    c = MR.Case(name)
    r = MR.star_mtp(c.w, c.head, c.H, c.H_neigh if c.has_neigh else None, c.edge_index, c.centers, c.target, c.heads, c.layers,
                    reduction=c.reduction, assume_undirected=c.assume_undirected, row_ptr=c.row_ptr, dst_sorted=c.dst_sorted)
    assert MR.rel(r["loss"], c.f64["loss"]) < 1e-10 or float(c.f64["loss"]) == 0.0 == float(r["loss"])
    for k, v in c.f64.items():
        if k.startswith("stat."):
            assert abs(r["stats"][k[5:]] - float(v)) <= 1e-10 * max(1.0, abs(float(v))), k
        elif k.startswith("g."):
            key = k[2:]
            got = r["g"][key[:-7]][:8] if key.endswith("__rows8") else r["g"][key[:-6]].norm() if key.endswith("__norm") else r["g"][key]
            assert MR.rel(got, v) < 1e-10, (k, MR.rel(got, v))
    assert sorted(r["stats"]) == sorted(k[5:] for k in c.f64 if k.startswith("stat."))


# ------------------------------------------------------------------------------- the config surface
def _cfg(hidden=32, **training):
    cfg = gp.cylinder_config(2, hidden)
    cfg["training"] = dict(cfg["training"], **training)
    return cfg


def test_get_spatial_mtp_defaults_and_refusals():
    assert gp.get_spatial_mtp(gp.cylinder_config(2, 32)) is None
    assert gp.get_spatial_mtp({"model": {"hidden_size": 7}}) is None and gp.get_spatial_mtp(_cfg(use_spatial_mtp=False, spatial_mtp_num_heads=0)) is None
    got = gp.get_spatial_mtp(_cfg(use_spatial_mtp=True))
    assert got == {"spatial_mtp_alpha": 0.20, "spatial_mtp_centers_per_step": 256, "spatial_mtp_num_heads": 4, "spatial_mtp_num_layers": 1,
                   "spatial_mtp_assume_undirected": True, "spatial_mtp_max_neighbors": None}
    got = gp.get_spatial_mtp(_cfg(use_spatial_mtp=True, spatial_mtp_alpha=0.5, spatial_mtp_centers_per_step=7, spatial_mtp_num_heads=8,
                                  spatial_mtp_num_layers=3, spatial_mtp_assume_undirected=False, spatial_mtp_max_neighbors=5))
    assert got == {"spatial_mtp_alpha": 0.5, "spatial_mtp_centers_per_step": 7, "spatial_mtp_num_heads": 8, "spatial_mtp_num_layers": 3,
                   "spatial_mtp_assume_undirected": False, "spatial_mtp_max_neighbors": 5}
    for key in ("spatial_mtp_centers_per_step", "spatial_mtp_num_heads", "spatial_mtp_num_layers", "spatial_mtp_max_neighbors"):
        for bad in (0, -3):
            with pytest.raises(ValueError, match=key):
                gp.get_spatial_mtp(_cfg(use_spatial_mtp=True, **{key: bad}))
    with pytest.raises(ValueError, match="spatial_mtp_num_heads"):
        gp.get_spatial_mtp(_cfg(use_spatial_mtp=True, spatial_mtp_num_heads=3))    # does not divide 32
    with pytest.raises(ValueError, match="hidden_size"):
        gp.get_spatial_mtp(_cfg(hidden=48, use_spatial_mtp=True))
    with pytest.raises(ValueError, match="hidden_size"):
        gp.get_spatial_mtp(_cfg(hidden=256, use_spatial_mtp=True))


# ------------------------------------------------------------------------------- the Engine on the CPU
def _torch_model(param, only_processor=False):
    m = param["model"]
    return MR.TorchEPD(m["message_passing_num"], m["node_input_size"] + 9, m["edge_input_size"], m["output_size"], m["hidden_size"])


def _batch(n_graphs=2, n_nodes=60, seed=3):
    g = gp.collate([gp.cylinder_mesh(n_nodes, seed + i) for i in range(n_graphs)])
    rng = np.random.default_rng(seed)
    g.y = g.x[:, :2] + torch.from_numpy(0.1 * rng.standard_normal((g.x.shape[0], 2)).astype(np.float32))
    return g


def _cpu_engine(monkeypatch, **training):
    monkeypatch.setattr(harness, "get_model", _torch_model)
    torch.manual_seed(5)
    return harness.Engine(_cfg(**training), torch.device("cpu"), learning_rate=1e-3, warmup=1)


def test_engine_step_adds_alpha_times_the_auxiliary_loss(monkeypatch):
    eng = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_alpha=0.3, spatial_mtp_num_layers=2)
    mtp = eng.spatial_mtp
    assert isinstance(mtp, gp.SpatialMTP1Hop) and mtp.d_model == 32 and mtp.num_layers == 2 and eng.mtp["spatial_mtp_alpha"] == 0.3
    opt_params = {id(p) for grp in eng.opt.param_groups for p in grp["params"]}
    assert all(id(p) in opt_params for p in mtp.parameters()) and all(id(p) in opt_params for p in eng.sim.parameters())
    assert len(opt_params) == len(list(eng.sim.parameters())) + len(list(mtp.parameters()))
    assert len(eng.model.decode_module._forward_pre_hooks) == 1 and len(eng.model.nodes_encoder._forward_hooks) == 1
    batch = _batch()
    N = batch.x.shape[0]
    centers = torch.tensor([0, 7, 61, N - 1, 33, 90])
    # the two parts, computed separately on the same weights and the same normaliser state (a first step accumulates it)
    eng.sim.train()
    node_type = batch.x[:, eng.sim.node_type_index]
    net_out, target, _ = eng.sim(batch)
    H, Hn = eng._mtp_H, eng._mtp_H_neigh
    assert H.shape == (N, 32) and Hn.shape == (N, 32) and H.requires_grad
    base = eng._loss(batch, net_out, target, node_type)
    aux, stats = mtp(H=H, edge_index=batch.edge_index, centers=centers, out_head=eng.model.decode_module, target=target, H_neigh=Hn)
    dec_w = eng.model.decode_module[0].weight
    g_base = torch.autograd.grad(base, dec_w, retain_graph=True)[0]
    g_aux = torch.autograd.grad(aux, dec_w, retain_graph=True)[0]
    before = {k: v.clone() for k, v in mtp.state_dict().items()}
    # a second Engine from the same seed: the same weights, and its first step accumulates the same normaliser statistics
    eng2 = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_alpha=0.3, spatial_mtp_num_layers=2)
    assert all(torch.equal(a, b) for a, b in zip(eng.sim.parameters(), eng2.sim.parameters()))
    assert all(torch.equal(v, before[k]) for k, v in eng2.spatial_mtp.state_dict().items())
    grads = {}
    hook = eng2.model.decode_module[0].weight.register_hook(lambda g: grads.setdefault("dec", g.clone()))
    loss = eng2.train_step(batch, mtp_centers=centers)
    hook.remove()
    assert MR.rel(loss, base.detach() + 0.3 * aux.detach()) < 1e-6
    assert MR.rel(grads["dec"], g_base + 0.3 * g_aux) < 1e-5
    assert eng2._mtp_H is None and eng2._mtp_H_neigh is None                       # cleared after the step
    st = eng2.last_mtp_stats
    assert sorted(st) == sorted(list(MR.STAT_NAMES) + ["sp_mtp/aux_loss"]) and MR.rel(st["sp_mtp/aux_loss"], aux.detach()) < 1e-6
    assert float(st["sp_mtp/centers"]) == 6 and float(st["sp_mtp/pairs"]) == float(stats["sp_mtp/pairs"]) > 0
    changed = [k for k, v in eng2.spatial_mtp.state_dict().items() if not torch.equal(v, before[k])]
    assert len(changed) == len(before), sorted(set(before) - set(changed))           # every MTP weight moved
    # the Engine's own draw: B = min(N, centres per step) distinct nodes, reproducible from the seed
    eng2.train_step(batch)
    assert float(eng2.last_mtp_stats["sp_mtp/centers"]) == min(N, 256)
    # checkpoints carry the module under the reference's prefix
    sd = eng2.state_dict()
    assert {k for k in sd if k.startswith("spatial_mtp.")} == {"spatial_mtp." + k for k in before}
    eng3 = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_num_layers=2)
    eng3.load_state_dict(sd)
    assert all(torch.equal(v, sd["spatial_mtp." + k]) for k, v in eng3.spatial_mtp.state_dict().items())
    assert all(torch.equal(v, sd[k]) for k, v in eng3.sim.state_dict().items())
    eng2.remove_spatial_mtp_hooks()
    assert len(eng2.model.decode_module._forward_pre_hooks) == 0 and len(eng2.model.nodes_encoder._forward_hooks) == 0


class _RenumberingEPD(MR.TorchEPD):
    """the stand-in with a numbering of its own, as the package's models have: rows are permuted on entry and back on exit, and the
    forward records the rank its two hooked modules saw.  ``early``: the rows come back BEFORE the decoder (the temporal block)."""
    early = False

    def forward(self, graph):
        n = graph.x.shape[0]
        order = torch.randperm(n, generator=torch.Generator().manual_seed(n))
        rank = torch.empty_like(order)
        rank[order] = torch.arange(n)
        x, e = self.nodes_encoder(graph.x[order]), self.edges_encoder(graph.edge_attr)
        self.last_node_rank = {"nodes_encoder": rank, "decode_module": None if self.early else rank}
        row, col = rank[graph.edge_index[0]], rank[graph.edge_index[1]]
        for blk in self.processor_list:
            m = blk.edge_block(torch.cat([e, x[col], x[row]], dim=-1))
            agg = torch.zeros_like(x).index_add_(0, col, m)
            x, e = x + blk.node_block(torch.cat([x, agg], dim=-1)), e + m
        return self.decode_module(x[rank]) if self.early else self.decode_module(x)[rank]


@pytest.mark.parametrize("early", [False, True])
def test_engine_uses_the_numbering_the_model_recorded(monkeypatch, early):
    batch = _batch()
    centers = torch.tensor([0, 7, 61, 33, 90, 119])
    plain = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_alpha=0.3)
    plain_w = [p.detach().clone() for p in plain.sim.parameters()]
    want = plain.train_step(batch, mtp_centers=centers)
    monkeypatch.setattr(_RenumberingEPD, "early", early)
    monkeypatch.setattr(MR, "TorchEPD", _RenumberingEPD)
    ren = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_alpha=0.3)
    assert isinstance(ren.model, _RenumberingEPD) and all(torch.equal(p, q) for p, q in zip(plain_w, ren.sim.parameters()))
    got = ren.train_step(batch, mtp_centers=centers)
    assert MR.rel(got, want) < 1e-5
    for k in ("sp_mtp/aux_loss", "sp_mtp/mean_pair_loss", "sp_mtp/pairs"):
        assert MR.rel(ren.last_mtp_stats[k], plain.last_mtp_stats[k]) < 1e-5, k
    # and it matters: without the recorded ranks the branch pairs rows of the model's numbering with the caller's neighbours
    blind = _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_alpha=0.3)
    fwd = blind.model.forward
    blind.model.forward = lambda g: (fwd(g), setattr(blind.model, "last_node_rank", None))[0]
    blind.train_step(batch, mtp_centers=centers)
    assert MR.rel(blind.last_mtp_stats["sp_mtp/aux_loss"], plain.last_mtp_stats["sp_mtp/aux_loss"]) > 1e-5   # (misses the bar above)


def test_engine_without_the_key_is_the_parent_engine(monkeypatch):
    for training in ({}, {"use_spatial_mtp": False, "spatial_mtp_num_heads": 3}):
        eng = _cpu_engine(monkeypatch, **training)
        assert getattr(eng, "spatial_mtp", None) is None and eng.mtp is None and eng.last_mtp_stats is None
        assert len(eng.model.decode_module._forward_pre_hooks) == 0 and len(eng.model.nodes_encoder._forward_hooks) == 0
        n_opt = sum(len(grp["params"]) for grp in eng.opt.param_groups)
        assert n_opt == len(list(eng.sim.parameters()))
        loss = eng.train_step(_batch())
        assert bool(torch.isfinite(loss)) and eng.last_mtp_stats is None
        with pytest.raises(RuntimeError, match="spatial_mtp"):
            eng.load_state_dict({**eng.state_dict(), "spatial_mtp.in_ln.scale": torch.ones(32)})


def test_engine_refusals(monkeypatch):
    with pytest.raises(NotImplementedError, match="use_spatial_mtp.*enable_vram_optimizations"):
        _cpu_engine(monkeypatch, use_spatial_mtp=True, enable_vram_optimizations=True)
    eng = _cpu_engine(monkeypatch, use_spatial_mtp=True)
    with pytest.raises(NotImplementedError, match="capture_train_step.*use_spatial_mtp"):
        eng.capture_train_step(_batch())
    from graph_physics_amd import distributed
    with pytest.raises(NotImplementedError, match="use_spatial_mtp.*partitioned"):
        distributed.check_partitioned_loss(_cfg(use_spatial_mtp=True))
    with pytest.raises(NotImplementedError, match="use_spatial_mtp.*partitioned"):
        distributed.partitioned_loss(torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(3), param=_cfg(use_spatial_mtp=True))
    distributed.check_partitioned_loss(_cfg())                                  # the key off: as before
    with pytest.raises(ValueError, match="spatial_mtp_num_heads"):             # the settings are validated when the Engine is built
        _cpu_engine(monkeypatch, use_spatial_mtp=True, spatial_mtp_num_heads=5)

    class _OnlyProcessor(torch.nn.Module):
        def forward(self, graph):
            return graph.x

    monkeypatch.setattr(harness, "get_model", lambda param, only_processor=False: _OnlyProcessor())
    with pytest.raises(ValueError, match="Spatial MTP requires a processor with an output head"):
        harness.Engine(_cfg(use_spatial_mtp=True), torch.device("cpu"))


# ------------------------------------------------------------------------------- the third header
def _mtp_header():
    with open(os.path.join(REPO, "include", "mgn_hip_mtp.h")) as fh:
        return fh.read()


def _mtp_prototypes():
    """name -> (return class, [argument classes]) of include/mgn_hip_mtp.h, read as test_validate_host.py reads the second header"""
    text = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", CL._strip_comments(_mtp_header()), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\s*\b(mgn_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        assert name not in out
        out[name] = (CL._c_class(ret.strip(), False), [] if params in (["void"], [""]) else [CL._c_class(p, True) for p in params])
    return out


def test_mtp_symbols_match_the_third_header():
    protos = _mtp_prototypes()
    assert sorted(protos) == sorted(_capi.MTP_SYMBOLS) and len(protos) == 7
    assert "struct" not in CL._strip_comments(_mtp_header())
    lib, src = _capi.lib(), CL.unit_source("attn")
    for name, (ret, args) in protos.items():
        res, argtypes = _capi.MTP_SYMBOLS[name]
        assert [CL.ctypes_class(t) for t in argtypes] == args, name
        assert CL.ctypes_class(res) == ret, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(argtypes)
        assert CL.defines(src, name), f"{name} is not defined under mgn_attn.hip"
        assert name not in _capi.SYMBOLS and name not in _capi.EXT_SYMBOLS and _capi._UNIT_OF[name] == "attn"
    assert '#include "mgn_starattn.inc"' in open(os.path.join(CL.CSRC, "mgn_attn.hip")).read()
    assert lib.mgn_star_attn_tile_rows() >= 8
    assert lib.mgn_version() == 136 == _capi.EXPECTED_VERSION and len(_capi.UNITS) == 9 == len(_capi.SOURCES)


def test_new_sources_enter_the_source_hash(tmp_path, monkeypatch):
    inc = os.path.join(CL.CSRC, "mgn_starattn.inc")
    assert inc in _capi.DEPS
    rule = open(os.path.join(CL.CSRC, "Makefile")).read()
    assert "csrc/mgn_starattn.inc" in rule and "include/mgn_hip_mtp.h" in rule
    before = _capi.source_hash()
    for attr, path in (("MTP_HEADER", _capi.MTP_HEADER), ("DEPS", inc)):
        copy = tmp_path / os.path.basename(path)
        shutil.copy(path, copy)
        with open(copy, "a") as fh:
            fh.write("\n")
        monkeypatch.setattr(_capi, attr, str(copy) if attr == "MTP_HEADER" else [d for d in _capi.DEPS if d != inc] + [str(copy)])
        assert _capi.source_hash() != before, attr
        monkeypatch.undo()
    assert _capi.source_hash() == before


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _capi.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)     # a non-null pointer that is never dereferenced: every call is refused
    big = 0x7FFFFFFF // 384 + 1
    calls = {
        "mgn_star_attn_fwd": [lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 48, 4, p, p, None), lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 256, 4, p, p, None),
                              lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 32, 3, p, p, None), lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 16, 32, p, p, None),
                              lambda: lib.mgn_star_attn_fwd(None, p, 5, 1, 32, 4, p, p, None), lambda: lib.mgn_star_attn_fwd(p, None, 5, 1, 32, 4, p, p, None),
                              lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 32, 4, None, p, None), lambda: lib.mgn_star_attn_fwd(p, p, 5, 1, 32, 4, p, None, None),
                              lambda: lib.mgn_star_attn_fwd(p, p, big, 1, 32, 4, p, p, None), lambda: lib.mgn_star_attn_fwd(p, p, -1, 1, 32, 4, p, p, None)],
        "mgn_star_attn_bwd": [lambda: lib.mgn_star_attn_bwd(p, p, p, p, p, 5, 1, 48, 4, p, None), lambda: lib.mgn_star_attn_bwd(p, p, p, p, p, 5, 1, 64, 5, p, None),
                              lambda: lib.mgn_star_attn_bwd(None, p, p, p, p, 5, 1, 32, 4, p, None), lambda: lib.mgn_star_attn_bwd(p, p, p, p, p, 5, 1, 32, 4, None, None),
                              lambda: lib.mgn_star_attn_bwd(p, p, p, None, p, 5, 1, 32, 4, p, None), lambda: lib.mgn_star_attn_bwd(p, p, p, p, p, big, 1, 32, 4, p, None)],
        "mgn_star_pack": [lambda: lib.mgn_star_pack(p, p, p, p, None, p, p, p, 9, 2, 5, 48, 0, p, p, p, p, p, p, p, p, None),
                          lambda: lib.mgn_star_pack(p, p, p, p, None, None, p, p, 9, 2, 5, 32, 0, p, p, p, p, p, p, p, p, None),
                          lambda: lib.mgn_star_pack(p, p, p, p, None, p, p, p, 9, 2, 5, 32, 0, p, p, p, p, p, p, None, p, None),
                          lambda: lib.mgn_star_pack(p, p, p, p, None, p, p, p, 9, 6, 5, 32, 0, p, p, p, p, p, p, p, p, None),
                          lambda: lib.mgn_star_pack(p, p, p, p, None, p, p, p, 9, 2, big, 32, 0, p, p, p, p, p, p, p, p, None)],
        "mgn_star_offsets": [lambda: lib.mgn_star_offsets(None, p, 9, 2, 0, p, p, p, None), lambda: lib.mgn_star_offsets(p, None, 9, 2, 0, p, p, p, None),
                             lambda: lib.mgn_star_offsets(p, p, 9, 2, 0, None, p, p, None), lambda: lib.mgn_star_offsets(p, p, -1, 2, 0, p, p, p, None),
                             lambda: lib.mgn_star_offsets(p, p, 9, big, 0, p, p, p, None)],
        "mgn_star_cap": [lambda: lib.mgn_star_cap(p, p, p, 9, 2, 0, 1, 0, p, None), lambda: lib.mgn_star_cap(p, p, p, 9, 2, 4, 1, 0, None, None),
                         lambda: lib.mgn_star_cap(None, p, p, 9, 2, 4, 1, 0, p, None)],
        "mgn_star_loss": [lambda: lib.mgn_star_loss(p, p, p, p, 9, 2, 5, 0, 0, p, p, None), lambda: lib.mgn_star_loss(p, p, p, p, 9, 2, 5, 33, 0, p, p, None),
                          lambda: lib.mgn_star_loss(p, p, p, p, 9, 2, 5, 2, 2, p, p, None), lambda: lib.mgn_star_loss(p, p, p, p, 9, 2, 2, 2, 0, p, p, None),
                          lambda: lib.mgn_star_loss(None, p, p, p, 9, 2, 5, 2, 0, p, p, None), lambda: lib.mgn_star_loss(p, p, p, p, 9, 2, 5, 2, 0, p, None, None)],
    }
    assert sorted(calls) == sorted(n for n in _capi.MTP_SYMBOLS if n != "mgn_star_attn_tile_rows")
    for name, cases in calls.items():
        for i, fn in enumerate(cases):
            assert lib.mgn_head_axis_attn_fwd(None, None, None, 4, 30, 4, None, None, None) == 1   # another refusal of the unit overwrites the text
            assert b"mgn_head_axis_attn_fwd" in lib.mgn_attn_last_error()
            assert fn() == 1, (name, i)
            text = lib.mgn_attn_last_error().decode()
            assert text.startswith(name + ": "), (name, i, text)
            with pytest.raises(RuntimeError) as e:
                _capi.check(1, name)
            assert str(e.value) == f"{name} failed (code 1): {text}"
    # nothing to do: 0 without a launch (null pointers are never touched)
    assert lib.mgn_star_attn_fwd(None, None, 0, 0, 32, 4, None, None, None) == 0
    assert lib.mgn_star_attn_bwd(None, None, None, None, None, 0, 0, 32, 4, None, None) == 0
    assert lib.mgn_star_pack(None, None, None, None, None, None, None, None, 9, 0, 0, 32, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.mgn_star_cap(p, p, p, 9, 0, 4, 1, 0, p, None) == 0
