"""CPU: the case table of tests/mlp_cases.py is what it says it is, and the references alone stay inside the bars the GPU
file (tests/test_hip_mlp_matrix.py) holds the engine to -- the fp32 oracle within HALF of them from the fp64 oracle, so
that a failure there is the engine's.  Also the host-side behaviour of ops.MlpFunction that needs no device."""
import pytest
import torch

import graph_physics_amd as gp
import mlp_cases as MC
from conftest import elem_err, rel_err, rms_err
from graph_physics_amd import ops

ALL = [(fam, n) for fam, tab in (("A", MC.FAMILY_A), ("B", MC.FAMILY_B), ("C", MC.FAMILY_C)) for n in tab]
_worst = {}


def _note(fam, act, what, v):
    key = (fam, act, what)
    _worst[key] = max(_worst.get(key, 0.0), v)


@pytest.mark.parametrize("fam,name", ALL, ids=[n for _, n in ALL])
def test_fp32_oracle_within_half_the_bars_of_fp64(fam, name):
    c = MC._find(name)
    r32, r64 = MC.reference(name, torch.float32), MC.reference(name, torch.float64)
    for a, b in zip(r32.out, r64.out):
        r, q, e = rel_err(a, b), rms_err(a, b), elem_err(a, b)
        _note(fam, c.act, "forward", r)
        assert r < 0.5 * MC.FWD_TOL and q < 0.5 * MC.FWD_TOL and e < 0.5 * 100.0 * MC.FWD_TOL, (name, r, q, e)
    for what, pairs in (("input gradient", [(a, b) for a, b in zip(r32.dins, r64.dins) if a is not None]),
                        ("parameter gradients", [(r32.grads[k], r64.grads[k]) for k in r32.grads])):
        for a, b in pairs:
            g = rel_err(a, b)
            _note(fam, c.act, what, g)
            # (ReLU too: a mask flipped between fp32 and fp64 would show as a gap of this size; none does in this table)
            assert g < 0.5 * MC.GRAD_TOL, (name, what, g)


def test_report_worst_reference_gaps():
    """prints the table (pytest -s); runs after the sweep above in file order"""
    for (fam, act, what), v in sorted(_worst.items()):
        print(f"worst fp32-vs-fp64 gap  family {fam}  {act:4s}  {what:20s} {v:.2e}")
    assert all(v == v for v in _worst.values())


def _computed_masks(c):
    m = set()
    if c.fin % 16:
        m.add("in")
    if MC.pad16(c.fin) < c.H:
        m.add("inblk")
    if c.fout % 16:
        m.add("out")
    if MC.pad16(c.fout) < c.H:
        m.add("outblk")
    return m


@pytest.mark.parametrize("name", list(MC.FAMILY_A))
def test_case_masks_what_its_name_says(name):
    c = MC.FAMILY_A[name]
    assert c.name == name and f"_in{c.fin}_" in name and f"_out{c.fout}_" in name and f"_m{c.M}_" in name
    assert _computed_masks(c) == set(c.masks), (name, sorted(_computed_masks(c)), sorted(c.masks))
    assert c.fin <= c.H and c.fout <= c.H and 2 <= c.NL <= 8 and (not c.norm or c.fout == c.H)
    if c.M not in (16, 64):
        assert c.M % 16 != 0                       # rows of the last tile are clamped on load and masked on store
    if c.M <= 48:
        assert (c.M + 15) // 16 < 4                # waves of the only workgroup own no row at all


def test_table_covers_what_it_is_for():
    A = list(MC.FAMILY_A.values())
    for H in MC.HS:
        at = [c for c in A if c.H == H]
        assert {c.M for c in at} >= {1, 15, 16, 17, 63, 64, 65, 257}
        assert {c.NL for c in at} >= {2, 3, 4, 5, 8} and {c.act for c in at} == set(MC.ACTS)
        assert {(c.fin, c.fout) for c in at} >= {(1, 1), (3, 2), (11, 3), (H - 1, H - 1), (H, 3), (H, H), (H, H - 1)}
        assert any(c.norm for c in at) and any(not c.norm and c.fout == H for c in at)
    at = [c for c in A if c.H == 128]
    for route, acts in (("full", {"relu", "silu"}), ("enc", {"relu", "silu"}), ("generic", {"relu", "silu", "gelu"})):
        assert {c.act for c in at if c.route == route} >= acts, route
    assert {c.NL for c in at if c.route == "enc"} == {3, 4}
    assert {c.NL for c in at if c.route == "generic" and c.fin == c.fout == 128 and c.act != "gelu"} >= {5, 8}
    assert any(c.route == "generic" and c.NL == 2 and c.fin < 128 and c.fout == 128 for c in at)
    assert {(c.H, c.NL) for c in MC.FAMILY_B.values()} == {(h, n) for h in (16, 32, 64) for n in (2, 4, 5)} | {(128, 5), (128, 8)}
    assert {c.act for c in MC.FAMILY_B.values() if c.H == 128} == {"relu", "silu"}
    for c in MC.FAMILY_C.values():   # both launches of the block take two tiles per wave, the last wave's tile is ragged
        assert c.N >= MC.MT2_ROWS and c.E >= MC.MT2_ROWS and c.N % 32 and c.E % 32 and c.H in (16, 32)
    assert len(MC.FAMILY_D) == 8 and sum(c.act == "silu" for c in MC.FAMILY_D.values()) == 2


@pytest.mark.parametrize("name", list(MC.FAMILY_B))
def test_block_graph_is_ragged(name):
    c = MC.FAMILY_B[name]
    ei = MC.block_graph(c)
    deg = torch.bincount(ei[1], minlength=c.N)
    assert int(deg[c.N - 1]) == 0 and int(deg.max()) >= 120                      # isolated last node, one long segment
    assert bool((ei[0] == ei[1]).any())                                          # self loop
    assert torch.unique(ei, dim=1).shape[1] < ei.shape[1]                        # duplicates
    assert c.E % 16 != 0 and c.N % 16 != 0


@pytest.mark.parametrize("name", list(MC.FAMILY_D))
def test_bf16_references_agree_to_rounding_decisions(name):
    """the two forward references of the bf16 mode differ by rounding decisions only: a few bf16 ulps (2^-8 each) at the
    tensor's scale on single elements, far less in the RMS sense"""
    mixed, explicit = MC.reference(name, torch.float32, True).out[0], MC.bf16_explicit_forward(name)
    d_rel, d_rms = rel_err(mixed, explicit), rms_err(mixed, explicit)
    print(f"bf16 reference distance  {name:36s} rel {d_rel:.2e}  rms {d_rms:.2e}")
    assert d_rel < 4 * 2.0 ** -8 and d_rms < 2.0 ** -8, (name, d_rel, d_rms)
    assert rel_err(explicit, MC.reference(name, torch.float32).out[0]) > MC.FWD_TOL   # and neither is the fp32 result


def test_padded_buffer_is_contiguous_and_fenced():
    t = torch.arange(12.0).reshape(4, 3)
    p = MC.padded(t)
    assert p.is_contiguous() and torch.equal(p, t)
    assert p.untyped_storage().nbytes() == (4 + MC.PAD_ROWS) * 3 * 4


# ------------------------------------------------------------------- ops.MlpFunction on the host (no device needed)
def test_cpu_tensor_is_refused():
    mlp = gp.build_mlp(3, 16, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp(torch.zeros(4, 3))


def test_depth_above_eight_is_rejected_with_a_message(monkeypatch):
    """the check sits in front of every allocation and launch: with the device test stubbed out it is the first thing a
    CPU call meets (a 9-layer MLP used to die on a ctypes index error inside the launch wrapper)"""
    monkeypatch.setattr(ops, "_require_device", lambda *ts: None)
    mlp = gp.build_mlp(16, 16, 16, nb_of_layers=9)
    with pytest.raises(AssertionError, match="at most 8 layers"):
        mlp(torch.zeros(4, 16))


def test_unsupported_widths_are_rejected_with_a_message(monkeypatch):
    monkeypatch.setattr(ops, "_require_device", lambda *ts: None)
    for fin, H, fout in ((17, 16, 16), (16, 16, 17), (8, 48, 8)):
        with pytest.raises(NotImplementedError, match="not supported by the MI355X engine"):
            gp.build_mlp(fin, H, fout)(torch.zeros(4, fin))
