"""CPU: the references and cases of tests/agg_cases.py stand on their own -- seq32 is CPU ``index_add_`` bit for bit and inside
the textbook bound of recursive summation against fp64, two_level is the hub path and differs from the one-level sum where it
should, ops._chunk_csr (plain torch, run here on CPU tensors) builds the tables the Python loop builds, pack_b16 is the order
the header gives, and every case has the property it is in the table for.  Conditions on inputs, not measurements."""
import numpy as np
import pytest
import torch

import agg_cases as AC
from graph_physics_amd import ops


def _hub_parts(d, H):
    c = AC.hub(d)
    t = AC.topology_reference(c.edge_index[0], c.edge_index[1], c.n)
    m = AC.hub_rows(d, H)
    return c, t, m, m[t["perm_dst"].long().numpy()]     # rows in edge order and in dst-sorted order


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("n", [None, 1, 8, 13])
@pytest.mark.parametrize("H", AC.HS)
def test_seq32_is_index_add_on_the_ladder(H, n):
    c = AC.degree_ladder(H, n)
    key = np.repeat(np.arange(c.n), np.diff(c.rowptr))
    assert np.array_equal(AC.seq32(c.src, c.rowptr), AC.index_add32(c.src, key, c.n))


@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_seq32_is_index_add_on_the_hub_graphs(d):
    """both CSRs of a topology: a stable grouping keeps ascending row order inside a segment, which is the order index_add_ sums in"""
    c, t, m, ms = _hub_parts(d, 16)
    assert np.array_equal(AC.seq32(ms, t["rowptr_dst"]), AC.index_add32(m, c.edge_index[1], c.n))
    assert np.array_equal(AC.seq32(ms, t["rowptr_src"], t["perm_src"]), AC.index_add32(ms, t["src_s"], c.n))


def _inside(got, src, rowptr, perm):
    s64, a64 = AC.sum64(src, rowptr, perm)
    return bool((np.abs(got.astype(np.float64) - s64) <= AC.gamma_bound(rowptr, a64)).all())


@pytest.mark.parametrize("H", AC.HS)
def test_seq32_inside_the_gamma_bound_on_the_ladder(H):
    for n in (None, 1, 8, 13):
        c = AC.degree_ladder(H, n)
        assert _inside(AC.seq32(c.src, c.rowptr), c.src, c.rowptr, None)
        assert _inside(AC.seq32(c.src, c.rowptr2, c.perm2), c.src, c.rowptr2, c.perm2)


@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_seq32_inside_the_gamma_bound_on_the_hub_graphs(d):
    c, t, m, ms = _hub_parts(d, 128)
    assert _inside(AC.seq32(ms, t["rowptr_dst"]), ms, t["rowptr_dst"], None)
    assert _inside(AC.seq32(ms, t["rowptr_src"], t["perm_src"]), ms, t["rowptr_src"], t["perm_src"])


def test_gamma_bound_is_zero_for_one_row_and_u_for_two():
    b = AC.gamma_bound(np.asarray([0, 0, 1, 3]), np.ones((3, 1)))
    assert b[0, 0] == 0.0 and b[1, 0] == 0.0 and b[2, 0] == AC.U / (1 - AC.U)


@pytest.mark.parametrize("H", [16, 128])
def test_two_level_is_seq32_without_a_long_segment(H):
    c = AC.degree_ladder(H)
    assert max(c.facts["degrees"]) <= AC.CHUNK
    assert np.array_equal(AC.two_level(c.src, c.rowptr), AC.seq32(c.src, c.rowptr))
    assert np.array_equal(AC.two_level(c.src, c.rowptr2, c.perm2), AC.seq32(c.src, c.rowptr2, c.perm2))


@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_two_level_differs_from_seq32_where_a_second_chunk_is_summed(d):
    """1024: one chunk.  1025: chunks of 1024 and 1, and ((+0 + c0) + c1) is the sequential sum itself.  From 2048 the second
    chunk is a sum of its own and the association differs: an implementation that ignored the tables would not pass there."""
    c, t, m, ms = _hub_parts(d, 128)
    for rp, pm, h in ((t["rowptr_dst"], None, c.hub_in), (t["rowptr_src"], t["perm_src"], c.hub_out)):
        one, two = AC.seq32(ms, rp, pm), AC.two_level(ms, rp, pm)
        others = np.arange(c.n) != h
        assert np.array_equal(one[others], two[others])
        assert np.array_equal(one[h], two[h]) == (d <= AC.CHUNK + 1), d


# ------------------------------------------------------------------------------------------- chunk tables
def test_chunk_constant_is_the_engines():
    assert AC.CHUNK == ops.HUB_CHUNK


@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_chunk_csr_equals_the_python_loop(d):
    c = AC.hub(d)
    t = AC.topology_reference(c.edge_index[0], c.edge_index[1], c.n)
    for rp, h, empty in ((t["rowptr_dst"], c.hub_in, (c.hub_in - 1, c.hub_in + 1)), (t["rowptr_src"], c.hub_out, (c.hub_out - 1, c.hub_out + 1))):
        crp, ncp = ops._chunk_csr(rp)
        want_crp, want_ncp = AC.chunk_tables(rp)
        assert crp.dtype == torch.int32 and ncp.dtype == torch.int32
        assert np.array_equal(crp.numpy(), want_crp) and np.array_equal(ncp.numpy(), want_ncp)
        lens = np.diff(want_crp)[want_ncp[h]:want_ncp[h + 1]]
        assert int(rp[h + 1] - rp[h]) == d
        assert list(lens) == {1024: [1024], 1025: [1024, 1], 2048: [1024, 1024], 2049: [1024, 1024, 1]}[d]
        for z in empty:
            assert int(rp[z + 1] - rp[z]) == 0 and want_ncp[z] == want_ncp[z + 1]
        assert int(np.diff(want_crp).min()) >= 1 and int(want_ncp[-1]) == want_crp.size - 1


def test_chunk_csr_without_rows():
    crp, ncp = ops._chunk_csr(torch.zeros(4, dtype=torch.int32))
    want_crp, want_ncp = AC.chunk_tables(np.zeros(4, dtype=np.int64))
    assert np.array_equal(crp.numpy(), want_crp) and np.array_equal(ncp.numpy(), want_ncp) and crp.numel() == 1


# ------------------------------------------------------------------------------------------ two-byte rows
def test_pack_b16_is_the_headers_order():
    assert sorted(AC.PACKED_ORDER.tolist()) == list(range(128))
    element_of = np.empty(128, dtype=np.int64)
    element_of[AC.PACKED_ORDER] = np.arange(128)
    for f, e in ((0, 0), (4, 8), (16, 4), (20, 12), (31, 31), (32, 32)):
        assert element_of[f] == e, (f, element_of[f], e)
    f = np.arange(128)
    assert np.array_equal(element_of, 32 * (f // 32) + 8 * ((f % 16) // 4) + 4 * ((f % 32) // 16) + f % 4)


def test_pack_b16_round_trips():
    rows = AC.bf16_round(np.random.default_rng(0).standard_normal((5, 128)).astype(np.float32))
    p = AC.pack_b16(rows)
    assert p.dtype == np.uint16 and p.shape == (5, 128)
    assert np.array_equal(AC.unpack_b16(p), rows)
    one = np.zeros((1, 128), dtype=np.float32)
    one[0, 20] = 1.0
    assert np.flatnonzero(AC.pack_b16(one)[0]).tolist() == [12] and AC.pack_b16(one)[0, 12] == 0x3F80
    with pytest.raises(AssertionError, match="not bf16"):
        AC.pack_b16(np.full((1, 128), 1.0 + 2.0 ** -20, dtype=np.float32))


# --------------------------------------------------------------------------------- the cases are what they say
def test_case_names():
    names = set(AC.csr_cases())
    assert {f"scan_seam_{n}" for n in (1023, 1024, 1025, 2048, 2049, 3073)} <= names
    assert {"length_ladder", "many_big_600", "many_big_1100", "ascending", "descending", "all_equal_n1", "n3_all_key1",
            "no_edges_n0", "no_edges_n1", "no_edges_n5"} <= names
    assert max(c.key.size for c in AC.csr_cases().values()) <= 70_000


@pytest.mark.parametrize("n", AC.SEAM_NS)
def test_scan_seam_has_counts_at_the_seam(n):
    c = AC.csr_cases()[f"scan_seam_{n}"]
    cnt = AC.lengths_of(c.key, c.n)
    assert c.n == n and 3.5 * n <= c.key.size <= 4.1 * n and c.key.min() >= 0 and c.key.max() == n - 1
    assert set(c.facts["seam"]) == {i for i in (1023, 1024, n - 1) if i < n}
    for i in c.facts["seam"]:
        assert cnt[i] >= 3
    if n > 1024:      # counts on both sides of the first seam, and empty nodes right up to it
        assert cnt[:1024].sum() > 0 and cnt[1024:].sum() > 0
        a, b = c.facts["before"]
        assert b == 1023 and not cnt[a:b].any()
    if n == 3073:     # the one size with room for an empty run across a later seam
        a, b = c.facts["empty"]
        assert a < 2048 < b and not cnt[a:b].any() and cnt[a - 1] > 0 and cnt[b] > 0
    else:
        assert c.facts["empty"] is None


def test_length_ladder_has_the_lengths():
    c = AC.csr_cases()["length_ladder"]
    cnt = AC.lengths_of(c.key, c.n)
    assert tuple(cnt) == AC.LADDER_LENGTHS
    assert {0, 1, 2, 47, 48, 49, 255, 256, 257, 513} <= set(cnt.tolist())
    assert AC.SMALL_SEG == 48 and cnt[0] == 0 and cnt[-1] == 0
    assert not np.array_equal(c.key, np.sort(c.key))     # shuffled edge ids


@pytest.mark.parametrize("n", AC.BIG_NS)
def test_many_big_fills_the_worklist_more_than_once(n):
    c = AC.csr_cases()[f"many_big_{n}"]
    cnt = AC.lengths_of(c.key, c.n)
    assert cnt.min() >= 49 and cnt.max() <= 60
    big = int((cnt > AC.SMALL_SEG).sum())
    assert big > AC.SORTBIG_GRID and c.facts["trips"] == -(-big // AC.SORTBIG_GRID) >= 2
    if n == 1100:
        assert big > 2 * AC.SORTBIG_GRID and c.facts["trips"] == 3


def test_orderings():
    cs = AC.csr_cases()
    a, d = cs["ascending"], cs["descending"]
    assert (np.diff(a.key) >= 0).all() and (np.diff(d.key) <= 0).all() and np.array_equal(a.key, d.key[::-1])
    assert AC.lengths_of(a.key, a.n).max() > AC.SMALL_SEG and AC.lengths_of(a.key, a.n).min() <= AC.SMALL_SEG
    for name in ("all_equal_n1", "n3_all_key1", "no_edges_n0", "no_edges_n1", "no_edges_n5"):
        c = cs[name]
        assert tuple(AC.lengths_of(c.key, c.n)) == c.facts["lengths"] and len(c.facts["lengths"]) == c.n
    assert cs["all_equal_n1"].key.size > 2 * 256     # three strides of the rank sort in one segment


@pytest.mark.parametrize("H", AC.HS)
def test_degree_ladder_has_the_degrees(H):
    c = AC.degree_ladder(H)
    deg = np.diff(c.rowptr)
    assert set(range(21)) | {31, 32, 33, 1000} <= set(deg.tolist())
    assert deg[0] == 0 and deg[-1] == 0 and c.src.shape == (c.rowptr[-1], H)
    assert (c.n * H // 4) % 256 != 0 and c.n * H // 4 > 256           # a ragged last workgroup, more than one workgroup
    assert sorted(np.diff(c.rowptr2).tolist()) == sorted(deg.tolist()) and c.rowptr2[-1] == c.rowptr[-1]
    assert sorted(c.perm2.tolist()) == list(range(c.src.shape[0])) and not np.array_equal(c.perm2, np.arange(c.perm2.size))
    for n in (1, 8, 13):
        s = AC.degree_ladder(H, n)
        assert s.n == n and tuple(np.diff(s.rowptr)) == AC.SMALL_DEGREES[:n]
    assert {7, 8, 9} <= set(AC.SMALL_DEGREES[:8])


@pytest.mark.parametrize("d", AC.HUB_DEGREES)
def test_hub_graph_has_the_hubs(d):
    c = AC.hub(d)
    din, dout = AC.lengths_of(c.edge_index[1], c.n), AC.lengths_of(c.edge_index[0], c.n)
    assert din[c.hub_in] == d and dout[c.hub_out] == d
    assert din[c.hub_in - 1] == 0 and din[c.hub_in + 1] == 0 and dout[c.hub_out - 1] == 0 and dout[c.hub_out + 1] == 0
    assert np.sort(din)[-2] < AC.CHUNK // 2 and np.sort(dout)[-2] < AC.CHUNK // 2
    assert c.n >= 36 and (din > 0).sum() >= 30 and (dout > 0).sum() >= 30
