"""Cases and references for the aggregation kernels (mgn_csr_build, mgn_topology_build, mgn_segsum, mgn_segsum2,
mgn_segsum2_b16, the hub chunk tables of ops.Topology) -- NumPy / torch on the CPU, nothing of the engine is imported.

The contract of the family is an ORDER: a segment is summed sequentially in k order, k ascending in edge id, in fp32 from +0
(CPU ``index_add_``).  seq32 restates exactly that, two_level restates the hub path (chunks of 1024 rows summed by seq32, the
chunk rows of a node summed by seq32), so the GPU file (tests/test_hip_agg.py) asserts equality and holds no tolerance.  The one
bound here is the textbook one of recursive summation, gamma_bound, against fp64.  tests/test_agg_cases_host.py shows on the CPU
that the references agree with ``index_add_`` and that every case has the property it is in the table for."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32, round to nearest
CHUNK = 1024            # ops.HUB_CHUNK, restated (the host test compares the two)
SMALL_SEG = 48          # CSR_SMALL_SEG of csrc/mgn_kernels.hip: longer segments are sorted by a whole workgroup
SORTBIG_GRID = 512      # workgroups of that launch
SCAN_CHUNK = 1024       # elements per trip of the single-block scan
HS = (16, 32, 64, 128)


# ------------------------------------------------------------------------------------------------- references
def _np(a, dt):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dt, copy=False)


def seq32(src, rowptr, perm=None) -> np.ndarray:
    """out[i] = ((+0 + src[p(r)]) + src[p(r + 1)]) + ... over r = rowptr[i] .. rowptr[i + 1] - 1 with p = perm or the identity, every
    addition in fp32.  The loop runs over the position j inside the segment: step j adds row j of every segment longer than j
    (distinct output rows, so the indexed add is one IEEE fp32 addition per element)."""
    src, rp = _np(src, np.float32), _np(rowptr, np.int64)
    pm = None if perm is None else _np(perm, np.int64)
    n = rp.size - 1
    deg = rp[1:] - rp[:-1]
    out = np.zeros((n, src.shape[1]), dtype=np.float32)
    rows = np.arange(n)
    for j in range(int(deg.max()) if n else 0):
        rows = rows[deg[rows] > j]
        k = rp[rows] + j
        out[rows] = out[rows] + src[k if pm is None else pm[k]]
    return out


def sum64(src, rowptr, perm=None):
    """(fp64 segment sums, fp64 sums of magnitudes): the yardstick and the scale of gamma_bound"""
    src, rp = _np(src, np.float64), _np(rowptr, np.int64)
    rows = src[: rp[-1]] if perm is None else src[_np(perm, np.int64)[: rp[-1]]]
    owner = np.repeat(np.arange(rp.size - 1), rp[1:] - rp[:-1])
    s, a = np.zeros((rp.size - 1, src.shape[1])), np.zeros((rp.size - 1, src.shape[1]))
    np.add.at(s, owner, rows)
    np.add.at(a, owner, np.abs(rows))
    return s, a


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def gamma_bound(rowptr, sum_abs) -> np.ndarray:
    """|seq32 - exact| <= gamma_{d-1} sum|v| for a segment of d rows (d - 1 rounded additions; the first one, to +0, is exact):
    Higham, Accuracy and Stability of Numerical Algorithms, section 4.2.  The fp64 yardstick is itself within
    gamma64_{d-1} sum|v| of exact, which the gap between gamma_{d-1} and the first-order (d - 1) u (>= d (d - 1) / 2 u^2, 2^29
    times fp64's unit) covers, so the bound is used against the fp64 sum as it stands.  d <= 1: the bound is 0 and holds."""
    rp = _np(rowptr, np.int64)
    d = rp[1:] - rp[:-1]
    return gamma(np.maximum(d - 1, 0))[:, None] * sum_abs


def chunk_tables(rowptr, chunk=CHUNK):
    """(chunk_rowptr[C + 1], node_chunkptr[n + 1]) by a loop over the nodes: node i owns chunks node_chunkptr[i] ..
    node_chunkptr[i + 1], chunk c covers rows chunk_rowptr[c] .. chunk_rowptr[c + 1]; no chunk is longer than ``chunk`` rows and a
    node without rows owns none"""
    rp = _np(rowptr, np.int64)
    starts, ncp = [], [0]
    for i in range(rp.size - 1):
        b, e = int(rp[i]), int(rp[i + 1])
        while b < e:
            starts.append(b)
            b = min(b + chunk, e)
        ncp.append(len(starts))
    starts.append(int(rp[-1]))
    return np.asarray(starts, dtype=np.int64), np.asarray(ncp, dtype=np.int64)


def two_level(src, rowptr, perm=None, chunk=CHUNK) -> np.ndarray:
    """the hub path: one fp32 row per chunk (seq32), then the chunk rows of each node in order (seq32 again)"""
    crp, ncp = chunk_tables(rowptr, chunk)
    return seq32(seq32(src, crp, perm), ncp, None)


def index_add32(src, key, n) -> np.ndarray:
    """torch.zeros(n, H).index_add_(0, key, src) on the CPU: what the contract names"""
    src = torch.from_numpy(_np(src, np.float32))
    return torch.zeros(n, src.shape[1]).index_add_(0, torch.from_numpy(_np(key, np.int64)), src).numpy()


# ------------------------------------------------------------------------------------------- two-byte rows
def _packed_order():
    """feature held by each element of a two-byte row, from the words of include/mgn_hip.h (mgn_mlp_fwd_args.precision): K-slice
    p at element 32 p; inside it, for g = 0..3: features 32p + 4g .. + 3, then 32p + 16 + 4g .. + 3"""
    order = []
    for p in range(4):
        for g in range(4):
            order += [32 * p + 4 * g + i for i in range(4)]
            order += [32 * p + 16 + 4 * g + i for i in range(4)]
    return np.asarray(order, dtype=np.int64)


PACKED_ORDER = _packed_order()


def bf16_round(x) -> np.ndarray:
    """fp32 values rounded to the nearest bf16 (ties to even), still stored as fp32"""
    return torch.from_numpy(_np(x, np.float32).copy()).to(torch.bfloat16).float().numpy()


def pack_b16(rows) -> np.ndarray:
    """rows [*, 128] of bf16-valued fp32 -> uint16 [*, 128] in the packed feature order (the upper half of each fp32 word)"""
    rows = np.ascontiguousarray(_np(rows, np.float32))
    assert rows.shape[1] == 128
    bits = rows.view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not bf16 values"
    return (bits >> 16).astype(np.uint16)[:, PACKED_ORDER]


def unpack_b16(packed) -> np.ndarray:
    out = np.empty(packed.shape, dtype=np.uint32)
    out[:, PACKED_ORDER] = packed.astype(np.uint32) << 16
    return out.view(np.float32)


# ---------------------------------------------------------------------------------------------- CSR cases
class CsrCase(NamedTuple):
    name: str
    key: np.ndarray          # int64 [E]
    n: int
    facts: dict              # what the case is in the table for (checked by tests/test_agg_cases_host.py)


def _rng(*seed):
    return np.random.default_rng([20240917, *seed])


def scan_seam(n: int) -> CsrCase:
    """about 4 n keys; counts at nodes 1023, 1024 and n - 1 (where they exist), so the carry of the single-block scan crosses a
    seam with something on both sides; a run of empty nodes across a multiple of 1024 where n leaves room for one beside those"""
    rng = _rng(1, n)
    key = rng.integers(0, n, size=4 * n)
    seam = sorted({i for i in (SCAN_CHUNK - 1, SCAN_CHUNK, n - 1) if 0 <= i < n})
    empty = None
    for m in range(2 * SCAN_CHUNK, n, SCAN_CHUNK):     # a later seam with room on both sides
        if m + 8 < n - 1:
            empty = (m - 8, m + 8)
    if empty is not None:
        key = key[(key < empty[0]) | (key >= empty[1])]
    before = (SCAN_CHUNK - 9, SCAN_CHUNK - 1) if n > SCAN_CHUNK else None   # empty nodes right up to the first seam
    if before is not None:
        key = key[(key < before[0]) | (key >= before[1])]
    key = np.concatenate([key, np.repeat(np.asarray(seam, dtype=np.int64), 3)])
    return CsrCase(f"scan_seam_{n}", rng.permutation(key).astype(np.int64), n, dict(seam=seam, empty=empty, before=before))


LADDER_LENGTHS = (0, 1, 2, 47, 48, 49, 255, 256, 257, 513, 0, 512, 3, 0)


def length_ladder() -> CsrCase:
    """segment lengths on both sides of CSR_SMALL_SEG and of the 256-thread stride of the rank sort; edge ids shuffled"""
    rng = _rng(2)
    key = np.repeat(np.arange(len(LADDER_LENGTHS), dtype=np.int64), LADDER_LENGTHS)
    return CsrCase("length_ladder", rng.permutation(key), len(LADDER_LENGTHS), dict(lengths=LADDER_LENGTHS))


def many_big(n: int) -> CsrCase:
    """every segment 49 .. 60 long: n worklist entries for the 512 workgroups of the rank sort"""
    rng = _rng(3, n)
    key = np.repeat(np.arange(n, dtype=np.int64), rng.integers(SMALL_SEG + 1, 61, size=n))
    return CsrCase(f"many_big_{n}", rng.permutation(key), n, dict(min_len=SMALL_SEG + 1, trips=-(-n // SORTBIG_GRID)))


def _mixed_keys():
    rng = _rng(4)
    return np.concatenate([rng.integers(0, 200, size=5000), np.full(300, 57), np.full(49, 199)]).astype(np.int64)


def orderings():
    k = _mixed_keys()
    asc = np.sort(k)
    return [
        CsrCase("ascending", asc, 200, dict(order=1)),
        CsrCase("descending", asc[::-1].copy(), 200, dict(order=-1)),
        CsrCase("all_equal_n1", np.zeros(700, dtype=np.int64), 1, dict(lengths=(700,))),
        CsrCase("n3_all_key1", np.ones(100, dtype=np.int64), 3, dict(lengths=(0, 100, 0))),
        CsrCase("no_edges_n0", np.zeros(0, dtype=np.int64), 0, dict(lengths=())),
        CsrCase("no_edges_n1", np.zeros(0, dtype=np.int64), 1, dict(lengths=(0,))),
        CsrCase("no_edges_n5", np.zeros(0, dtype=np.int64), 5, dict(lengths=(0,) * 5)),
    ]


SEAM_NS = (1023, 1024, 1025, 2048, 2049, 3073)
BIG_NS = (600, 1100)


@functools.lru_cache(maxsize=None)
def csr_cases() -> dict:
    cs = [scan_seam(n) for n in SEAM_NS] + [length_ladder()] + [many_big(n) for n in BIG_NS] + orderings()
    return {c.name: c for c in cs}


def random_src(c: CsrCase) -> np.ndarray:
    """source ids to go with a case's keys as destinations (ops.Topology)"""
    return _rng(6, c.key.size, c.n).integers(0, max(c.n, 1), size=c.key.size).astype(np.int64)


def lengths_of(key, n) -> np.ndarray:
    return np.bincount(key, minlength=n)[:n] if n else np.zeros(0, dtype=np.int64)


# ----------------------------------------------------------------------------------------- segment-sum cases
class SumCase(NamedTuple):
    name: str
    H: int
    n: int
    src: np.ndarray                  # fp32 [R, H]
    rowptr: np.ndarray               # int64 [n + 1]: segments over the rows of src, in order
    rowptr2: np.ndarray              # a second CSR over the same rows ...
    perm2: np.ndarray                # ... through a random permutation
    facts: dict


LADDER_DEGREES = tuple(range(21)) + (31, 32, 33, 1000)
SMALL_DEGREES = (9, 0, 7, 8, 1, 0, 16, 17, 2, 33, 15, 0, 24)     # the first N of these for N below the ladder's length
LADDER_N = 77            # 77 H / 4 is no multiple of 256 for H in 16, 32, 64, 128; two workgroups already at H = 16


@functools.lru_cache(maxsize=None)
def degree_ladder(H: int, n: Optional[int] = None) -> SumCase:
    """degrees around the 8-deep unroll (7, 8, 9, 15, 16, 17, 31, 32, 33), 0 .. 20, one of 1000; an empty first and last
    segment at the ladder's N; the same rows a second time through a random permutation with degrees of their own"""
    n = LADDER_N if n is None else n
    rng = _rng(7, H, n)
    if n >= len(LADDER_DEGREES) + 2:
        mid = np.concatenate([LADDER_DEGREES, rng.integers(0, 13, size=n - len(LADDER_DEGREES) - 2)])
        deg = np.concatenate([[0], rng.permutation(mid), [0]])
    else:
        deg = np.asarray(SMALL_DEGREES[:n])
    assert deg.size == n
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    R = int(rowptr[-1])
    src = rng.standard_normal((R, H)).astype(np.float32)
    deg2 = rng.permutation(deg)
    rowptr2 = np.concatenate([[0], np.cumsum(deg2)]).astype(np.int64)
    return SumCase(f"ladder_H{H}_n{n}", H, n, src, rowptr, rowptr2, rng.permutation(R).astype(np.int64),
                   dict(degrees=tuple(int(d) for d in deg)))


class HubCase(NamedTuple):
    name: str
    d: int
    n: int
    edge_index: np.ndarray           # int64 [2, E]
    hub_in: int                      # node with d incoming edges, a node without incoming edges on each side of it
    hub_out: int                     # node with d outgoing edges, a node without outgoing edges on each side of it


HUB_DEGREES = (1024, 1025, 2048, 2049)


@functools.lru_cache(maxsize=None)
def hub(d: int) -> HubCase:
    """40 nodes: node 7 receives d edges and nodes 6, 8 none; node 21 sends d edges and nodes 20, 22 none; the ordinary nodes
    exchange a few edges each.  No other degree comes near CHUNK, so d alone decides whether the tables exist."""
    rng = _rng(8, d)
    n, hub_in, hub_out = 40, 7, 21
    no_in, no_out = (6, 7, 8), (20, 21, 22)
    dst_ok = np.asarray([i for i in range(n) if i not in no_in])
    src_ok = np.asarray([i for i in range(n) if i not in no_out])
    base = np.stack([rng.choice(src_ok, 150), rng.choice(dst_ok, 150)])
    into = np.stack([rng.choice(src_ok, d), np.full(d, hub_in)])
    outof = np.stack([np.full(d, hub_out), rng.choice(dst_ok, d)])
    ei = np.concatenate([base, into, outof], axis=1)
    return HubCase(f"hub_{d}", d, n, ei[:, rng.permutation(ei.shape[1])].astype(np.int64), hub_in, hub_out)


def hub_rows(d: int, H: int) -> np.ndarray:
    """fp32 rows [E, H] for hub(d), in the order of its edge list"""
    return _rng(9, d, H).standard_normal((hub(d).edge_index.shape[1], H)).astype(np.float32)


def topology_reference(src, dst, n):
    """what ops.Topology holds: the destination CSR, src_s / dst_s in its order, the source CSR over those rows, the degree maxima"""
    from oracle.mgn_oracle import csr_by_key

    src, dst = torch.from_numpy(_np(src, np.int64)), torch.from_numpy(_np(dst, np.int64))
    rp_d, pm_d = csr_by_key(dst, n)
    src_s, dst_s = src[pm_d.long()], dst[pm_d.long()]
    rp_s, pm_s = csr_by_key(src_s, n)
    din = int((rp_d[1:] - rp_d[:-1]).max()) if n else 0
    dout = int((rp_s[1:] - rp_s[:-1]).max()) if n else 0
    return dict(rowptr_dst=rp_d, perm_dst=pm_d, src_s=src_s.to(torch.int32), dst_s=dst_s.to(torch.int32), rowptr_src=rp_s, perm_src=pm_s,
                max_in_degree=din, max_out_degree=dout)
