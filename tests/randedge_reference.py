"""The sparse-regime stream of ``preprocess.add_random_edges`` restated in numpy from its contract (include/mgn_hip.h,
``mgn_randedge``): K = round(E p) // 2 new node pairs that are not yet edges, drawn from a counter-based
Philox stream, accepted in (round, candidate index) order.  Integer work, so the device result is compared bit for bit.  The
only code shared with anything else is ``oracle.mgn_oracle.philox4x32_10`` (pinned by the Random123 known-answer vectors)."""
import numpy as np

from oracle.mgn_oracle import philox4x32_10

ROUNDS = 4
KEY_TWEAK = 0x45444745


def num_pairs(E: int, p: float) -> int:
    return round(E * p) // 2          # Python's round: half to even


def total_pairs(N: int) -> int:
    return N * (N - 1) // 2


def is_sparse(N: int, E: int, K: int) -> bool:
    return 4 * (E + K) <= total_pairs(N)


def default_candidates(N: int, E: int, K: int) -> int:
    return int(1.1 * K / (1 - E / total_pairs(N))) + 64


def occupied_codes(edge_index: np.ndarray, N: int) -> np.ndarray:
    """sorted codes lo * N + hi of the pairs the input holds in either direction (self loops and stray entries: none)"""
    a, b = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    ok = (a >= 0) & (a < N) & (b >= 0) & (b < N) & (a != b)
    return np.unique(np.minimum(a, b)[ok] * np.int64(N) + np.maximum(a, b)[ok])


def draw(N: int, M: int, rnd: int, seed: int, offset: int):
    """(a, b) of the M candidates of round ``rnd``"""
    c = np.arange(M, dtype=np.uint64)
    r0, r1 = philox4x32_10(seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ KEY_TWEAK, c & np.uint64(0xFFFFFFFF), c >> np.uint64(32),
                           np.uint64(rnd), np.uint64(offset & 0xFFFFFFFF))
    a = (r0.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)
    b = (r1.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)
    return a.astype(np.int64), b.astype(np.int64)


def new_pairs(edge_index: np.ndarray, N: int, K: int, seed: int = 0, offset: int = 0, M: int = None):
    """(lo[K'], hi[K']) in acceptance order, K' <= K"""
    E = int(np.asarray(edge_index).shape[1])
    if M is None:
        M = default_candidates(N, E, K)
    taken = set(occupied_codes(edge_index, N).tolist())      # occupied, then also accepted
    lo_out, hi_out = [], []
    for rnd in range(ROUNDS):
        if len(lo_out) >= K:
            break
        a, b = draw(N, M, rnd, seed, offset)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        code = lo * np.int64(N) + hi
        seen_this_round = set()
        accepted = []
        for i in range(M):                                   # candidate order
            if a[i] == b[i]:
                continue
            k = int(code[i])
            if k in taken or k in seen_this_round:
                continue
            seen_this_round.add(k)
            accepted.append(i)
        taken |= seen_this_round
        for i in accepted:
            if len(lo_out) >= K:
                break
            lo_out.append(int(lo[i]))
            hi_out.append(int(hi[i]))
    return np.asarray(lo_out, dtype=np.int64), np.asarray(hi_out, dtype=np.int64)


def add_random_edges_reference(edge_index: np.ndarray, N: int, p: float, seed: int = 0, offset: int = 0, M: int = None):
    """(result int64 [2, E + 2K], short): the input columns, the new pairs (lo, hi), the same reversed; where fewer than K pairs
    were accepted the missing columns hold 0 and ``short`` is True.  K == 0 or N < 2 gives the input back."""
    ei = np.asarray(edge_index, dtype=np.int64)
    E = int(ei.shape[1])
    K = num_pairs(E, p)
    if K == 0 or N < 2:
        return ei, False
    assert is_sparse(N, E, K), "the restatement covers the sparse regime only"
    lo, hi = new_pairs(ei, N, K, seed, offset, M)
    out = np.zeros((2, E + 2 * K), dtype=np.int64)
    out[:, :E] = ei
    n = lo.shape[0]
    out[0, E:E + n], out[1, E:E + n] = lo, hi
    out[0, E + K:E + K + n], out[1, E + K:E + K + n] = hi, lo
    return out, n < K


def check_properties(out, ei, N, K):
    """the contract of section 1 on one result; returns the K new (lo, hi) pairs"""
    E = ei.shape[1]
    assert out.dtype == np.int64 and out.shape == (2, E + 2 * K)
    assert np.array_equal(out[:, :E], ei)                                   # the input first, untouched and in order
    lo, hi = out[0, E:E + K], out[1, E:E + K]
    assert np.array_equal(out[0, E + K:], hi) and np.array_equal(out[1, E + K:], lo)   # then the same pairs reversed
    assert (lo < hi).all() and (lo >= 0).all() and (hi < N).all()           # lo < hi: no self loop
    code = lo * N + hi
    assert np.unique(code).size == K                                        # distinct
    assert not np.isin(code, occupied_codes(ei, N)).any()                # never an edge of the input, in either direction
    return lo, hi
