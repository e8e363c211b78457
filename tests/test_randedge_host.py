"""CPU: the host side of the random-extra-edges feature (``dataset.new_edges_ratio``) -- the arithmetic of K, M and the regime
predicate, the numpy restatement of the stream (tests/randedge_reference.py) on hand-written graphs and its uniformity, the C
ABI of csrc/mgn_randedge.hip (declared, exported, prototyped; argument checks before any launch) and the config surface.
Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import randedge_reference as RR
from randedge_reference import check_properties

SYMBOLS = ("mgn_randedge_default_candidates", "mgn_randedge_workspace_bytes", "mgn_randedge", "mgn_randedge_last_error")


def ring(n):
    i = np.arange(n)
    return np.concatenate([np.stack([i, (i + 1) % n]), np.stack([(i + 1) % n, i])], axis=1).astype(np.int64)


def test_k_arithmetic_and_regime_predicate():
    from graph_physics_amd import preprocess as P

    assert RR.num_pairs(5, 0.5) == 1 and RR.num_pairs(7, 0.5) == 2         # round(2.5) = 2, round(3.5) = 4: half to even
    assert RR.num_pairs(180082, 0.1) == 9004 and RR.num_pairs(32, 0.5) == 8 and RR.num_pairs(3, 0.1) == 0 and RR.num_pairs(10, 1.0) == 5
    for E, p in ((5, 0.5), (7, 0.5), (180082, 0.1), (0, 1.0), (11, 0.3)):
        assert P.num_random_pairs(E, p) == RR.num_pairs(E, p)
    # 4 (E + K) <= P: the 40-ring (E 80, K 20, P 780) is sparse, the 16-ring (E 32, K 8, P 120) is not ... at p = 0.5
    assert RR.is_sparse(40, 80, 20) and P.random_edges_sparse(40, 80, 20)
    assert not RR.is_sparse(16, 32, 8) and not P.random_edges_sparse(16, 32, 8)
    assert RR.is_sparse(9, 8, 1) and not RR.is_sparse(9, 8, 2)             # P = 36: the boundary itself
    assert P.random_edges_sparse(9, 8, 1) and not P.random_edges_sparse(9, 8, 2)
    assert RR.default_candidates(40, 80, 20) == int(1.1 * 20 / (1 - 80 / 780)) + 64 == 88
    assert P.random_edges_candidates(30160, 180082, 45020) == RR.default_candidates(30160, 180082, 45020)


def test_restatement_on_hand_written_graphs():
    N = 40
    ei = ring(N)
    out, short = RR.add_random_edges_reference(ei, N, 0.5, seed=3, offset=0)
    assert not short
    check_properties(out, ei, N, 20)
    again, _ = RR.add_random_edges_reference(ei, N, 0.5, seed=3, offset=0)
    assert np.array_equal(out, again)                                       # deterministic
    other, _ = RR.add_random_edges_reference(ei, N, 0.5, seed=3, offset=1)
    assert not np.array_equal(out, other)                                   # another offset, another draw
    other, _ = RR.add_random_edges_reference(ei, N, 0.5, seed=4, offset=0)
    assert not np.array_equal(out, other)
    # acceptance order is candidate order: the first accepted pair is the first candidate that is neither a loop nor occupied
    a, b = RR.draw(N, RR.default_candidates(N, 80, 20), 0, 3, 0)
    occ = set(RR.occupied_codes(ei, N).tolist())
    first = next(i for i in range(a.size) if a[i] != b[i] and min(a[i], b[i]) * N + max(a[i], b[i]) not in occ)
    assert (out[0, 80], out[1, 80]) == (min(a[first], b[first]), max(a[first], b[first]))
    # a pair present only as (j, i), j > i, a duplicate and a self loop: (2, 7) stays occupied, the loop occupies nothing
    messy = np.array([[7, 0, 0, 5, 30], [2, 1, 1, 5, 31]], dtype=np.int64)
    assert RR.occupied_codes(messy, N).tolist() == [0 * N + 1, 2 * N + 7, 30 * N + 31]
    for off in range(50):
        out, short = RR.add_random_edges_reference(messy, N, 1.0, seed=1, offset=off)
        check_properties(out, messy, N, 2)
    # K == 0 and N < 2: the input comes back
    assert RR.add_random_edges_reference(ei, N, 0.0)[0] is ei and RR.add_random_edges_reference(ei[:, :3], 1, 1.0)[0].shape == (2, 3)
    # too few candidates: the result is short, the missing columns hold 0
    out, short = RR.add_random_edges_reference(ei, N, 0.5, seed=3, M=1)
    assert short and out.shape == (2, 120) and (out[:, 80 + 4:100] == 0).all() and (out[:, 100 + 4:] == 0).all()


def test_later_rounds_skip_what_earlier_rounds_accepted():
    N = 300
    ei = ring(N)
    K = RR.num_pairs(ei.shape[1], 0.5)
    M = K // 2                                                              # rounds 0 .. 2 at least
    out, short = RR.add_random_edges_reference(ei, N, 0.5, seed=9, M=M)
    assert not short
    check_properties(out, ei, N, K)
    # and the stream of round 1 does repeat codes of round 0 somewhere in these offsets (the case the skip exists for)
    hits = 0
    for off in range(20):
        c = [np.minimum(*RR.draw(N, M, r, 9, off)) * N + np.maximum(*RR.draw(N, M, r, 9, off)) for r in (0, 1)]
        hits += int(np.isin(c[1], c[0]).sum())
        check_properties(RR.add_random_edges_reference(ei, N, 0.5, seed=9, offset=off, M=M)[0], ei, N, K)
    assert hits > 0


def test_restatement_is_uniform_over_the_free_pairs():
    """symmetric 16-ring, E = 32, p = 0.5 -> K = 8 of F = 104 free pairs; T = 2000 draws.  Every free pair is drawn and every
    count lies within 5 sigma of T K / F, sigma from the binomial.  (The 16-ring is dense by the predicate; the restatement's
    stream does not depend on the regime, which only decides who samples on the device.)"""
    N, T = 16, 2000
    ei = ring(N)
    K, F = 8, 16 * 15 // 2 - 16
    counts = np.zeros((N, N), dtype=np.int64)
    for off in range(T):
        lo, hi = RR.new_pairs(ei, N, K, seed=1234, offset=off)
        assert lo.size == K                                                 # no draw came up short
        counts[lo, hi] += 1
    occ = RR.occupied_codes(ei, N)
    free = np.array([[i, j] for i in range(N) for j in range(i + 1, N) if i * N + j not in set(occ.tolist())])
    assert free.shape[0] == F and counts.sum() == T * K
    c = counts[free[:, 0], free[:, 1]]
    assert counts.sum() == c.sum()                                          # nothing outside the free pairs
    q = K / F
    mean, sigma = T * q, math.sqrt(T * q * (1 - q))
    worst = np.abs(c - mean).max() / sigma
    print(f"uniformity: mean {mean:.1f} sigma {sigma:.2f} min {c.min()} max {c.max()} worst {worst:.2f} sigma")
    assert c.min() > 0 and worst < 5.0


def test_randedge_symbols_declared_exported_and_prototyped():
    from conftest import REPO
    from graph_physics_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mgn_hip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in mgn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.SYMBOLS, f"{name} has no ctypes prototype"
    assert any(s.endswith("mgn_randedge.hip") for s in _capi.SOURCES)
    assert any(s.endswith("mgn_philox.inc") for s in _capi.DEPS)           # the shared generator is part of the source hash
    mk = open(os.path.join(REPO, "graph-physics_amd", "csrc", "Makefile")).read()
    assert "mgn_randedge.hip" in mk and "mgn_philox.inc" in mk
    for inc in ("mgn_host.inc", "mgn_graphprim.inc"):                       # the shared scaffolding and edge primitives too
        assert any(s.endswith(inc) for s in _capi.DEPS) and inc in mk, inc
    assert lib.mgn_version() == _capi.EXPECTED_VERSION == 136              # additive change: the ABI number stays


def test_randedge_host_queries_and_argument_checks_need_no_gpu():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    for N, E, K in ((40, 80, 20), (30160, 180082, 45020), (1000003, 5999924, 299996), (2 ** 20 + 3, 4096, 1024)):
        assert lib.mgn_randedge_default_candidates(N, E, K) == RR.default_candidates(N, E, K)
    small, more_cand, more_edges = (lib.mgn_randedge_workspace_bytes(1000, e, 50, m) for e, m in ((600, 100), (600, 5000), (60000, 100)))
    assert 0 < small < more_cand and small < more_edges
    assert lib.mgn_randedge_workspace_bytes(1000, 600, 50, 0) == lib.mgn_randedge_workspace_bytes(1000, 600, 50, RR.default_candidates(1000, 600, 50))
    assert lib.mgn_randedge_workspace_bytes(1, 600, 50, 0) == 0 and lib.mgn_randedge_workspace_bytes(2 ** 31, 600, 50, 0) == 0
    assert lib.mgn_randedge_workspace_bytes(16, 32, 8, 0) == 0             # the dense regime is not the kernels'
    buf = C.create_string_buffer(4096)
    ws = C.cast(buf, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)                     # never dereferenced: every call below returns before a launch

    def call(E=600, N=1000, K=50, M=0, row=p, out=p, flags=p, ws_=ws, ws_bytes=4096):
        return lib.mgn_randedge(row, row, E, N, K, M, 1, 0, out, out, flags, ws_, ws_bytes, None)

    err = lib.mgn_randedge_last_error
    assert call(N=1) == 1 and b"N must" in err()
    assert call(N=2 ** 31) == 1 and b"N must" in err()
    assert call(E=0) == 1 and b"E must" in err()
    assert call(E=2 ** 31) == 1 and b"E must" in err()
    assert call(K=0) == 1 and b"K must" in err()
    assert call(K=601) == 1 and b"K must" in err()
    assert call(N=16, E=32, K=8) == 1 and b"dense" in err()
    assert call(M=-1) == 1 and b"M must" in err()
    assert call(M=2 ** 30) == 1 and b"M must" in err()
    assert call(row=None) == 1 and b"row0" in err()
    assert call(out=None) == 1 and b"out0" in err()
    assert call(flags=None) == 1 and b"flags" in err()
    assert call(ws_=None) == 1 and b"workspace" in err()
    assert call() == 1 and b"workspace" in err() and b"ws_bytes" in err()   # 4096 bytes are not enough


def test_randedge_python_argument_checks_need_no_gpu():
    from graph_physics_amd import preprocess as P

    ei = torch.zeros(2, 8, dtype=torch.int64)
    for bad in (-0.1, 1.5, "0.5", None, True):
        with pytest.raises(ValueError):
            P.add_random_edges(ei, 9, bad)
        with pytest.raises(ValueError):
            P.build_preprocessing(new_edges_ratio=bad)
    with pytest.raises(ValueError):
        P.add_random_edges(ei, 2 ** 31, 0.5)
    with pytest.raises(ValueError):
        P.add_random_edges(torch.zeros(3, 8, dtype=torch.int64), 9, 0.5)
    with pytest.raises(RuntimeError):                                      # CPU tensors: no CPU path
        P.add_random_edges(ei, 9, 0.5)
    assert callable(P.build_preprocessing(new_edges_ratio=0.25))           # constructing the callable needs no GPU
    P.random_edges_resolve()                                               # nothing queued: nothing to wait for
    P.random_edges_check()


BASE = {"index": {"node_type_index": 2}}


def _captured(monkeypatch, param, device, **kw):
    """the arguments get_preprocessing hands to preprocess.build_preprocessing"""
    from graph_physics_amd import parse_parameters as PP, preprocess as P

    seen = {}
    real = P.build_preprocessing

    def spy(**kwargs):
        seen.update(kwargs)
        return real(**kwargs)

    monkeypatch.setattr(P, "build_preprocessing", spy)
    assert callable(PP.get_preprocessing(param, device, **kw))
    return seen


@pytest.mark.parametrize("bad", [-0.1, 1.5, 2, "0.1", True, [0.1]])
def test_get_preprocessing_refuses_a_bad_ratio(bad):
    from graph_physics_amd import parse_parameters as PP

    for device in (torch.device("cpu"), torch.device("cuda")):
        with pytest.raises(ValueError, match=r"dataset\.new_edges_ratio"):
            PP.get_preprocessing(dict(BASE, dataset={"new_edges_ratio": bad}), device)


def test_get_preprocessing_hands_the_ratio_on(monkeypatch):
    cuda = torch.device("cuda")
    seen = _captured(monkeypatch, dict(BASE, dataset={"new_edges_ratio": 0.1}), cuda)
    assert seen["new_edges_ratio"] == 0.1 and seen["khop"] == 1
    seen = _captured(monkeypatch, dict(BASE, dataset={"new_edges_ratio": 1, "khop": 2}), torch.device("cuda:0"))
    assert seen["new_edges_ratio"] == 1.0 and seen["khop"] == 2 and seen["khop_cache"] == {}
    seen = _captured(monkeypatch, dict(BASE, dataset={"new_edges_ratio": 0.5}), cuda, use_partitioning=True, num_partitions=3)
    assert seen["new_edges_ratio"] == 0.5 and seen["partitioning"]["num_partitions"] == 3
    for off in (0, 0.0, None):                                             # off: the keyword stays at its default
        for device in (cuda, torch.device("cpu")):
            assert "new_edges_ratio" not in _captured(monkeypatch, dict(BASE, dataset={"new_edges_ratio": off}), device)
    assert "new_edges_ratio" not in _captured(monkeypatch, BASE, cuda)


def test_get_preprocessing_has_no_host_path_for_the_ratio():
    from graph_physics_amd import parse_parameters as PP

    with pytest.raises(NotImplementedError, match=r"dataset\.new_edges_ratio"):
        PP.get_preprocessing(dict(BASE, dataset={"new_edges_ratio": 1.0}), torch.device("cpu"))
