"""CPU: the host side of the k-hop feature -- the scipy reference formulation against hand-written answers, the C ABI of
csrc/mgn_khop.hip (declared, exported, prototyped; argument checks before any launch) and the config surface
``parse_parameters.get_preprocessing`` (``dataset.khop``).  Nothing here needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from khop_reference import khop_reference

KHOP_SYMBOLS = ("mgn_khop_workspace_bytes", "mgn_khop_row_capacity", "mgn_khop_count", "mgn_khop_fill", "mgn_khop_last_error")


def test_reference_formulation_on_hand_written_answers():
    path = np.array([[0, 1, 2], [1, 2, 3]])
    got = khop_reference(path, 4, 2)
    assert got.dtype == np.int64
    assert got.T.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    ring = np.stack([np.arange(64), (np.arange(64) + 1) % 64])
    got = khop_reference(ring, 64, 5)
    assert got.shape == (2, 64 * 5)
    for i in range(64):
        assert got[1, got[0] == i].tolist() == sorted((i + d) % 64 for d in range(1, 6))
    empty = khop_reference(np.zeros((2, 0), dtype=np.int64), 7, 2)
    assert empty.shape == (2, 0) and empty.dtype == np.int64
    # unsorted input with a duplicate and a self loop gives the same set
    messy = np.array([[2, 0, 1, 1, 0], [3, 1, 2, 1, 1]])
    assert np.array_equal(khop_reference(messy, 4, 2), khop_reference(path, 4, 2))


def test_khop_symbols_declared_exported_and_prototyped():
    import os

    from conftest import REPO
    from graph_physics_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mgn_hip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in KHOP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in mgn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.SYMBOLS, f"{name} has no ctypes prototype"
    assert any(s.endswith("mgn_khop.hip") for s in _capi.SOURCES)
    assert "mgn_khop.hip" in open(os.path.join(REPO, "graph-physics_amd", "csrc", "Makefile")).read()
    assert lib.mgn_version() == _capi.EXPECTED_VERSION == 136   # additive change: the ABI number stays


def test_khop_host_queries_and_argument_checks_need_no_gpu():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    assert lib.mgn_khop_row_capacity() >= 256
    small, more_edges, more_nodes = (lib.mgn_khop_workspace_bytes(n, e) for n, e in ((1000, 6000), (1000, 60000), (100000, 6000)))
    assert 0 < small < more_edges and small < more_nodes
    assert lib.mgn_khop_workspace_bytes(0, 10) == 0 and lib.mgn_khop_workspace_bytes(10, -1) == 0
    assert lib.mgn_khop_workspace_bytes(2 ** 31 - 1, 10) == 0
    n_out, n_ovf = C.c_int64(-1), C.c_int64(-1)
    buf = C.create_string_buffer(1024)
    ws = C.cast(buf, C.c_void_p)

    def count(E, N, hops, ws_bytes):
        return lib.mgn_khop_count(None, None, E, N, hops, C.byref(n_out), C.byref(n_ovf), ws, ws_bytes, None)

    assert count(10, 100, 1, 1024) == 1 and b"hops" in lib.mgn_khop_last_error()
    assert count(10, 100, 0, 1024) == 1 and b"hops" in lib.mgn_khop_last_error()
    assert count(10, 0, 2, 1024) == 1 and b"N" in lib.mgn_khop_last_error().split(b":")[1]
    assert count(10, 2 ** 31 - 1, 2, 1024) == 1 and b"N" in lib.mgn_khop_last_error().split(b":")[1]
    assert count(-1, 100, 2, 1024) == 1 and b"E" in lib.mgn_khop_last_error().split(b":")[1]
    assert count(10, 100, 2, 1024) == 1 and b"workspace" in lib.mgn_khop_last_error() and b"ws_bytes" in lib.mgn_khop_last_error()
    # the fill half: the same checks, before it looks at the workspace
    assert lib.mgn_khop_fill(ws, 1024, 100, 1, None, None, 0, None) == 1 and b"hops" in lib.mgn_khop_last_error()
    assert lib.mgn_khop_fill(ws, 1024, 0, 2, None, None, 0, None) == 1 and b"N" in lib.mgn_khop_last_error().split(b":")[1]
    assert lib.mgn_khop_fill(ws, 16, 100, 2, None, None, 0, None) == 1 and b"workspace" in lib.mgn_khop_last_error()


def test_khop_python_argument_checks_need_no_gpu():
    from graph_physics_amd import preprocess as P

    ei = torch.zeros(2, 3, dtype=torch.int64)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            P.khop_edges(ei, 4, bad)
    with pytest.raises(RuntimeError):       # CPU tensors: no CPU path
        P.khop_edges(ei, 4, 2)
    for bad in (0, 2.0, "2"):
        with pytest.raises(ValueError):
            P.build_preprocessing(khop=bad)


BASE = {"index": {"node_type_index": 2}}


def _captured(monkeypatch, param, **kw):
    """the arguments get_preprocessing hands to preprocess.build_preprocessing"""
    from graph_physics_amd import parse_parameters as PP, preprocess as P

    seen = {}
    real = P.build_preprocessing

    def spy(**kwargs):
        seen.update(kwargs)
        return real(**kwargs)

    monkeypatch.setattr(P, "build_preprocessing", spy)
    fn = PP.get_preprocessing(param, torch.device("cpu"), **kw)
    assert callable(fn)                       # constructing the callable needs no GPU
    return seen


def test_get_preprocessing_reads_the_reference_keys(monkeypatch):
    prep = {"noise": 0.02, "noise_index_start": [0], "noise_index_end": [2]}
    param = dict(BASE, transformations={"preprocessing": prep})
    seen = _captured(monkeypatch, param)
    assert seen["noise_parameters"] == {"noise_index_start": [0], "noise_index_end": [2], "noise_scale": 0.02, "node_type_index": 2}
    assert seen["world_pos_parameters"] is None and seen["add_edges_features"] is True
    assert seen["khop"] == 1 and seen["khop_cache"] is None
    assert seen["extra_node_features"] is None and seen["extra_edge_features"] is None
    # remove_noise drops the noise step; noise 0 (the default) never adds it
    assert _captured(monkeypatch, param, remove_noise=True)["noise_parameters"] is None
    assert _captured(monkeypatch, BASE)["noise_parameters"] is None
    assert _captured(monkeypatch, BASE, use_edge_feature=False)["add_edges_features"] is False
    f, g = (lambda graph: graph), (lambda graph: graph)
    seen = _captured(monkeypatch, BASE, extra_node_features=f, extra_edge_features=[g])
    assert seen["extra_node_features"] is f and seen["extra_edge_features"] == [g]


def test_get_preprocessing_world_position_block(monkeypatch):
    world = {"use": True, "world_pos_index_start": 0, "world_pos_index_end": 3}
    seen = _captured(monkeypatch, {"index": {"node_type_index": 6}, "transformations": {"world_pos_parameters": world}})
    assert seen["world_pos_parameters"] == {"world_pos_index_start": 0, "world_pos_index_end": 3, "node_type_index": 6}
    world = dict(world, use=False)
    assert _captured(monkeypatch, {"index": {"node_type_index": 6}, "transformations": {"world_pos_parameters": world}})["world_pos_parameters"] is None


def test_get_preprocessing_honours_dataset_khop(monkeypatch):
    assert _captured(monkeypatch, dict(BASE, dataset={}))["khop"] == 1
    seen = _captured(monkeypatch, dict(BASE, dataset={"khop": 1}))
    assert seen["khop"] == 1 and seen["khop_cache"] is None
    seen = _captured(monkeypatch, dict(BASE, dataset={"khop": 3}))
    assert seen["khop"] == 3 and seen["khop_cache"] == {}
    assert _captured(monkeypatch, dict(BASE, dataset={"khop": 2, "new_edges_ratio": 0}))["khop"] == 2


@pytest.mark.parametrize("bad", [0, -2, 2.5, "2", None, True])
def test_get_preprocessing_refuses_a_bad_khop(bad):
    from graph_physics_amd import parse_parameters as PP

    with pytest.raises(ValueError, match=r"dataset\.khop"):
        PP.get_preprocessing(dict(BASE, dataset={"khop": bad}), torch.device("cpu"))


def test_get_preprocessing_refuses_new_edges_ratio():
    from graph_physics_amd import parse_parameters as PP

    with pytest.raises(NotImplementedError, match=r"dataset\.new_edges_ratio"):
        PP.get_preprocessing(dict(BASE, dataset={"new_edges_ratio": 0.1}), torch.device("cpu"))
