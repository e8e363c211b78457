"""CPU: the host side of the sub-mesh (dataset partitioning) feature -- the numpy restatement of PyG's ``subgraph`` against
hand-written answers, the C ABI of csrc/mgn_subgraph.hip (declared, exported, prototyped, the job struct's layout, argument
checks before any launch), the partition arithmetic of ``preprocess`` and the config surface
``parse_parameters.get_preprocessing(use_partitioning=...)``.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import recipe as R
from subgraph_reference import apply_partition_reference, subgraph_reference

SUBGRAPH_SYMBOLS = ("mgn_subgraph_workspace_bytes", "mgn_subgraph_block_edges", "mgn_subgraph_count", "mgn_subgraph_fill",
                    "mgn_gather_rows_batch", "mgn_subgraph_last_error")


def test_reference_formulation_on_hand_written_answers():
    # the path 0-1-2-3-4, both directions, in an order of its own; subset [3, 1, 2] relabels 3 -> 0, 1 -> 1, 2 -> 2
    path = np.array([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
    attr = np.arange(8, dtype=np.float32)[:, None] * np.ones((1, 3), dtype=np.float32)
    ei, ea, mask = subgraph_reference([3, 1, 2], path, attr, num_nodes=5, return_edge_mask=True)
    assert ei.dtype == np.int64
    assert ei.T.tolist() == [[1, 2], [2, 1], [2, 0], [0, 2]]            # edges 1-2, 2-1, 2-3, 3-2 in input order
    assert mask.tolist() == [False, False, True, True, True, True, False, False]
    assert ea[:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]
    # a self loop and a duplicate edge are kept as they are
    messy = np.array([[1, 1, 2, 1, 0], [1, 2, 1, 2, 1]])
    ei, ea = subgraph_reference([1, 2], messy, num_nodes=3)
    assert ea is None and ei.T.tolist() == [[0, 0], [0, 1], [1, 0], [0, 1]]
    # an empty subset keeps nothing
    ei, ea, mask = subgraph_reference([], path, attr, num_nodes=5, return_edge_mask=True)
    assert ei.shape == (2, 0) and ei.dtype == np.int64 and ea.shape == (0, 3) and not mask.any()
    with pytest.raises(IndexError):
        subgraph_reference([5], path, num_nodes=5)
    # _apply_partition sorts the ids first and carries exactly these fields
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    g = apply_partition_reference(x, x + 100, x[:, :1], path, attr, [3, 1, 2], traj_index=7)
    assert sorted(g) == ["edge_attr", "edge_index", "num_nodes", "pos", "traj_index", "x", "y"]
    assert g["x"].tolist() == x[[1, 2, 3]].tolist() and g["y"].tolist() == (x + 100)[[1, 2, 3]].tolist()
    assert g["edge_index"].T.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1]] and g["num_nodes"] == 3 and g["traj_index"] == 7


def test_subgraph_symbols_declared_exported_and_prototyped():
    from conftest import REPO
    from graph_physics_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mgn_hip.h")).read(), flags=re.S)
    lib = _capi.lib()
    for name in SUBGRAPH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in mgn_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.SYMBOLS, f"{name} has no ctypes prototype"
    assert any(s.endswith("mgn_subgraph.hip") for s in _capi.SOURCES)
    assert "mgn_subgraph.hip" in open(os.path.join(REPO, "graph-physics_amd", "csrc", "Makefile")).read()
    assert lib.mgn_version() == _capi.EXPECTED_VERSION


def test_gather_job_layout_matches_header(tmp_path):
    import capi_layout
    from graph_physics_amd import _capi

    st = _capi.GatherJob
    got = capi_layout.gcc_layout(tmp_path, {"mgn_gather_job": st}, macros=["MGN_MAX_GATHER_JOBS"])
    capi_layout.assert_layout(got, "mgn_gather_job", st)
    assert got["MGN_MAX_GATHER_JOBS"] == _capi.MAX_GATHER_JOBS == 8
    assert [f for f, _ in st._fields_] == ["src", "ld_src", "width", "idx", "rows", "dst", "ld_dst", "src_rows"]


def test_subgraph_host_queries_need_no_gpu():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    assert lib.mgn_subgraph_block_edges() >= 64
    small, more_edges, more_nodes = (lib.mgn_subgraph_workspace_bytes(n, e) for n, e in ((1000, 6000), (1000, 60000), (100000, 6000)))
    assert 0 < small < more_edges and small < more_nodes
    assert lib.mgn_subgraph_workspace_bytes(0, 0) > 0                       # an empty graph is a valid input
    assert lib.mgn_subgraph_workspace_bytes(-1, 10) == 0 and lib.mgn_subgraph_workspace_bytes(10, -1) == 0
    assert lib.mgn_subgraph_workspace_bytes(2 ** 31 - 1, 10) == 0 and lib.mgn_subgraph_workspace_bytes(10, 2 ** 40 + 1) == 0


def test_subgraph_argument_checks_return_before_any_launch():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    err = lib.mgn_subgraph_last_error
    n_edges = C.c_int64(-1)
    buf = C.create_string_buffer(4096)
    ws = C.cast(buf, C.c_void_p)
    ids = C.cast(C.create_string_buffer(64), C.c_void_p)       # never read: every call below returns before a launch

    def count(node_ids, S, N, src, dst, E, out=C.byref(n_edges), w=ws, ws_bytes=4096):
        return lib.mgn_subgraph_count(node_ids, S, N, src, dst, E, out, w, ws_bytes, None)

    assert count(ids, 4, -1, ids, ids, 4) == 1 and b"N must" in err()
    assert count(ids, 4, 2 ** 31 - 1, ids, ids, 4) == 1 and b"N must" in err()          # beyond the 32-bit table
    assert count(ids, -1, 10, ids, ids, 4) == 1 and b"S must" in err()
    assert count(ids, 4, 10, ids, ids, -1) == 1 and b"E must" in err()
    assert count(ids, 4, 10, ids, ids, 2 ** 40 + 1) == 1 and b"E must" in err()
    assert count(None, 4, 10, ids, ids, 4) == 1 and b"node_ids" in err()
    assert count(ids, 4, 10, None, ids, 4) == 1 and b"src / dst" in err()
    assert count(ids, 4, 10, ids, None, 4) == 1 and b"src / dst" in err()
    assert count(ids, 4, 10, ids, ids, 4, out=None) == 1 and b"n_edges_host" in err()
    assert count(ids, 4, 10, ids, ids, 4, w=None) == 1 and b"workspace" in err()
    assert count(ids, 4, 100000, ids, ids, 4) == 1 and b"workspace" in err() and b"ws_bytes" in err()
    assert n_edges.value == -1                                                         # nothing was touched

    def fill(w, ws_bytes, E, cap):
        return lib.mgn_subgraph_fill(w, ws_bytes, E, None, None, None, None, cap, None)

    assert fill(ws, 4096, -1, 0) == 1 and b"E must" in err()
    assert fill(ws, 4096, 2 ** 40 + 1, 0) == 1 and b"E must" in err()
    assert fill(ws, 4096, 4, -1) == 1 and b"cap" in err()
    assert fill(None, 4096, 4, 0) == 1 and b"workspace" in err()
    assert fill(ws, 16, 4, 0) == 1 and b"workspace" in err()

    jobs = (_capi.GatherJob * 9)()

    def job(**kw):
        j = jobs[0]
        j.src = j.idx = j.dst = ids.value
        j.ld_src, j.width, j.rows, j.ld_dst, j.src_rows = 4, 4, 2, 4, 2
        for k, v in kw.items():
            setattr(j, k, v)
        return lib.mgn_gather_rows_batch(1, jobs, None)

    assert lib.mgn_gather_rows_batch(-1, jobs, None) == 1 and b"n_jobs" in err()
    assert lib.mgn_gather_rows_batch(9, jobs, None) == 1 and b"n_jobs" in err()
    assert lib.mgn_gather_rows_batch(1, None, None) == 1 and b"jobs" in err()
    assert job(width=0) == 1 and b"width" in err()
    assert job(width=2 ** 31) == 1 and b"width" in err()
    assert job(rows=-1) == 1 and b"rows" in err()
    assert job(src_rows=-1) == 1 and b"rows" in err()
    assert job(ld_src=3) == 1 and b"ld_src" in err()
    assert job(ld_dst=3) == 1 and b"ld_src / ld_dst" in err()
    assert job(src=None) == 1 and b"null" in err()
    assert job(idx=None) == 1 and b"null" in err()
    assert job(dst=None) == 1 and b"null" in err()
    assert lib.mgn_gather_rows_batch(0, None, None) == 0                                # nothing to do is not an error
    assert job(rows=0, src=None, idx=None, dst=None) == 0                              # nor is a job without rows


def test_num_partitions_for_and_partition_sample():
    from graph_physics_amd import preprocess as P

    assert P.num_partitions_for(1001, max_nodes_per_partition=250) == 5                # ceil(1001 / 250)
    assert P.num_partitions_for(1000, max_nodes_per_partition=250) == 4
    assert P.num_partitions_for(10, max_nodes_per_partition=250) == 1
    assert P.num_partitions_for(1001, num_partitions=8) == 8                           # a fixed count, whatever the mesh
    with pytest.raises(ValueError, match="not both"):
        P.num_partitions_for(1001, 4, 250)
    with pytest.raises(ValueError, match="specify either"):
        P.num_partitions_for(1001)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            P.num_partitions_for(1001, num_partitions=bad)
        with pytest.raises(ValueError):
            P.num_partitions_for(1001, max_nodes_per_partition=bad)
    # _get_indices: the parts of one frame are consecutive samples
    assert [P.partition_sample(i, 3) for i in range(7)] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)]
    assert P.partition_sample(5, 1) == (5, 0)


def test_python_argument_checks_need_no_gpu():
    import graph_physics_amd as gp
    from graph_physics_amd import preprocess as P

    ei = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError):       # CPU tensors: no CPU path
        P.subgraph(torch.arange(2), ei, num_nodes=4)
    with pytest.raises(RuntimeError):
        P.apply_partition(gp.Graph(x=torch.zeros(4, 3), edge_index=ei), torch.arange(2))
    with pytest.raises(RuntimeError):
        P.gather_rows_batch([torch.zeros(4, 3)], [torch.arange(2)])
    with pytest.raises(ValueError, match="not both"):
        P.build_preprocessing(partitioning={"num_partitions": 2, "max_nodes_per_partition": 100})
    with pytest.raises(ValueError, match="specify either"):
        P.build_preprocessing(partitioning={})
    with pytest.raises(ValueError, match="unknown keys"):
        P.build_preprocessing(partitioning={"num_partitions": 2, "parts": 3})
    with pytest.raises(ValueError):
        P.partition_node_ids(gp.Graph(x=torch.zeros(4, 3), edge_index=ei), 0)
    # the host half of the pipeline runs where the graph lives: one part is every node, k parts are disjoint and covering
    _, mesh_ei, _ = R.delaunay_graph(200, 3)
    g = gp.Graph(x=torch.zeros(200, 3), pos=torch.rand(200, 2, generator=torch.Generator().manual_seed(0)), edge_index=mesh_ei)
    one = P.partition_node_ids(g, 1)
    assert len(one) == 1 and one[0].dtype == torch.int64 and torch.equal(one[0], torch.arange(200))
    parts = P.partition_node_ids(g, 3)
    assert len(parts) == 3 and all(p.dtype == torch.int64 and torch.equal(p, p.sort()[0]) for p in parts)
    assert torch.equal(torch.cat(parts).sort()[0], torch.arange(200))
    # without the argument the callable of today: no ``part`` keyword, no cache
    import inspect
    assert list(inspect.signature(P.build_preprocessing()).parameters) == ["graph", "step"]
    f = P.build_preprocessing(partitioning={"num_partitions": 3})
    assert list(inspect.signature(f).parameters) == ["graph", "step", "part"] and f.partition_cache == {}


BASE = {"index": {"node_type_index": 2}}


def _captured(monkeypatch, param, **kw):
    """the arguments get_preprocessing hands to preprocess.build_preprocessing"""
    from graph_physics_amd import parse_parameters as PP, preprocess as P

    seen = {}
    real = P.build_preprocessing

    def spy(**kwargs):
        seen.clear()
        seen.update(kwargs)
        return real(**kwargs)

    monkeypatch.setattr(P, "build_preprocessing", spy)
    fn = PP.get_preprocessing(param, torch.device("cpu"), **kw)
    assert callable(fn)                       # constructing the callable needs no GPU
    return dict(seen)


def test_get_preprocessing_passes_the_partitioning_arguments(monkeypatch):
    today = {"noise_parameters", "world_pos_parameters", "add_edges_features", "extra_node_features", "extra_edge_features", "khop",
             "khop_cache"}
    assert set(_captured(monkeypatch, BASE)) == today                                  # what it builds today, argument for argument
    assert set(_captured(monkeypatch, BASE, num_partitions=4)) == today                # the counts alone switch nothing on (upstream too)
    seen = _captured(monkeypatch, BASE, use_partitioning=True, num_partitions=4)
    assert set(seen) == today | {"partitioning"}
    assert seen["partitioning"] == {"num_partitions": 4, "max_nodes_per_partition": None}
    seen = _captured(monkeypatch, dict(BASE, dataset={"khop": 2}), use_partitioning=True, max_nodes_per_partition=250)
    assert seen["partitioning"] == {"num_partitions": None, "max_nodes_per_partition": 250} and seen["khop"] == 2
    from graph_physics_amd import parse_parameters as PP
    with pytest.raises(ValueError, match="not both"):
        PP.get_preprocessing(BASE, torch.device("cpu"), use_partitioning=True, num_partitions=4, max_nodes_per_partition=250)
    with pytest.raises(ValueError, match="specify either"):
        PP.get_preprocessing(BASE, torch.device("cpu"), use_partitioning=True)


def test_a_loss_that_reads_faces_is_refused_with_partitioning():
    from graph_physics_amd import parse_parameters as PP

    cpu = torch.device("cpu")
    physics = dict(BASE, loss={"type": ["l2loss", "divergencel2loss"], "weights": [1.0, 0.1], "gradient_method": "least_squares"})
    with pytest.raises(ValueError, match=r"use_partitioning.*graph\.face"):
        PP.get_preprocessing(physics, cpu, use_partitioning=True, num_partitions=3)
    assert callable(PP.get_preprocessing(physics, cpu))                                 # unpartitioned: trains as before
    # finite differences read edge_index only, and a plain loss nothing of the mesh: both train on parts
    fd = dict(physics, loss=dict(physics["loss"], gradient_method="finite_diff"))
    assert callable(PP.get_preprocessing(fd, cpu, use_partitioning=True, num_partitions=3))
    plain = dict(BASE, loss={"type": ["l2loss"]})
    assert callable(PP.get_preprocessing(plain, cpu, use_partitioning=True, num_partitions=3))
    assert callable(PP.get_preprocessing(BASE, cpu, use_partitioning=True, num_partitions=3))
    with pytest.raises(ValueError, match=r"graph\.face"):
        PP.check_partitioned_loss(physics)
    PP.check_partitioned_loss(fd)
