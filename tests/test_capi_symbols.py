"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/mgn_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

from conftest import REPO

import capi_layout as CL


def _declared():
    src = open(os.path.join(REPO, "include", "mgn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mgn_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mgn_hip.h but not exported"
        assert n in _capi.SYMBOLS, f"{n} has no ctypes prototype"
    assert lib.mgn_version() >= 100
    assert lib.mgn_last_error() == b""


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of every argument struct as gcc lays out include/mgn_hip.h (LP64) against the ctypes mirrors in
    _capi.py: every ``ctypes.Structure`` the binding defines, every struct the header declares, field for field."""
    from graph_physics_amd import _capi as c

    structs, fields = CL.mirrors(c), CL.header_structs()
    assert len(structs) == 13 and set(structs) == set(fields), set(structs) ^ set(fields)
    got = CL.gcc_layout(tmp_path, structs)
    for name, st in structs.items():
        assert [f for f, _ in st._fields_] == fields[name], name
        CL.assert_layout(got, name, st)
    assert c.MAX_LAYERS == 8 and c.MAX_PHASES == 3 and c.MAX_WGRAD_JOBS == 48
    assert c.WPACK_BYTES == 98304


def test_prototypes_match_header():
    """every prototype of the header against ``_capi.SYMBOLS``: the argument count, the class of each argument (pointer, 32-bit
    integer, 64-bit integer, float, double) and of the return value"""
    from graph_physics_amd import _capi

    protos = CL.header_prototypes()
    assert sorted(protos) == _declared() == sorted(_capi.SYMBOLS) and len(protos) == 93
    for name, (ret, args) in protos.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args), f"{name}: {len(argtypes)} argtypes, {len(args)} parameters"
        got = [CL.ctypes_class(t) for t in argtypes]
        assert got == args, f"{name}: argument {[i for i, (g, a) in enumerate(zip(got, args)) if g != a]}: {got} vs {args}"
        assert CL.ctypes_class(res) == ret, f"{name}: returns {ret}"


def test_symbol_groups_name_the_defining_unit():
    """``_capi.UNITS`` files each symbol under the translation unit whose error text ``check`` reports: the name must be defined in
    that csrc/mgn_<unit>.hip (or an .inc it includes), and SYMBOLS is the flat union of the groups"""
    from graph_physics_amd import _capi

    assert [os.path.basename(s) for s in _capi.SOURCES] == [f"mgn_{u}.hip" for u in _capi.UNITS]
    assert sum(len(g) for g in _capi.UNITS.values()) == len(_capi.SYMBOLS)
    for unit, group in _capi.UNITS.items():
        src = CL.unit_source(unit)
        assert ("mgn_last_error" if unit == "kernels" else f"mgn_{unit}_last_error") in group
        for name in group:
            assert _capi.SYMBOLS[name] is group[name]
            assert CL.defines(src, name), f"{name} is not defined in mgn_{unit}.hip"


def _refused_calls(_capi):
    """per translation unit one call with invalid arguments that returns before any HIP call: (symbol, call)"""
    lib = _capi.lib()
    n64 = ctypes.c_int64(0)
    ws = ctypes.cast(ctypes.create_string_buffer(1024), ctypes.c_void_p)
    fwd = _capi.MlpFwdArgs()
    fwd.M, fwd.H, fwd.NL, fwd.nphase, fwd.out_w = 0, 100, 4, 1, 100
    return {
        "kernels": ("mgn_mlp_fwd", lambda: lib.mgn_mlp_fwd(ctypes.byref(fwd), None)),
        "prep": ("mgn_edge_features", lambda: lib.mgn_edge_features(None, 5, None, None, 0, None, None)),
        "attn": ("mgn_head_axis_attn_fwd", lambda: lib.mgn_head_axis_attn_fwd(None, None, None, 4, 128, 3, None, None, None)),
        "dense": ("mgn_rownorm_fwd", lambda: lib.mgn_rownorm_fwd(None, 0, 0, None, 0.0, 0, None, None, None)),
        "loss": ("mgn_loss_fwd", lambda: lib.mgn_loss_fwd(ctypes.byref(_capi.LossArgs()), None)),
        "khop": ("mgn_khop_count", lambda: lib.mgn_khop_count(None, None, 10, 100, 1, ctypes.byref(n64), ctypes.byref(n64), ws, 1024, None)),
        "subgraph": ("mgn_subgraph_count", lambda: lib.mgn_subgraph_count(ws, 4, -1, ws, ws, 4, ctypes.byref(n64), ws, 1024, None)),
        "randedge": ("mgn_randedge", lambda: lib.mgn_randedge(ws, ws, 600, 1, 50, 0, 1, 0, ws, ws, ws, ws, 1024, None)),
        "knn": ("mgn_knn_search", lambda: lib.mgn_knn_search(ws, 10, ws, 10, 1, 3, ws, ws, 1, 0, ws, ws, None)),
    }


def test_check_finds_the_error_channel_from_the_symbol():
    """for each of the nine units: a refused call, then ``check(rc, name)`` WITHOUT a unit keyword raises with that unit's text
    (the other units hold the text of their own last refusal by then); the keywords still serve a ``what`` that is no symbol"""
    import pytest

    from graph_physics_amd import _capi

    lib = _capi.lib()
    calls = _refused_calls(_capi)
    assert list(calls) == list(_capi.UNITS)
    for name, call in calls.values():    # every channel holds a text of its own
        assert call() == 1
    for unit, (name, call) in calls.items():
        assert call() == 1
        text = getattr(lib, "mgn_last_error" if unit == "kernels" else f"mgn_{unit}_last_error")().decode()
        assert ("H must be" if unit == "kernels" else name) in text, (unit, text)   # (mgn_kernels.hip does not prefix the symbol)
        with pytest.raises(RuntimeError) as e:
            _capi.check(1, name)
        assert str(e.value) == f"{name} failed (code 1): {text}"
        if unit != "kernels":
            with pytest.raises(RuntimeError) as e:
                _capi.check(1, "a launch", **{unit: True})
            assert str(e.value) == f"a launch failed (code 1): {text}"
            with pytest.raises(RuntimeError) as e:   # a symbol name outranks a keyword of another unit
                _capi.check(1, "mgn_mlp_fwd", **{unit: True})
            assert str(e.value) == f"mgn_mlp_fwd failed (code 1): {lib.mgn_last_error().decode()}"
    _capi.check(0, "mgn_mlp_fwd")


def test_host_side_queries_need_no_gpu():
    from graph_physics_amd import _capi

    lib = _capi.lib()
    assert lib.mgn_csr_workspace_bytes(100, 10) >= 10 * 4
    assert lib.mgn_mlp_bwd_workspace_bytes(1000, 128, 4) > 0
    # argument validation happens before any launch
    a = _capi.MlpFwdArgs()
    a.M, a.H, a.NL, a.nphase, a.out_w = 0, 100, 4, 1, 100
    assert lib.mgn_mlp_fwd(ctypes.byref(a), None) == 1
    assert b"H must be" in lib.mgn_last_error()


def test_two_byte_operands_are_refused_outside_the_bf16_packed_path():
    """[r4] negative leading dimensions of mgn_wgrad_job (two-byte rows) and precision 2 of mgn_mlp_fwd are taken only where a kernel
    reads / writes that form: validated before any launch, so this runs without a GPU."""
    from graph_physics_amd import _capi

    lib = _capi.lib()
    job = (_capi.WgradJob * 1)()
    job[0].M, job[0].lda, job[0].ldb, job[0].ldw, job[0].nja, job[0].nkb, job[0].kw = 1000, -128, 128, 128, 8, 8, 128
    assert lib.mgn_wgrad_p(1, job, None, 0, 0, None) == 1           # fp32-grade precision: no two-byte operand
    assert b"negative leading dimension" in lib.mgn_last_error()
    job[0].lda, job[0].nja = -64, 4                                   # not a full 128 x 128 job
    assert lib.mgn_wgrad_p(1, job, None, 0, 1, None) == 1
    a = _capi.MlpFwdArgs()
    a.M, a.H, a.NL, a.nphase, a.out_w, a.precision = 100, 128, 4, 1, 128, 2   # no packed weights: not the split-bf16 path
    a.kw[0] = 128
    assert lib.mgn_mlp_fwd(ctypes.byref(a), None) == 1
    assert b"precision 2" in lib.mgn_last_error()
    a.precision = 3
    assert lib.mgn_mlp_fwd(ctypes.byref(a), None) == 1
