"""include/mgn_hip.h as a C compiler and a text search see it, for the tests that hold the ctypes binding (_capi.py) to it:
struct layouts by gcc, prototypes and struct fields by regular expressions over the header, and the translation unit that
defines a symbol by a search of csrc/."""
import ctypes as C
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "graph-physics_amd", "csrc")

#: ctypes mirror in _capi.py -> the header's struct
C_NAMES = {"MlpFwdArgs": "mgn_mlp_fwd_args", "MlpBwdArgs": "mgn_mlp_bwd_args", "ColredJob": "mgn_colred_job", "WgradJob": "mgn_wgrad_job",
           "WpackBlock": "mgn_wpack_block", "SimDesc": "mgn_sim_desc", "EdgeBwdFusedArgs": "mgn_edge_bwd_fused_args",
           "LinearArgs": "mgn_linear_args", "RownormPhase": "mgn_rownorm_phase", "OptTensor": "mgn_opt_tensor", "TBlock": "mgn_tblock",
           "LossArgs": "mgn_loss_args", "GatherJob": "mgn_gather_job"}


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_text():
    """the header without comments"""
    with open(os.path.join(REPO, "include", "mgn_hip.h")) as fh:
        return _strip_comments(fh.read())


def header_structs():
    """C name -> field names in declaration order, of every ``typedef struct { ... } name;`` of the header"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", header_text(), flags=re.S):
        decls = [d for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", d.strip()).group(1) for d in decls]
    return out


def mirrors(capi):
    """C name -> class, of every ``ctypes.Structure`` subclass that ``capi`` defines"""
    found = [v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == capi.__name__]
    missing = [v.__name__ for v in found if v.__name__ not in C_NAMES]
    assert not missing, f"no C name listed for {missing}"
    return {C_NAMES[v.__name__]: v for v in found}


def gcc_layout(tmp_path, structs, macros=()):
    """``{"<struct>": sizeof, "<struct>.<field>": offsetof, "<MACRO>": value}`` as gcc lays out the header (LP64), for the fields
    of the ctypes mirrors ``structs`` (C name -> class) and the integer macros named"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the toolchain contract"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mgn_hip.h"', "int main(void) {"]
    for name, st in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{fld} %zu\\n", offsetof({name}, {fld}));' for fld, _ in st._fields_]
    lines += [f'printf("{m} %d\\n", {m});' for m in macros] + ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (l.split() for l in out.splitlines())}


def assert_layout(got, name, st):
    assert got[name] == C.sizeof(st), name
    for fld, _ in st._fields_:
        assert got[f"{name}.{fld}"] == getattr(st, fld).offset, f"{name}.{fld}"


# ------------------------------------------------------------------------------- prototypes
_C_CLASS = {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "unsigned": "i32", "int64_t": "i64", "uint64_t": "i64", "size_t": "i64",
            "float": "float", "double": "double", "void": "void"}


def _c_class(decl, named):
    """class of one C declaration: a parameter (``named``: with its name) or a return type"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]
    assert len(words) == 1 and words[0] in _C_CLASS, f"unclassified C type: {decl!r}"
    return _C_CLASS[words[0]]


def header_prototypes():
    """name -> (return class, [argument classes]) of every function the header declares; the classes are ptr, i32, i64, float,
    double and void (size_t and the 64-bit integers are one class: LP64)"""
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", header_text(), flags=re.S)
    text = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\s*\b(mgn_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        args = [] if params == ["void"] or params == [""] else [_c_class(p, True) for p in params]
        assert name not in out, f"{name} is declared twice"
        out[name] = (_c_class(ret.strip(), False), args)
    return out


def ctypes_class(t):
    if t is None:
        return "void"
    if issubclass(t, (C._Pointer, C.Array)) or t in (C.c_void_p, C.c_char_p):
        return "ptr"
    code = t._type_
    if code in "fd":
        return {"f": "float", "d": "double"}[code]
    assert code in "iIlLqQ", f"unclassified ctypes type: {t}"
    return f"i{8 * C.sizeof(t)}"


# ------------------------------------------------------------------------------- which unit defines a symbol
def unit_source(unit):
    """csrc/mgn_<unit>.hip with the ``.inc`` files it includes (transitively), without comments"""
    seen, todo, text = set(), [f"mgn_{unit}.hip"], ""
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(os.path.join(CSRC, f)):
            continue
        seen.add(f)
        with open(os.path.join(CSRC, f)) as fh:
            src = _strip_comments(fh.read())
        text += src
        todo += re.findall(r'#include\s+"(\w+\.inc)"', src)
    return text


def defines(source, name):
    """a function body of ``name`` at the start of a declaration (not a call inside an expression)"""
    return re.search(r"^[^\n(=;]*\b%s\s*\([^;{}]*\)\s*\{" % name, source, flags=re.M) is not None
