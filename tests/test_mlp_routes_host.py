"""Which kernel takes a launch, pinned on the CPU.  tests/route_driver.cpp includes csrc/mgn_kernels.hip (host side only), stands in
for the HIP runtime and calls mgn_mlp_fwd, mgn_mlp_bwd, mgn_colred_batch and mgn_wgrad_p over shapes and MGN_* switches on both
sides of every threshold of the routing; its output -- return code, error text and every launch as `name grid block lds`, for a
weight-gradient launch also its width, interleave and first workgroup per job -- must
equal tests/mlp_routes_expected.txt line by line.  That file records what the code computed before the routes moved into
route_fwd / route_bwd / route_wgrad: a line that differs is a behaviour change.  Whoever adds a kernel adds its cases to the
driver and its lines to the file.  The driver also exits non-zero if a launch with dynamic LDS was not preceded by a reservation
of at least that many bytes for that kernel.

How the recorded file was made (from the commit before the routes moved, which had no kernel table to name a launch through): a
copy of the driver whose stand-ins for hipLaunchKernel / hipFuncSetAttribute / the call configuration do nothing, and which
records at the launch statement instead, by these lines in front of `#include "mgn_kernels.hip"`:

    struct WgradLaunch;
    static int g_H = 0;  // H of the running case (set by begin_case): spells the HB of the generic instantiations as a number
    template <class T> static std::string rd_extra(const T&) { return ""; }
    static std::string wgrad_handout(const WgradLaunch& L);  // as in the driver
    template <class... A>
    static void rd_launch(const char* k, dim3 g, dim3 b, size_t lds, const A&... args) {
      std::string extra = (rd_extra(args) + ... + std::string());
      std::string n;
      for (const char* p = k; *p; ++p)
        if (*p != ' ') n += *p;
      if (n.size() >= 2 && n[0] == '(' && n[n.size() - 1] == ')') n = n.substr(1, n.size() - 2);
      const size_t at = n.find("<HB,");
      if (at != std::string::npos) n.replace(at, 4, "<" + std::to_string(g_H / 16) + ",");
      if (g.y == 1) printf("  %s grid=%u block=%u lds=%zu%s\\n", n.c_str(), g.x, b.x, lds, extra.c_str());
      else printf("  %s grid=%ux%u block=%u lds=%zu%s\\n", n.c_str(), g.x, g.y, b.x, lds, extra.c_str());
    }
    #undef hipLaunchKernelGGL
    #define hipLaunchKernelGGL(k, g, b, lds, s, ...) rd_launch(#k, g, b, lds, __VA_ARGS__)

and behind the include `template <> std::string rd_extra<WgradLaunch>(const WgradLaunch& L) { return wgrad_handout(L); }`.

    hipcc --offload-arch=gfx950 --cuda-host-only -x hip -std=c++17 -O1 -I graph-physics_amd/csrc -I include -c mint.cpp -o mint.o
    clang++ mint.o -o mint -Wl,--unresolved-symbols=ignore-all && ./mint > tests/mlp_routes_expected.txt

The cases are the driver's, unchanged: 349 of them, in which all 85 kernel instantiations that the four entry points can launch
appear, every `fail(1, ...)` of theirs is raised, and each of the fifteen MGN_* switches changes at least one launch."""
import os, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _host_linker():
    """a C++ driver that links a plain host program: the clang++ next to hipcc, else the system's"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"),
              shutil.which("clang++"), shutil.which("c++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no C++ compiler driver to link the route driver with")


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_every_route_and_refusal_equals_the_recorded_one(tmp_path):
    obj, exe = str(tmp_path / "route_driver.o"), str(tmp_path / "route_driver")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1",
                        "-I", os.path.join(ROOT, "graph-physics_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        "-c", os.path.join(ROOT, "tests", "route_driver.cpp"), "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # no HIP runtime: the driver defines what the object calls; the device image's symbol stays unresolved and unused
    r = subprocess.run([_host_linker(), obj, "-o", exe, "-Wl,--unresolved-symbols=ignore-all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    got = r.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "mlp_routes_expected.txt")).read().splitlines()
    case = ""
    for i, (g, w) in enumerate(zip(got, want)):
        if w.startswith("== "):
            case = w
        assert g == w, f"line {i + 1}, case '{case}': got '{g}', recorded '{w}'"
    assert len(got) == len(want), f"{len(got)} lines, {len(want)} recorded"
    assert r.returncode == 0, "a launch with dynamic LDS had no reservation:\n" + "\n".join(l for l in got if "NOT RESERVED" in l)
    kernels = {l.split()[0] for l in want if l.startswith("  k_")}
    assert len(kernels) == 85, len(kernels)  # every instantiation these entry points can launch appears
