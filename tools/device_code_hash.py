#!/usr/bin/env python3
"""sha256 of the gfx950 device ELF of every library source: two checkouts whose lists are equal ship the same device code
(same instructions, LDS sizes, register counts, kernel descriptors), so a refactor of csrc/ can be proved on a CPU machine.
-cuid=fixed: without it two builds of one source differ in CUID-derived symbol names; the default bundled output is compressed
and never comparable. Extra arguments after -- go to hipcc (e.g. -- -DMGN_TIMELINE).
usage: python tools/device_code_hash.py [--csrc DIR] [-- HIPCC_FLAGS...]"""
import argparse, hashlib, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "graph-physics_amd"))
import _capi  # by path: the module alone needs neither torch nor a GPU

ap = argparse.ArgumentParser()
ap.add_argument("--csrc", default=os.path.dirname(_capi.SOURCES[0]), help="csrc/ of another checkout (its include/ is ../../include)")
ap.add_argument("extra", nargs="*", help="further hipcc flags, after --")
a = ap.parse_args()
csrc = os.path.abspath(a.csrc)
inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")

def one(name):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, name + ".o")
        cmd = [_capi.hipcc_path(), "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-cuid=fixed", "-O3", "-std=c++17"]
        r = subprocess.run(cmd + _capi.DEVICE_FLAGS + a.extra + ["-I", inc, "-c", os.path.join(csrc, name), "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"hipcc failed on {name}:\n{r.stdout}{r.stderr}")
        with open(out, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest(), r.stderr

names = [os.path.basename(s) for s in _capi.SOURCES]
with ThreadPoolExecutor(len(names)) as ex:
    for name, (h, warn) in zip(names, ex.map(one, names)):
        sys.stderr.write(warn)
        print(f"{h}  {name}")
