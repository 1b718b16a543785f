"""Builds the native pieces in-tree with hipcc (cross-compiles for gfx950 without a GPU).

    python -m rpsmf_amd.build            # libpsmf_hip.so  (only what is stale)
    python -m rpsmf_amd.build --force    # everything from source

The library is a handful of translation units, compiled side by side (at most 16 at a time) and linked: the C ABI (psmf_capi.hip), the launched
per-step engine with the host driver of the persistent one (psmf_step.hip), the communicator (psmf_comm.hip), the noise rotation
(psmf_rotation.hip), the series buffers -- resident or a ring: uploads, downloads, reductions over stored rows --
(psmf_series.hip), the blocked engine's host driver and kernels (psmf_blocked.hip), the filter3 family of block filters
(psmf_filter34.hip), the persistent per-step engine (psmf_pstep.hip), the four units of the entry points without a handle, host side on
psmf_batch.h -- the masked small-shape engine with its route to the large-d handle (psmf_impute.hip), the batched filter with linear-Gaussian
dynamics and an observation map (psmf_ssm.hip), the batched Bayesian online change-point detection (psmf_bocpd.hip), the batched
probabilistic matrix factorisation (psmf_pmf.hip) and its Bayesian form, the Gibbs sampler (psmf_bpmf.hip) -- the convergence
experiment, one lane per replica (psmf_conv.hip), also on psmf_batch.h,
and the build identity (psmf_buildid.cpp: `psmf_build_id()` returns the SHA-256 of every source file and of the compiler flags the library was built
from).  An object is stale when the hash of what its source reaches through `#include "..."`, followed transitively, differs from the one
it was compiled from -- no list of dependencies is kept by hand.  `build_library` rebuilds whenever the whole-library hash differs from
the sources on disk -- modification times play no part -- and `source_hash()` / `library_build_id()` let `__graft_entry__.build()`
prove that the shipped binary is the compiled form of the shipped sources.
"""

import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libpsmf_hip.so")
HEADER = os.path.join(ROOT, "include", "psmf_hip.h")

# -amdgpu-mfma-vgpr-form: MFMAs with VGPR accumulators in every kernel.  By default the compiler takes that form only
# when a wave is limited to 256 registers (512-thread workgroups); the 256-thread kernels got accumulators in AGPRs and a
# copy in and out around every dependent MFMA.  With the flag they keep all 512 registers AND the short form, and what
# does not fit the 256 VGPRs is parked in AGPRs (one instruction) instead of scratch memory.
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wno-unused-value", "-mllvm", "-amdgpu-mfma-vgpr-form"]
FLAGS += os.environ.get("PSMF_CXXFLAGS", "").split()      # diagnostic builds (e.g. -DPSTEP_PROF); part of the build id
LINK = ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]

UNITS = ("psmf_capi.hip", "psmf_series.hip", "psmf_blocked.hip", "psmf_filter34.hip", "psmf_impute.hip", "psmf_pstep.hip", "psmf_ssm.hip",
         "psmf_bocpd.hip", "psmf_pmf.hip", "psmf_bpmf.hip", "psmf_conv.hip", "psmf_step.hip", "psmf_comm.hip", "psmf_rotation.hip")
# psmf_conv.hip: no contraction of a * b + c by the compiler -- the unit writes its fused multiply-adds out, so that the instances of
# a shape (shared data, own data) are the same arithmetic and give the same bits
UNIT_FLAGS = {"psmf_conv.hip": ["-ffp-contract=off"]}
MAX_JOBS = 16


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))


def _hash_files(paths, extra=""):
    h = hashlib.sha256()
    h.update((" ".join(FLAGS + LINK) + extra).encode())
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def source_hash():
    """SHA-256 over every file of rpsmf_amd/csrc, include/psmf_hip.h and the compiler flags."""
    return _hash_files(_sources() + [HEADER])


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def _reached(src):
    """the files `src` reaches through #include "...", followed transitively; `src` itself first"""
    seen, todo = [], [os.path.normpath(src)]
    while todo:
        p = todo.pop()
        if p in seen:
            continue
        seen.append(p)
        with open(p, encoding="utf-8") as f:
            text = f.read()
        todo += [os.path.normpath(os.path.join(os.path.dirname(p), inc)) for inc in _INCLUDE.findall(text)]
    return [seen[0]] + sorted(seen[1:])


def _units():
    """(object name, source, files whose content decides whether the object is stale, extra flags)"""
    return [(u.replace(".hip", ".o"), os.path.join(CSRC, u), _reached(os.path.join(CSRC, u)), UNIT_FLAGS.get(u, [])) for u in UNITS]


def library_build_id():
    """what the library on disk says it was built from ('' if it is missing or predates psmf_build_id); read from the file's
    bytes, not through dlopen: a process that has already mapped a stale library would be handed the same image again"""
    if not os.path.exists(LIB_PATH):
        return ""
    with open(LIB_PATH, "rb") as f:
        blob = f.read()
    i = blob.find(b"PSMF_BUILD_ID=")
    if i < 0:
        return ""
    return blob[i + 14:i + 14 + 64].decode("ascii", "replace")


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_library(force=False, verbose=True):
    """hipcc --offload-arch=gfx950 -> rpsmf_amd/lib/libpsmf_hip.so; returns its path.  Compiles nothing when the library's
    build id equals the hash of the sources on disk."""
    want = source_hash()
    if not force and library_build_id() == want:
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I", os.path.join(ROOT, "include")]
    jobs = []
    for obj, src, deps, extra in _units():
        out = os.path.join(OBJ_DIR, obj)
        stamp = out + ".sha256"
        dep_hash = _hash_files(deps, " ".join(extra))
        fresh = (not force and os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == dep_hash)
        if not fresh:
            jobs.append((out, stamp, dep_hash, [hipcc] + FLAGS + extra + inc + ["-c", src, "-o", out]))

    def compile_one(job):
        out, stamp, dep_hash, cmd = job
        if os.path.exists(stamp):
            os.remove(stamp)
        _run(cmd, verbose)
        with open(stamp, "w") as f:
            f.write(dep_hash)

    with ThreadPoolExecutor(max_workers=max(1, min(MAX_JOBS, len(jobs)))) as ex:
        list(ex.map(compile_one, jobs))
    idobj = os.path.join(OBJ_DIR, "psmf_buildid.o")
    _run([hipcc, "-O2", "-std=c++17", "-fPIC", "-x", "c++", f'-DPSMF_BUILD_ID="{want}"'] + inc + ["-c", os.path.join(CSRC, "psmf_buildid.cpp"), "-o", idobj], verbose)
    objs = [os.path.join(OBJ_DIR, u[0]) for u in _units()] + [idobj]
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs + LINK, verbose)
    got = library_build_id()
    if got != want:
        raise RuntimeError(f"{LIB_PATH} reports build id {got!r}, expected {want!r}")
    return LIB_PATH


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(f"{LIB_PATH}: build id {library_build_id()[:16]}...")
