"""Who owns a device resource is stated by types: rpsmf_amd/csrc/psmf_own.h holds the owning types (Owned: a handle and the function
that destroys it -- events, streams, pinned memory; Buf: a buffer and its size) and is the only file of the native library that names
the HIP functions which allocate, create, free or destroy.  Everywhere else a create call that takes flags may stand at its use site,
writing through the put() of an owning object; the process-lifetime event chain of launch_pstep is the one named exception.
psmf_destroy deletes the handle and frees nothing by hand, and no host code leaves a function through `goto`.  CPU only: the first
tests read sources; the last compiles tests/native/own_check.cpp -- the same class text over counting host allocators -- with the
address and undefined-behaviour sanitizers and runs it as a child process (no device, and the test preloads nothing)."""

import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rpsmf_amd", "csrc")
OWN = "psmf_own.h"
CREATE = ("hipMalloc", "hipHostMalloc", "hipEventCreate", "hipEventCreateWithFlags", "hipStreamCreate", "hipStreamCreateWithFlags")
RELEASE = ("hipFree", "hipHostFree", "hipEventDestroy", "hipStreamDestroy")
ANY = re.compile(r"\b(%s)\b" % "|".join(CREATE + RELEASE))
# <create>(<owning object>.put(), ...: the out-argument is the object's own slot, which put() has emptied
THROUGH_PUT = re.compile(r"\b(%s)\s*\(\s*[A-Za-z_][\w.\[\]>-]*\.put\(\)\s*[,)]" % "|".join(CREATE))
PS_EVENT_LINE = "if (!g_ps_event[dev]) HIP_TRY(h, hipEventCreateWithFlags(&g_ps_event[dev], hipEventDisableTiming));"


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _files():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _body(text, head):
    """the text from `head` to the closing brace of the block it opens"""
    start = text.index(head)
    i = text.index("{", start)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[start:j + 1]
    raise AssertionError(f"unbalanced braces after {head!r}")


def test_the_patterns_tell_a_put_from_a_raw_out_argument():
    assert THROUGH_PUT.search("HIP_TRY(h, hipEventCreateWithFlags(h->evF[i].put(), hipEventDisableTiming));")
    assert THROUGH_PUT.search("hipHostMalloc(h->err_host.put(), sizeof(int), hipHostMallocMapped)")
    assert THROUGH_PUT.search("hipStreamCreateWithFlags(s.put(), hipStreamNonBlocking)")
    assert THROUGH_PUT.search("HIP_TRY(h, hipEventCreate(e0.put()));")
    assert not THROUGH_PUT.search("hipEventCreateWithFlags(&h->evS, hipEventDisableTiming)")
    assert not THROUGH_PUT.search("hipMalloc((void**)&h->st, n)")
    assert not THROUGH_PUT.search("hipFree(x.put(), 0)")
    assert [m.group(1) for m in ANY.finditer("hipFree(p); hipMallocAsync(q); hipHostMallocMapped; hipExtStreamCreateWithCUMask")] == ["hipFree"]


def test_only_psmf_own_h_names_the_functions_that_create_or_release():
    assert ANY.search(_read(OWN)), "psmf_own.h is where the create / release functions are named"
    ps_event_lines = 0
    for f in _files():
        if f == OWN:
            continue
        for n, line in enumerate(_read(f).splitlines(), 1):       # comments and strings too: the names appear nowhere else
            names = [m.group(1) for m in ANY.finditer(line)]
            if not names:
                continue
            if line.strip() == PS_EVENT_LINE:
                ps_event_lines += 1
                continue
            through_put = [m.group(1) for m in THROUGH_PUT.finditer(line)]
            assert names == through_put, f"{f}:{n}: {sorted(set(names))} outside psmf_own.h and not a create call through put(): {line.strip()}"
    assert ps_event_lines == 1, "the event chain of launch_pstep (psmf_step.hip) is the one exception, on one line"


def test_psmf_destroy_releases_nothing_by_hand():
    body = _body(_read("psmf_capi.hip"), "void psmf_destroy(psmf_handle h)")
    assert "delete h;" in body and "destroy_graph(h);" in body and "ncclCommDestroy(" in body
    for name in RELEASE:
        assert name not in body, f"psmf_destroy names {name}: the members release themselves"
    assert len(body.splitlines()) <= 12, "psmf_destroy is the short list of what is not plain ownership"


def test_no_host_code_uses_goto():
    for f in _files():
        assert not re.search(r"\bgoto\b", _strip_comments(_read(f))), f"{f}: goto (an owning local releases on every return)"


def test_the_handle_keeps_no_size_beside_a_buffer():
    struct = _strip_comments(_body(_read("psmf_host.h"), "struct psmf_filter {"))
    fields = set(re.findall(r"\b(\w+(?:_cap|_bytes))\b\s*(?:=[^;,]*)?[;,]", struct))
    assert {"th_cap", "T_cap"} <= fields, fields        # element and row counts: they stay
    assert fields == {"th_cap", "T_cap"}, f"{sorted(fields - {'th_cap', 'T_cap'})}: a buffer's size is its bytes()"
    for raw in re.findall(r"^\s*(?:hipStream_t|hipEvent_t)\s+\w+", struct, flags=re.M):
        raise AssertionError(f"psmf_filter holds a raw {raw.split()[0]}: {raw.strip()}")


def test_own_check_runs_clean_under_the_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "own_check")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-g",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",      # host code only
           os.path.join(ROOT, "tests", "native", "own_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)      # (the program links its sanitizer runtime itself)
    assert ran.returncode == 0 and "own_check OK" in ran.stdout, (ran.returncode, ran.stdout[-2000:], ran.stderr[-4000:])
