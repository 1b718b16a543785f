"""The entry points without a handle (psmf_impute_run, psmf_impute_run_rows, psmf_ssm_run, psmf_ssm_run_ex, psmf_bocpd_run, psmf_pmf_run,
psmf_bpmf_run) share one host scaffold, rpsmf_amd/csrc/psmf_batch.h: the failure functor, the device check, typed transfers, the chunk
plan with its memory query, the per-item slots, the timed launch and the closing status loop are written there and nowhere else.  CPU
only: the first tests read sources, in the manner of tests/test_native_ownership.py; the last compiles tests/native/batch_check.cpp --
the transfer helpers, the per-item slots and the chunk plan over memcpy, counting host allocators and a made-up memory query -- with the
address and undefined-behaviour sanitizers and runs it as a child process (no device, and the test preloads nothing)."""

import os
import re
import subprocess

from conftest import ROOT
from test_native_ownership import _body, _read, _strip_comments

UNITS = ("psmf_impute.hip", "psmf_ssm.hip", "psmf_bocpd.hip", "psmf_pmf.hip", "psmf_bpmf.hip")
CHUNKED = ("psmf_bocpd.hip", "psmf_pmf.hip", "psmf_bpmf.hip")       # the batch goes through the device in chunks
BATCH = "psmf_batch.h"
# what the scaffold does for its users: transfers, event timing, the device check, the memory query of the chunk plan
SCAFFOLD_CALLS = ("hipMemcpy(", "hipMemcpyAsync(", "hipMemset(", "hipEventRecord(", "hipEventSynchronize(", "hipEventElapsedTime(", "hipGetDeviceCount(",
                  "hipSetDevice(", "hipLaunchKernel(", "hipFuncSetAttribute(", "hipMemGetInfo(")


def _host_part(name):
    """the unit's text behind its last kernel, comments stripped (the whole of it where the kernels live in included files)"""
    text = _strip_comments(_read(name))
    starts = [m.start() for m in re.finditer(r"__global__", text)]
    return text[starts[-1] + len(_body(text[starts[-1]:], "__global__")):] if starts else text


def test_the_host_part_starts_behind_the_last_kernel():
    assert "__global__" not in _read("psmf_impute.hip"), "the impute kernels live in the files psmf_impute.hip includes"
    for unit in UNITS:
        host = _host_part(unit)
        assert "__global__" not in host and "extern \"C\"" in host and "EntryFail" in host, unit
    assert "psmf_bocpd_post_kernel(BocpdParams p)" not in _host_part("psmf_bocpd.hip") and "int bocpd_run(" in _host_part("psmf_bocpd.hip")
    assert "int ssm_run(" in _host_part("psmf_ssm.hip")


def test_the_units_leave_transfers_timing_and_the_device_check_to_the_scaffold():
    batch = _read(BATCH)
    for call in ("hipMemcpy", "hipMemset(", "hipEventRecord(", "hipEventSynchronize(", "hipEventElapsedTime(", "hipGetDeviceCount(", "hipSetDevice(",
                 "hipLaunchKernel(", "hipFuncSetAttribute(", "hipMemGetInfo("):
        assert call in batch, f"{BATCH} is where {call} is written"
    for unit in UNITS:
        host = _host_part(unit)
        assert f'#include "{BATCH}"' in _read(unit)
        for call in SCAFFOLD_CALLS:
            assert call not in host, f"{unit}: {call} outside {BATCH}"
        by_hand = [m.group(0).strip() for m in re.finditer(r"[^;{}\n]*\*\s*[48]\b[^;\n]*", host)]
        assert not by_hand, f"{unit}: an element size written by hand: {by_hand}"
        for m in re.finditer(r"\bstruct\s+(\w*)\s*\{[^}]*operator\(\)", host):
            raise AssertionError(f"{unit}: a functor of its own (struct {m.group(1)}): the failure functor is EntryFail")
        assert "g_create_error" not in host or unit == "psmf_impute.hip", f"{unit}: g_create_error is written by EntryFail"


def test_the_chunk_plan_and_the_per_item_transfers_are_the_scaffolds():
    batch = _strip_comments(_read(BATCH))
    assert "16 << 30" in batch and "budget" in batch and "int plan_chunk(" in batch
    for name in sorted(n for n in os.listdir(os.path.join(ROOT, "rpsmf_amd", "csrc")) if n.endswith(".hip")):
        text = _read(name)      # (comments included; psmf_capi.hip speaks of a kernel's "register budget", which is no memory budget)
        assert "hipMemGetInfo" not in text and "16 << 30" not in text and "budget" not in text.replace("register budget", ""), \
            f"{name}: the chunk plan is plan_chunk in {BATCH}"
    for unit in CHUNKED:
        host = _host_part(unit)
        assert "plan_chunk(fail, B, " in host and "alloc_items(fail, items, chunk)" in host, unit
        assert "fill_items(fail, items, s0, ns)" in host and "read_items(fail, items, s0, ns)" in host, unit
        # a per-item buffer is stated once, in its slot: the chunk loop moves and clears nothing by name
        loop = _body(host[host.index("for (int s0 = 0;"):], "for (int s0 = 0;")
        for call in ("copy_in(", "copy_out(", "zero_n(", "alloc_n("):
            assert call not in loop, f"{unit}: {call} inside the chunk loop"
    for unit in ("psmf_pmf.hip", "psmf_bpmf.hip"):
        host = _host_part(unit)
        assert "cols_per_workgroup(n, sw." in host and "isfinite(v[i])" not in host and "all_finite(" in host, unit


def test_g_create_error_is_written_by_the_failure_functor_alone():
    """... and by the large path of psmf_impute_run, which passes on the message of the handle it ran on"""
    lines = [ln.strip() for ln in _strip_comments(_read("psmf_impute.hip")).splitlines() if "g_create_error" in ln]
    assert len(lines) == 1 and lines[0].startswith("auto bail = ") and '"psmf_impute_run: ") + psmf_last_error(h)' in lines[0], lines
    assert "g_create_error = std::string(who) + \": \" + msg" in _read(BATCH)


def test_the_large_path_lives_with_its_engine_and_owns_its_handle():
    assert "impute_run_large" not in _read("psmf_capi.hip") and "impute_run_large" not in _read("psmf_host.h")
    text = _strip_comments(_read("psmf_impute.hip"))
    assert "int impute_run_large(" in text
    uses = [ln.strip() for ln in text.splitlines() if "psmf_destroy(" in ln]
    assert uses == ["hipError_t destroy_filter(psmf_handle h) { psmf_destroy(h); return hipSuccess; }"], uses
    assert "Owned<psmf_handle, destroy_filter>" in text
    body = _body(text, "int impute_run_large(")
    assert "psmf_create(h.put(), &pc)" in body and "failc" not in body
    # the message is read while the handle is alive: inside the function, whose return releases it
    assert 'if (code) g_create_error = std::string("psmf_impute_run: ") + psmf_last_error(h); return code;' in body


def test_the_scaffold_stands_without_the_rest_of_the_host_code():
    batch = _read(BATCH)
    includes = re.findall(r'#include\s+"([^"]+)"', batch)
    assert sorted(includes) == ["../../include/psmf_hip.h", "psmf_own.h"], includes
    assert "extern thread_local std::string g_create_error;" in batch
    assert not re.search(r"\bclass\b|\bvirtual\b", _strip_comments(batch)), "plain functions and small structs"


def test_batch_check_runs_clean_under_the_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "batch_check")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-g",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",      # host code only
           os.path.join(ROOT, "tests", "native", "batch_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)      # (the program links its sanitizer runtime itself)
    assert ran.returncode == 0 and "batch_check OK" in ran.stdout, (ran.returncode, ran.stdout[-2000:], ran.stderr[-4000:])
