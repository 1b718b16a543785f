"""The translation units of the native library (rpsmf_amd/build.py: _units()) and the include graph under rpsmf_amd/csrc: every file
belongs to a unit, a file that defines a non-template __global__ kernel belongs to exactly one (a second unit including it would
define the kernel twice), includes stand at the top of a file, and a unit's dependency scan -- what decides whether its object is
stale -- starts with the unit itself.  CPU only: reads sources, compiles nothing."""

import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rpsmf_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))


def _units():
    from rpsmf_amd import build

    return build._units()


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _defines_plain_global(text):
    """does the text define a __global__ function that is not a template?"""
    lines = _strip_comments(text).splitlines()
    for i, line in enumerate(lines):
        if "__global__" not in line or line.lstrip().startswith("#"):
            continue
        head = line.split("__global__")[0].strip()
        j = i - 1
        while not head and j >= 0 and not lines[j].strip():
            j -= 1
        before = head if head else (lines[j].strip() if j >= 0 else "")
        if not before.startswith("template"):
            return True
    return False


def test_the_detector_tells_templates_from_plain_kernels():
    assert _defines_plain_global("__global__ void k(int) {}\n")
    assert _defines_plain_global("// c\n__global__ __launch_bounds__(64) void k(int) {}\n")
    assert not _defines_plain_global("template <int N>\n__global__ void k(int) {}\n")
    assert not _defines_plain_global("template <int N> __global__ void k(int) {}\n")
    assert not _defines_plain_global("// a __global__ kernel lives elsewhere\n")


def test_every_source_file_is_reached_by_a_unit():
    reached = set()
    for _obj, _src, deps, _extra in _units():
        reached.update(deps)
    missing = [os.path.basename(p) for p in _csrc_files() if p not in reached and os.path.basename(p) != "psmf_buildid.cpp"]
    assert missing == [], f"under rpsmf_amd/csrc but compiled into no unit: {missing}"
    assert os.path.join(CSRC, "psmf_buildid.cpp") in _csrc_files()      # the build identity: a unit of its own, compiled by build_library


def test_a_file_with_a_plain_global_kernel_belongs_to_exactly_one_unit():
    units = _units()
    n_checked = 0
    for p in _csrc_files():
        if not _defines_plain_global(_read(p)):
            continue
        n_checked += 1
        owners = [os.path.basename(src) for _obj, src, deps, _extra in units if p in deps]
        assert len(owners) == 1, f"{os.path.basename(p)} defines a non-template __global__ kernel and is reached by {owners}"
    assert n_checked >= 7      # psmf_kernels, psmf_block, psmf_masked, psmf_blk16, psmf_blk32, psmf_blk34, psmf_impute2


def test_the_c_abi_unit_reaches_no_engine_kernels():
    """psmf_capi.hip is the glue: the per-step engine, the blocked engine and the rotation are launched by their own units"""
    deps = {os.path.basename(d) for _obj, src, ds, _extra in _units() if os.path.basename(src) == "psmf_capi.hip" for d in ds}
    assert "psmf_capi.hip" in deps and "psmf_host.h" in deps, deps
    engine_files = {"psmf_kernels.hip", "psmf_masked.hip", "psmf_wave16.hip", "psmf_ns.hip", "psmf_rotate.hip", "psmf_block.hip", "psmf_blk3.hip"}
    assert all(os.path.isfile(os.path.join(CSRC, f)) for f in engine_files)      # (a renamed file would pass the next line unseen)
    assert deps & engine_files == set(), f"psmf_capi.hip reaches {sorted(deps & engine_files)}"


def test_includes_stand_at_the_top_of_a_file():
    for p in _csrc_files():
        code_seen = None
        for n, line in enumerate(_strip_comments(_read(p)).splitlines(), 1):
            s = line.strip()
            if not s:
                continue
            if s.startswith("#"):
                assert not (code_seen and re.match(r'#\s*include\s*"', s)), \
                    f'{os.path.basename(p)}:{n}: #include "..." after code (line {code_seen})'
            elif code_seen is None:
                code_seen = n


def test_a_units_dependency_scan_contains_the_unit_and_the_public_header_where_reached():
    header = os.path.join(ROOT, "include", "psmf_hip.h")
    units = _units()
    assert len(units) >= 4
    for _obj, src, deps, _extra in units:
        assert src in deps, f"{os.path.basename(src)}: its own source is not among the files that decide staleness"
        assert all(os.path.isfile(d) for d in deps)
        text = "".join(_read(d) for d in deps)
        assert (header in deps) == ("include/psmf_hip.h" in text)
