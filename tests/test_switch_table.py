"""The environment switches are stated once: `struct Switches` in rpsmf_amd/csrc/psmf_host.h is the native library's only reader of
the environment, DESIGN section 9 lists the same variables, and every one that selects a kernel or a schedule is named by a test.
tests/test_hip_switches.py ("a fallback nobody runs rots") is only as good as the list of what exists.  CPU only: reads sources."""

import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rpsmf_amd", "csrc")
NAME = r"PSMF_[A-Z0-9_]+"

# read outside the native library: rpsmf_amd/psmf.py, bench.py, rpsmf_amd/build.py
NOT_NATIVE = {"PSMF_RECOGNISE", "PSMF_COMM_INIT_TIMEOUT", "PSMF_CXXFLAGS"}

# Switches that no test sets: diagnostics and tuning overrides, which select no kernel and no schedule.  A cap -- it may shrink, not grow.
DIAGNOSTIC_ONLY = {"PSMF_PSTEP_PROF", "PSMF_DBG_BREAKDOWN", "PSMF_HOST_TIMING", "PSMF_COPY_GRID", "PSMF_NS_TOL", "PSMF_NS_FAR", "PSMF_NS_SKIP"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _switches_struct():
    """(text before, the struct, text after) of psmf_host.h"""
    text = _read(os.path.join(CSRC, "psmf_host.h"))
    m = re.search(r"^struct Switches \{\n.*?^\};\n", text, flags=re.S | re.M)
    assert m, "struct Switches not found in psmf_host.h"
    return text[:m.start()], m.group(0), text[m.end():]


def _struct_names():
    return set(re.findall(r'"(%s)"' % NAME, _switches_struct()[1]))


def _design_names():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## 9\. Switches.*?(?=^## |\Z)", text, flags=re.S | re.M)
    assert m, "DESIGN section 9 not found"
    rows = [l for l in m.group(0).splitlines() if l.startswith("|")]
    assert len(rows) > 10
    return set(re.findall(r"`(%s)" % NAME, "\n".join(rows)))


def test_switches_is_the_only_reader_of_the_environment():
    before, struct, after = _switches_struct()
    assert "getenv(" in struct
    assert "getenv(" not in before and "getenv(" not in after
    for f in sorted(os.listdir(CSRC)):
        if f != "psmf_host.h":
            assert "getenv(" not in _read(os.path.join(CSRC, f)), f"{f} reads the environment; that is struct Switches' job"


def test_struct_and_design_table_agree():
    struct, design = _struct_names(), _design_names()
    assert len(struct) >= 30
    assert struct - design == set(), "in struct Switches but not in the table of DESIGN section 9"
    assert design - struct - NOT_NATIVE == set(), "in the table of DESIGN section 9 but read by nobody"


def test_every_switch_is_named_by_a_test_or_is_a_diagnostic():
    me = os.path.basename(__file__)
    tests = "\n".join(_read(os.path.join(ROOT, "tests", f)) for f in sorted(os.listdir(os.path.join(ROOT, "tests"))) if f.endswith(".py") and f != me)
    struct = _struct_names()
    untested = {v for v in struct if not re.search(r"\b%s\b" % v, tests)}
    assert untested - DIAGNOSTIC_ONLY == set(), "switches that no file under tests/ sets"
    assert DIAGNOSTIC_ONLY <= struct, "DIAGNOSTIC_ONLY names a switch that no longer exists"
