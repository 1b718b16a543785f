"""tests/decision_path_cases.py without a GPU: the list covers what it says it covers, and every problem is admissible by the
rule of tests/blocked_cases.py -- the float64 oracle's own answer moves by at most 1/16 of the case's bar when the inputs move by
one bit of their storage type -- with at most one case in eight redrawn (decision_path_cases.REDRAWN)."""

import numpy as np
import pytest

import blocked_cases as BC
import decision_path_cases as DP

CASES = DP.cases()
PROBLEMS = {DP.problem_key(cs): cs for cs in CASES}


def test_coverage():
    names = [cs["name"] for cs in CASES]
    assert len(set(names)) == len(names)
    for r, kernel in DP.SHAPES.items():
        mine = [cs for cs in CASES if cs["r"] == r]
        assert all(BC.expected_kernel(cs) == kernel for cs in mine)
        assert all(cs["T"] == 2 * cs["B"] + 1 for cs in mine)
        for robust in (False, True):
            assert {cs["path"] for cs in mine if cs["robust"] == robust} >= {"one", "two", "more", "sweep"}, (r, robust)
            assert {cs["path"] for cs in mine if cs["robust"] == robust and cs["storage"] == "f64"} >= {"two", "more", "sweep"}, (r, robust)
        assert any(cs["storage"] == "f32" for cs in mine), r
    assert any(cs["d"] == 3 for cs in CASES)
    assert any(cs["env"].get("PSMF_BLOCK_CHAIN") == "0" for cs in CASES)
    assert all(cs["d"] in (DP.D_ROWS, 3) for cs in CASES)
    assert set(DP.REDRAWN) <= set(names)
    assert 8 * len(DP.REDRAWN) <= len(CASES)


def test_expect_reads_the_counters():
    cs = next(c for c in CASES if c["path"] == "one" and c["on_pass"] == 1)
    T = cs["T"]
    ok = dict(ns_steps=T, sweep_steps=0, ns_iterations=T + 2, ns_failed=0)
    assert DP.expect(cs, [ok, ok]) is None
    assert DP.expect(cs, [ok, dict(ok, ns_iterations=2 * T)]) is not None
    assert DP.expect(cs, [ok, dict(ok, ns_steps=T - 1, sweep_steps=1)]) is not None
    assert DP.expect(cs, [dict(ok, ns_steps=T - 1), ok]) is not None
    cs = next(c for c in CASES if c["path"] == "two" and c["on_pass"] == 0)
    first = dict(ns_steps=T - 1, sweep_steps=1, ns_iterations=2 * (T - 1), ns_failed=0)
    assert DP.expect(cs, [first, ok]) is None
    assert DP.expect(cs, [dict(first, ns_iterations=3 * T), ok]) is not None
    cs = next(c for c in CASES if c["path"] == "sweep")
    T = cs["T"]
    assert DP.expect(cs, [ok, dict(ns_steps=0, sweep_steps=T, ns_iterations=T // 3 + 1, ns_failed=T // 3 + 1)]) is None
    assert DP.expect(cs, [ok, ok]) is not None
    cs = next(c for c in CASES if c["path"] == "more")
    assert DP.expect(cs, [ok, dict(ok, ns_iterations=4 * T)]) is None
    assert DP.expect(cs, [ok, dict(ok, ns_iterations=2 * T)]) is not None


@pytest.mark.parametrize("key", sorted(PROBLEMS, key=str), ids=lambda k: f"r{k[0]}-{'rPSMF' if k[1] else 'PSMF'}-{k[2]}-d{k[3]}-rho{k[5]:g}-q{k[6]:g}")
def test_problem_is_admissible(key):
    cs = PROBLEMS[key]
    ok, state = DP.admissible(cs)
    print(f"\n{key}: sensitivity {state:.3e}, bar {BC.bar(cs):.0e}")
    assert ok, (key, state, BC.bar(cs))
    assert np.isfinite(state)
