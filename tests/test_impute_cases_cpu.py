"""tests/impute_cases.py without a GPU: (1) the seeded case list of the masked one-workgroup engine's random-configuration net
covers what it claims to cover -- all twelve kernel instances with every method they take, every row edge of both column loops,
r = 15 / 16 on kernel2 and kernel2w at small and at large d, every series length (n >= 256, a second round of the held-out sums
over the 256 threads, on every instance), one / two / three passes, every band factor and lambda0, dense V0 / P0 and a general Q
on every instance, both noise-vector edges, batches of different replicas, both switches -- so that the net cannot go thin
unnoticed; (2) every case is admissible by the oracle alone: it runs every replica to finite values (bands included), its answer
moves by at most 1/16 of the case's bar when C0, X0 and Y move by a relative 2^-50, and no held-out entry lies within
1e-6 max(1, |y|) of a band edge, so that the exact coverage count cannot flip on rounding.  A case that is not admissible is
halved in n (not below 2, at most twice), then redrawn; impute_cases.RESOLUTION records the outcome and this file recomputes it.
Wall time: about a minute on one core.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73 (through oracle/impute_oracle.py)."""

from collections import Counter

import numpy as np
import pytest

import impute_cases as IC

CASES = [IC.device_case(i) for i in range(IC.N_CASES)]
KERNEL2 = ("psmf_impute_kernel2", "psmf_impute_kernel2w")


def _unequal(cs):
    return IC.facts(cs)["row_noise"]


def test_the_case_list_is_what_the_table_says():
    assert len(IC.TARGETS) == 42 and IC.N_CASES == 3 * len(IC.TARGETS) == 126 and len(IC.INSTANCES) == 12
    assert len(set(IC.TARGETS)) == 42 and {k for k, _ in IC.TARGETS} == set(IC.INSTANCES)
    assert all(m != "tmf" for k, m in IC.TARGETS if k in IC.ROW_NOISE)
    hits = Counter()
    for i, cs in enumerate(CASES):
        assert (IC.expected_kernel(cs), cs["method"]) == IC.TARGETS[i % len(IC.TARGETS)] == (cs["instance"], cs["method"]), i
        hits[(cs["instance"], cs["method"])] += 1
        assert 1 <= cs["d"] <= 512 and 1 <= cs["r"] <= 16 and 2 <= cs["n"] <= 300 and cs["batch"] in (1, 2, 3)
        assert cs["n_iter"] in IC.N_ITER and cs["sig"] in IC.SIGS and cs["lambda0"] in IC.LAMBDAS and cs["frac"] in IC.FRACTIONS
        assert set(cs["env"]) <= {"PSMF_IMPUTE_V3", "PSMF_IMPUTE_PAR"}
        assert cs["r"] <= 14 or cs["instance"] in KERNEL2
        # the default dispatch: kernel3 serves d <= 80 with r <= 14, kernel2 the rest; PSMF_IMPUTE_V3=0 moves the small shapes
        small = cs["d"] <= 80 and cs["r"] <= 14
        assert (cs["instance"] in KERNEL2) == (not small or cs["env"].get("PSMF_IMPUTE_V3") == "0"), cs
        assert _unequal(cs) == (cs["instance"] in IC.ROW_NOISE)
    print("\ncases per target:", dict(hits))
    assert set(hits) == set(IC.TARGETS) and min(hits.values()) >= 3, hits


def test_the_problem_of_a_case_is_what_the_table_says():
    for cs in CASES:
        pb = IC.problem(cs)
        d, n, r, B = cs["d"], cs["n"], cs["r"], cs["batch"]
        assert pb["M"].shape == pb["Mmiss"].shape == (B, d, n) and pb["C0"].shape == (B, d, r) and pb["X0"].shape == (B, r, n)
        for a in ("V", "P", "Q"):
            assert np.array_equal(pb[a], pb[a].T) and np.all(np.linalg.eigvalsh(pb[a]) > 0), (cs["i"], a)
        assert bool(np.count_nonzero(pb["V"] - np.diag(np.diag(pb["V"])))) == (cs["dense"] and r > 1)
        assert bool(np.count_nonzero(pb["Q"] - np.diag(np.diag(pb["Q"])))) == (cs["general_Q"] and r > 1)
        for b in range(B):
            M, Mm = pb["M"][b], pb["Mmiss"][b]
            assert set(np.unique(M)) <= {0, 1} and not np.any(Mm * M) and Mm.sum() >= 1, cs["i"]      # held out: never an observed entry
            empty = int(np.sum(M.sum(axis=0) == 0))
            want_empty = d >= 12 and n >= 4 and cs["method"] != "mle_smf" and r >= 3          # (r <= 2: impute_cases.empty_column)
            assert want_empty == IC.empty_column(cs)
            assert empty == int(want_empty) or (d <= 3 and empty <= 1 and cs["method"] != "mle_smf"), (cs["i"], empty)
            if d > 3:
                assert np.any(M.sum(axis=1) == 0)          # a row that is never observed
                if n >= 6:
                    assert np.any(M.sum(axis=0) == d - 1)      # a column observed on every other row
            elif n >= 6:
                assert np.any(M.sum(axis=0) == d)
        # the replicas are different problems
        for b in range(1, B):
            assert not np.array_equal(pb["C0"][b], pb["C0"][0]) and not np.array_equal(pb["X0"][b], pb["X0"][0])
            assert d * n < 8 or not np.array_equal(pb["M"][b], pb["M"][0])


def test_every_instance_sees_dense_priors_a_general_Q_and_a_long_series():
    dense, genq, long_ = {}, Counter(), Counter()
    for cs in CASES:
        if cs["dense"] and cs["r"] > 1 and cs["method"] != "tmf":          # (TMF reads neither V nor P)
            dense.setdefault(cs["instance"], set()).add(cs["method"])
        genq[cs["instance"]] += cs["general_Q"] and cs["r"] > 1 and cs["method"] != "tmf"
        long_[cs["instance"]] += cs["n"] >= 256
    print("\nmethods with dense V0 / P0 per instance:", {k: sorted(v) for k, v in dense.items()})
    print("general Q per instance:", dict(genq), "\nn >= 256 per instance:", dict(long_))
    for k in IC.INSTANCES:
        assert len(dense.get(k, ())) >= 2 and genq[k] >= 1 and long_[k] >= 1, k
    assert any(cs["general_Q"] and cs["r"] > 1 and cs["instance"] == "psmf_impute_kernel2" and cs["d"] > 80 and cs["method"] != "tmf" for cs in CASES)
    assert any(cs["general_Q"] and cs["r"] > 1 and cs["instance"] in IC.ROW_NOISE for cs in CASES)
    # TMF and MLE-SMF on kernel2's own shapes
    for m in IC.METHODS:
        assert any(cs["instance"] == "psmf_impute_kernel2" and cs["method"] == m and cs["d"] > 80 for cs in CASES), m


def test_every_row_edge_and_rank():
    for group, edges in ((("psmf_impute_kernel3",), IC.D_EDGES3), (KERNEL2, IC.D_EDGES2)):
        seen = Counter(cs["d"] for cs in CASES if cs["instance"].startswith(group))
        print("\nrow edges of", group[0], {d: seen[d] for d in edges})
        assert all(seen[d] >= 1 for d in edges), seen
    for k in KERNEL2:
        mine = [cs for cs in CASES if cs["instance"] == k]
        assert {cs["d"] % 4 for cs in mine} == {0, 1, 2, 3}, k
        for r in (15, 16):
            assert any(cs["r"] == r and cs["d"] <= 80 for cs in mine) and any(cs["r"] == r and cs["d"] > 256 for cs in mine), (k, r)
        # the small shapes that only the switch sends here
        assert any(cs["d"] <= 80 and cs["r"] <= 14 and cs["env"].get("PSMF_IMPUTE_V3") == "0" for cs in mine), k
    ranks = Counter(cs["r"] for cs in CASES)
    print("ranks:", dict(sorted(ranks.items())))
    assert all(ranks[r] >= 1 for r in IC.R_LIST + (15, 16))
    rel = Counter(("r=d-1" if cs["r"] == cs["d"] - 1 else "r=d" if cs["r"] == cs["d"] else "r=d+1" if cs["r"] == cs["d"] + 1 else
                   "r>d" if cs["r"] > cs["d"] else "r<d") for cs in CASES)
    print("rank against rows:", dict(rel))
    assert all(rel[k] >= 1 for k in ("r=d-1", "r=d", "r=d+1", "r>d", "r<d")), rel
    assert any(cs["r"] > cs["d"] + 1 for cs in CASES)


def test_every_series_length_pass_count_band_factor_and_lambda0():
    ns = Counter(cs["n"] for cs in CASES)
    print("\nseries lengths:", dict(sorted(ns.items())))
    assert all(ns[n] >= 1 for n in IC.N_LIST), ns
    iters = Counter((cs["method"] == "rpsmf", cs["n_iter"]) for cs in CASES)
    print("(rPSMF, passes):", dict(iters))
    assert all(iters[(rob, k)] >= 1 for rob in (True, False) for k in IC.N_ITER), iters
    sigs, lams = Counter(cs["sig"] for cs in CASES), Counter(cs["lambda0"] for cs in CASES if cs["method"] == "rpsmf")
    print("band factors:", dict(sigs), "lambda0 (rPSMF):", dict(lams))
    assert all(sigs[s] >= 1 for s in IC.SIGS) and all(lams[x] >= 1 for x in IC.LAMBDAS)
    assert {cs["sig"] for cs in CASES if cs["method"] in IC.BAND_METHODS} == set(IC.SIGS)          # sig != 2 where there is coverage
    assert {cs["frac"] for cs in CASES} == set(IC.FRACTIONS)


def test_batches_switches_and_noise_kinds():
    batches = Counter(cs["batch"] for cs in CASES)
    kinds = Counter((cs["R_kind"], cs["method"] == "tmf") for cs in CASES)
    print("\nbatch sizes:", dict(batches), "\n(noise kind, TMF):", dict(kinds))
    assert batches[2] + batches[3] >= 30 and batches[1] >= 1 and batches[2] >= 1 and batches[3] >= 1
    for name in ("PSMF_IMPUTE_V3", "PSMF_IMPUTE_PAR"):
        assert any(cs["env"].get(name) == "0" for cs in CASES), name
    assert any(cs["env"].get("PSMF_IMPUTE_PAR") == "0" and cs["instance"].startswith("psmf_impute_kernel3") for cs in CASES)
    assert any(cs["env"].get("PSMF_IMPUTE_PAR") == "0" and cs["instance"] in KERNEL2 for cs in CASES)
    for kind in ("scalar", "const_vector", "vector", "one_off"):
        assert kinds[(kind, False)] >= 1, kind
    assert {cs["rho"] for cs in CASES if cs["R_kind"] == "scalar"} == set(IC.RHOS)
    # a constant vector runs the scalar kernel and reports its name; so does TMF whatever vector it is given
    assert all(cs["instance"] in IC.UNIFORM for cs in CASES if cs["R_kind"] == "const_vector" or cs["method"] == "tmf")
    assert kinds[("vector", True)] + kinds[("one_off", True)] >= 1
    # the single differing entry: a last-bit difference and a plain one
    ratios = set()
    for cs in CASES:
        if cs["R_kind"] == "one_off" and cs["method"] != "tmf":
            R = IC.noise(cs)
            assert np.sum(R != cs["rho"]) == 1
            ratios.add(float(R[R != cs["rho"]][0] / cs["rho"]))
    assert ratios == {1.0 + 2.0 ** -52, 3.0}, ratios


def test_at_most_a_tenth_of_the_cases_was_shortened_or_replaced():
    print("\nshortened or replaced (case: (salt, times halved)):", IC.RESOLUTION)
    assert len(IC.RESOLUTION) <= IC.N_CASES // 10, len(IC.RESOLUTION)


@pytest.mark.parametrize("i", range(IC.N_CASES))
def test_case_is_admissible_by_the_oracle_alone(i):
    """No exception, finite, the oracle's response to a last-bit change of the inputs at most bar / 16, band margins kept: for
    the recorded resolution of the case, and -- for the cases the table lists -- not for the draw it replaced."""
    (salt, halved), log = IC.resolve(i)
    for line in log:
        print("\nnot admissible:", line)
    assert (salt, halved) == IC.RESOLUTION.get(i, (0, 0)), (i, salt, halved, log)
