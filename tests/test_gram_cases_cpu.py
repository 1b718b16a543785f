"""tests/gram_cases.py without a GPU: (1) the restated slab geometry of mgram_body is the table of that module's docstring;
(2) the seeded case list of the masked / weighted Gram net covers what it claims to cover -- every psmf_serial_mgram instance
under every reason that reaches it, every psmf_wgram_mfma instance and the vector-unit twin, every row edge of every NW class
(one slab per wave, a second slab of one row, three trips), every rank edge, both Q routes under a mask, 2 .. 4 uneven shards
with one below 16 rows and one pair that straddles the one-slab bound -- so that the net cannot go thin unnoticed; (3) every
case is well enough conditioned for its tolerance to mean something: the float64 oracle runs it to finite values, and its answer
moves by at most 1/16 of the case's bar when C0 and Y move by a relative 2^-50 (float32 storage: 2^-23, after the rounding).
A case that is not admissible is halved (at most twice), then redrawn; gram_cases.RESOLUTION records the outcome and this file
recomputes it.  No case is dropped on the device side: tests/test_hip_masked_gram_net.py runs range(N_CASES).
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73 (through oracle/)."""

from collections import Counter

import numpy as np
import pytest

import gram_cases as GC

CASES = [GC.device_case(i) for i in range(GC.N_CASES)]
MASKED = [cs for cs in CASES if cs["masked"]]
WEIGHTED = [cs for cs in CASES if not cs["masked"]]


def test_the_geometry_is_the_table_of_the_docstring():
    for r, nt, nw, bound in ((1, 1, 16, 65_536), (8, 1, 16, 65_536), (9, 1, 16, 65_536), (16, 1, 16, 65_536), (17, 2, 8, 32_768), (32, 2, 8, 32_768),
                             (33, 3, 4, 16_384), (48, 3, 4, 16_384), (49, 4, 4, 16_384), (64, 4, 4, 16_384)):
        p = GC.gram_plan(bound, r, "mgram")
        assert (p["nt"], p["nw"], p["n_wg"], p["bound"], p["trips"], p["last_rows"]) == (nt, nw, 256, bound, 1, 16), (r, p)
        q = GC.gram_plan(bound + 1, r, "mgram")
        assert (q["trips"], q["last_rows"], q["n_slab"]) == (2, 1, bound // 16 + 1), (r, q)
        assert GC.gram_plan(2 * bound + 2, r, "mgram")["trips"] == 3 and GC.gram_plan(1, r, "mgram")["trips"] == 1
        w = GC.gram_plan(32_768, r, "wgram")
        assert (w["nt"], w["nw"], w["trips"]) == (nt, 8, 1) and GC.gram_plan(32_769, r, "wgram")["trips"] == 2
    # the largest shapes of the suite before this net stayed on one trip
    assert GC.gram_plan(20_000, 10, "mgram")["trips"] == 1 and GC.gram_plan(3_001, 64, "wgram")["trips"] == 1 and GC.gram_plan(2_500, 48, "mgram")["trips"] == 1


def test_the_case_list_is_what_the_tables_say():
    assert len(GC.MASKED_TARGETS) == 36 and len(GC.WEIGHTED_TARGETS) == 10 and GC.N_CASES == len(GC.SPECS) == len(CASES)
    for i, cs in enumerate(CASES):
        assert GC.reached(cs) == GC.SPECS[i][0] == cs["target"], (i, cs["target"], GC.reached(cs))
        assert cs["parts"][0][0] == 0 and cs["parts"][-1][1] == cs["T"] and all(a < b for a, b in cs["parts"])
        assert all(p[1] == q[0] for p, q in zip(cs["parts"][:-1], cs["parts"][1:])), cs["parts"]
        assert 1 <= len(cs["parts"]) <= 3 and 1 <= cs["passes"] <= 3
        big = cs["d"] > GC.BIG_D
        assert (3 <= cs["T"] <= 6 and cs["passes"] == 1) if big else ((6 if cs["masked"] else 3) <= cs["T"] <= 30), cs
        assert not cs["shards"] or (2 <= len(cs["shards"]) <= 4 and sum(cs["shards"]) == cs["d"] and min(cs["shards"]) >= 1)
        if cs["masked"]:
            assert cs["d"] >= 8 and cs["r"] >= 2 and cs["T"] >= 5                     # step_cases.masked_ok; the marked columns
            assert not cs["empty_col"] or (cs["r"] >= 3 and cs["method"] != "mle_smf")
            assert 0.5 <= cs["rho"] <= 20 and 0.5 <= cs["lam"] <= 5 and 0.5 <= cs["sig"] <= 3
        else:
            assert cs["method"] in ("psmf", "rpsmf") and not (cs["rotated"] and (cs["shards"] or cs["d"] > 400))


def test_every_target_is_reached_by_every_method_that_reaches_it():
    hit = Counter(GC.reached(cs) for cs in CASES)
    print("\ncases per target:", dict(hit))
    assert set(hit) == set(GC.TARGETS), set(GC.TARGETS) ^ set(hit)
    # the ten psmf_serial_mgram instances x the methods: MLE-SMF and TMF on every one, PSMF and rPSMF between them on every one
    for cls in GC.CLASSES:
        for s in GC.STORAGES:
            methods = {cs["method"] for cs in MASKED if GC.class_of(cs["r"]) == cls and cs["storage"] == s}
            assert {"mle_smf", "tmf"} <= methods and methods & {"psmf", "rpsmf"}, (cls, s, methods)
        assert {"psmf", "rpsmf"} <= {cs["method"] for cs in MASKED if GC.class_of(cs["r"]) == cls}, cls
    # the eight psmf_wgram_mfma instances, the vector-unit twin once per storage, PSMF and rPSMF
    assert {t[1:3] for t in hit if t[0] == "w" and t[3] == "mfma"} == {(nt, s) for nt in (1, 2, 3, 4) for s in GC.STORAGES}
    assert {t[2] for t in hit if t[0] == "w" and t[3] == "valu"} == set(GC.STORAGES)
    assert {cs["method"] for cs in WEIGHTED} == {"psmf", "rpsmf"}
    # ranks: every class edge, an odd rank in every class of either mode
    ranks = {cs["r"] for cs in CASES}
    assert set(GC.RANK_EDGES) <= ranks, set(GC.RANK_EDGES) - ranks
    for group in (MASKED, WEIGHTED):
        for cls in GC.CLASSES:
            assert any(cs["r"] % 2 for cs in group if GC.class_of(cs["r"]) == cls), cls


def test_every_row_edge_and_every_trip_count():
    for g, (mode, nw, targets) in GC.GROUPS.items():
        mine = [cs for cs in CASES if cs["target"] in targets and not cs["shards"]]
        b = 16 * 256 * nw
        ds = {cs["d"] for cs in mine}
        assert set(GC.EDGES[g]) <= ds, (g, set(GC.EDGES[g]) - ds)
        assert {b - 1, b, b + 1, b + 17, 8, 15, 16, 17, 16 * nw - 1, 16 * nw + 1, 4095, 4097} <= set(GC.EDGES[g])
        assert any(2 * b < d < 3 * b and d % 16 not in (0, 1) for d in GC.EDGES[g])
        plans = [GC.plan_of(cs) for cs in mine]
        assert all(p["nw"] == nw and p["bound"] == b for p in plans), g
        assert any(p["trips"] == 1 for p in plans) and any(p["trips"] >= 3 for p in plans), g
        assert any(p["trips"] == 2 and p["last_rows"] == 1 and p["n_slab"] == p["stride"] + 1 for p in plans), g
        assert any(p["trips"] == 1 and p["n_slab"] == p["stride"] and p["last_rows"] == 16 for p in plans), g       # exactly one slab per wave
        assert any(p["n_slab"] == 1 and p["last_rows"] < 16 for p in plans), g                                        # 255 idle workgroups
        # a big-row case in both storages
        assert {cs["storage"] for cs in mine if GC.plan_of(cs)["trips"] >= 2} == set(GC.STORAGES), g


def test_masks_and_both_inversion_routes_under_a_mask():
    assert any(cs["general_Q"] for cs in MASKED) and any(not cs["general_Q"] for cs in MASKED)
    for method in ("psmf", "rpsmf", "mle_smf"):
        assert {cs["general_Q"] for cs in MASKED if cs["method"] == method} == {False, True}, method
    assert {cs["general_Q"] for cs in MASKED if GC.plan_of(cs)["trips"] >= 2 and cs["method"] != "tmf"} == {False, True}
    assert sum(1 for cs in MASKED if cs["route"] == "batch") >= len(MASKED) // 5 and any(cs["route"] == "batch" and cs["passes"] > 1 for cs in MASKED)
    assert any(cs["restate"] for cs in MASKED) and any(len(cs["parts"]) == 3 for cs in MASKED)
    assert any(2 in [b for _, b in cs["parts"][:-1]] for cs in MASKED if cs["empty_col"]) and any(4 in [b for _, b in cs["parts"][:-1]] for cs in MASKED)
    seen_two_trip = False
    for cs in MASKED:
        if cs["d"] > 70_000 and seen_two_trip:
            continue                    # (the marked columns are the same code: one big mask is enough here)
        M, p = GC.problem(cs)["M"], GC.plan_of(cs)
        s0 = p["n_slab"] // 2
        assert not M[3].any() and M[16 * s0:16 * (s0 + 1), 0].sum() == (1 if p["n_slab"] == 1 else 0)      # (one slab: the one observation every column keeps)
        assert not M[:16 * (p["n_slab"] - 1), 2].any() and M[16 * (p["n_slab"] - 1):, 2].sum() >= p["last_rows"] - 1
        assert M[:, 3].sum() == cs["d"] - 1
        assert (M[:, 1].sum() == 0) == cs["empty_col"]
        assert all(M[:, t].any() for t in range(cs["T"]) if t != 1)
        if p["trips"] >= 2:
            first = 16 * p["stride"]
            assert not M[:first, 4].any() and M[first:, 4].sum() >= cs["d"] - first - 1 and cs["d"] > first
            seen_two_trip = True
    assert seen_two_trip


def test_shards_and_weighted_inputs():
    sharded = [cs for cs in CASES if cs["shards"]]
    assert {len(cs["shards"]) for cs in sharded if cs["masked"]} == {2, 3, 4} and {len(cs["shards"]) for cs in sharded if not cs["masked"]} == {2, 3, 4}
    assert {cs["method"] for cs in sharded if cs["masked"]} == {"psmf", "rpsmf", "mle_smf", "tmf"}
    for group in (MASKED, WEIGHTED):
        mine = [cs for cs in group if cs["shards"]]
        assert any(min(cs["shards"]) < 16 for cs in mine)
        assert any({GC.plan_of(cs, dl)["trips"] for dl in cs["shards"]} == {1, 2} for cs in mine)       # one shard one-trip, one two-trip
        assert all(len(set(cs["shards"])) > 1 for cs in mine)                                              # uneven
    assert any(cs["r"] > 32 for cs in sharded if cs["masked"]) and any(cs["storage"] == "f32" for cs in sharded)
    assert sum(1 for cs in WEIGHTED if cs["rotated"]) >= len(WEIGHTED) // 6
    wide = [cs for cs in WEIGHTED if cs["wide_rho"]]
    assert len(wide) == 1
    rr = GC.problem(wide[0])["rho_rows"]
    assert rr.max() / rr.min() > 900
    rr = GC.problem(next(cs for cs in WEIGHTED if not cs["wide_rho"]))["rho_rows"]
    assert 0.3 <= rr.min() and rr.max() <= 2.3
    cs = next(cs for cs in WEIGHTED if cs["rotated"])
    U = GC.problem(cs)["U"]
    assert np.allclose(U.T @ U, np.eye(cs["d"]), atol=1e-12)
    # dense starts: V0 and P0 are SPD with off-diagonals
    pb = GC.problem(next(cs for cs in MASKED if cs["method"] == "psmf"))
    for k in ("V0", "P0"):
        assert np.linalg.eigvalsh(pb[k]).min() > 0 and np.abs(pb[k] - np.diag(np.diag(pb[k]))).max() > 1e-3


def test_at_most_a_tenth_of_the_cases_was_shortened_or_replaced():
    print("\nshortened or replaced (case: (salt, times halved)):", GC.RESOLUTION)
    assert len(GC.RESOLUTION) <= GC.N_CASES // 10, len(GC.RESOLUTION)


@pytest.mark.parametrize("i", range(GC.N_CASES))
def test_case_is_admissible_by_the_oracle_alone(i):
    """No LinAlgError, finite, and the oracle's response to a last-bit change of the inputs is at most bar / 16: for the recorded
    resolution of the case, and -- for the cases the table lists -- not for the draw it replaced."""
    (salt, halved), log = GC.resolve(i)
    for line in log:
        print("\nnot admissible:", line)
    assert (salt, halved) == GC.RESOLUTION.get(i, (0, 0)), (i, salt, halved, log)
