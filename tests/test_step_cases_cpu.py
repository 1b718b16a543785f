"""tests/step_cases.py without a GPU: (1) the restated planner is the table of that module's docstring; (2) the seeded case list
of the per-step engine's random-configuration net covers what it claims to cover on a device of 256 compute units -- every one of
the 44 instances of psmf_pstep_k twice, every reason for the launched form, every geometry edge, NP threshold and fan-in window,
every mode on the persistent kernel and on an NP > 4 instance of it -- so that the net cannot go thin unnoticed; (3) every case is
well enough conditioned for its tolerance to mean something: the float64 oracle runs it to finite values, and its answer moves by
at most 1/16 of the case's bar when C0, Y and theta move by a relative 2^-50 (float32 storage: 2^-23, after the rounding to
float32).  A case that is not admissible is halved (at most twice), then redrawn; step_cases.RESOLUTION records the outcome and
this file recomputes it.
Wall time: about four minutes on one core (the big-d cases run the oracle over up to 4.2e6 series entries, twice).
Reference: pypsmf/psmf/psmf.py:85-180, rpsmf.py:116-184; ExperimentImpute/PSMF.py:40-95 (through oracle/)."""

from collections import Counter

import pytest

import step_cases as SC

CASES = [SC.device_case(i) for i in range(SC.N_CASES)]
PERSISTENT = [cs for cs in CASES if SC.expected_kernel(cs) == "psmf_pstep_k"]
BIG_NP = [cs for cs in PERSISTENT if SC.instance_of(cs)[1] > 4]


def test_the_planner_is_the_table_of_the_docstring():
    table = {8: (261_120, 522_240, 783_360), 16: (130_560, 261_120, 391_680), 32: (65_280, 130_560, 195_840)}
    big = {41: (30_720, 61_440, 92_160, 122_880), 45: (28_160, 56_320, 84_480, 112_640), 48: (25_600, 51_200, 76_800, 102_400)}
    for r in range(1, 49):
        rpad = SC.rpad_of(r)
        row = table[rpad] if rpad < 64 else big[min(k for k in big if r <= k)]
        assert tuple(SC.d_max(r, n) for n in SC.np_list(rpad)) == row, r
        lo = 0
        for n, hi in zip(SC.np_list(rpad), row):
            # no window: every d of (lo, hi] has a geometry, on the smallest NP that takes it, its workgroups within both counts
            for d in sorted({lo + 1, lo + 2, (lo + hi) // 2, hi - 1, hi} | set(range(lo + 1, hi + 1, 997))):
                p = SC.plan(d, r)
                assert p is not None and p["np"] == n and p["rows_per_wg"] == n * p["rpw"], (r, d, p)
                assert p["n_row_wg"] == -(-d // p["rows_per_wg"]) <= min(255, p["fan_in"]), (r, d, p)
            lo = hi
        assert SC.plan(row[-1] + 1, r) is None and SC.plan(0, r) is None
        assert (SC.plan(1000, r, masked=True) is None) == (r > 32)
    assert SC.plan(1000, 49) is None and SC.plan(1000, 8, n_cu=1) is None
    assert [SC.fan_in(r) for r in (1, 31, 32, 33, 41, 42, 45, 46, 48)] == [408, 272, 255, 240, 240, 220, 220, 200, 200]
    # the headline shape and the one tests/test_hip_big_rank.py names
    assert (SC.plan(100_000, 32)["np"], SC.plan(100_000, 32)["n_row_wg"]) == (8, 196)
    assert (SC.plan(100_000, 48)["np"], SC.plan(100_000, 48)["n_row_wg"]) == (16, 196)
    # a device with fewer compute units: the same shapes on more passes, or not at all
    assert SC.plan(65_280, 32, n_cu=128)["np"] == 12 and SC.plan(100_000, 32, n_cu=128) is None


def test_the_case_list_is_what_the_table_says():
    assert len(SC.INSTANCES) == 44 == len(set(SC.INSTANCES)) and SC.N_CASES == len(SC.TARGETS)
    for i, cs in enumerate(CASES):
        t = SC.TARGETS[i]
        assert SC.target_of(cs) == (t if isinstance(t, tuple) else dict(SC.LAUNCHED)[t]), (i, t, SC.target_of(cs))
        assert cs["parts"][0][0] == 0 and cs["parts"][-1][1] == cs["T"] and all(a <= b for a, b in cs["parts"])
        assert all(p[1] == q[0] for p, q in zip(cs["parts"][:-1], cs["parts"][1:])), cs["parts"]
        assert 1 <= sum(1 for a, b in cs["parts"] if b > a) <= 3
        assert cs["r"] in SC.R_LIST and cs["d"] >= 1 and cs["T"] * cs["d"] <= SC.MAX_SERIES
        assert (3 <= cs["T"] <= 8) if cs["d"] > SC.BIG_D else (2 <= cs["T"] <= 36)
        assert not (cs["sched"] and cs["robust"]) and not (cs["recursive"] and cs["dyn"] != "cos_phase")
        if cs["masked"]:
            assert cs["dyn"] == "random_walk" and cs["hooks"] == "full" and not cs["sched"] and cs["d"] >= 8 and cs["T"] >= 3


def test_every_instance_and_every_launched_form():
    inst = Counter(SC.instance_of(cs) for cs in PERSISTENT)
    print("\ncases per instance:", dict(inst))
    assert set(inst) == set(SC.INSTANCES) and min(inst.values()) >= 2, inst
    launched = Counter(cs["target"] for cs in CASES if SC.expected_kernel(cs) == "psmf_sweep_solve")
    print("cases per launched form:", dict(launched))
    assert set(launched) == {name for name, _ in SC.LAUNCHED}, launched
    by = {cs["target"]: cs for cs in CASES if not isinstance(cs["target"], tuple)}
    assert {cs["r"] for cs in CASES if cs["target"] == "rank_49_to_64"} == set(SC.LAUNCHED_RANKS) and by["nonuniform_R"]["nonuniform"] and by["dense_jacobian_kind"]["dyn"] in ("scaled_walk", "scaled_walk_bias")
    assert by["masked_rank_above_32"]["masked"] and by["masked_rank_above_32"]["r"] > 32
    assert by["persistent_switch_off"]["env"] == {"PSMF_STEP_PERSISTENT": "0"} and by["persistent_switch_off"]["r"] <= 48
    assert by["big_switch_off_rank_33_to_48"]["env"] == {"PSMF_PSTEP_BIG": "0"} and 33 <= by["big_switch_off_rank_33_to_48"]["r"] <= 48
    assert any(cs["target"] == "rows_beyond_the_plan" and cs["r"] == 31 and cs["d"] == 195_841 for cs in CASES)
    # every rank of the list; both storage types with every residue of d mod 4
    assert {cs["r"] for cs in CASES} == set(SC.R_LIST)
    for storage in ("f32", "f64"):
        assert {cs["d"] % 4 for cs in PERSISTENT if cs["storage"] == storage} == {0, 1, 2, 3}, storage


def test_every_geometry_edge_threshold_and_window():
    have = {(cs["r"], cs["d"]) for cs in CASES}
    assert set(SC.EDGES) <= have, set(SC.EDGES) - have
    rows = {}
    for cs in PERSISTENT:
        rows.setdefault(SC.rpad_of(cs["r"]), set()).add((cs["r"], cs["d"]))
    for rpad in (8, 16, 32, 64):
        rpw, ds = SC.rows_per_pass(rpad), {d for _, d in rows[rpad]}
        assert {1, 2, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1} <= ds, (rpad, sorted(ds)[:20])
        assert any({(r, r - 1), (r, r), (r, r + 1)} <= rows[rpad] and r % 4 for r in SC.RANKS[rpad]), rpad
        assert any(r % 4 for r, _ in rows[rpad])
        # the last shape of every variant (the widest fan-in of the padded rank: r0) and the first shape of the next: its last
        # workgroup ends in a pass of one row; behind the last variant the launched form
        r0 = {8: 7, 16: 16, 32: 32, 64: 40}[rpad]
        for n in SC.np_list(rpad):
            top = SC.d_max(r0, n)
            assert any(cs["d"] == top and SC.instance_of(cs)[:2] == (rpad, n) for cs in PERSISTENT), (rpad, n)
            nxt = [cs for cs in CASES if cs["d"] == top + 1 and SC.rpad_of(cs["r"]) == rpad and SC.d_max(cs["r"], n) == top and not cs["env"]]
            assert nxt, (rpad, n)
            for cs in nxt:
                p = SC.plan(cs["d"], cs["r"])
                if n == SC.np_list(rpad)[-1]:
                    assert p is None and SC.expected_kernel(cs) == "psmf_sweep_solve"
                else:
                    assert p["np"] > n and (cs["d"] - (p["n_row_wg"] - 1) * p["rows_per_wg"]) % p["rpw"] == 1, (cs["d"], p)
    # a last workgroup that holds a single row: the second of two, and the last of many
    for n in (4, 12):
        assert any(cs["d"] % SC.plan(cs["d"], cs["r"])["rows_per_wg"] == 1 and SC.instance_of(cs)[1] == n and cs["d"] > 1 for cs in PERSISTENT), n
    # the fan-in exactly full
    full = {(cs["r"], SC.plan(cs["d"], cs["r"])["n_row_wg"]) for cs in PERSISTENT}
    assert (32, 255) in full and (40, 240) in full, sorted(full)[-10:]
    # the windows of d the planner refused before it tried the next variant: two fan-in classes, persistent now
    for r in (37, 48):
        assert SC.fan_in(37) != SC.fan_in(48)
        for lo, hi, n in ((30_721, 32_640, 8), (61_441, 65_280, 12), (92_161, 97_920, 16)):
            hit = [cs for cs in PERSISTENT if cs["r"] == r and lo <= cs["d"] <= hi]
            assert hit and all(SC.instance_of(cs)[1] == n for cs in hit), (r, lo, hi)


def _modes(cases):
    return dict(hooks={cs["hooks"] for cs in cases}, optimisers={cs["recursive"] for cs in cases if cs["recursive"]},
                update_every={cs["update_every"] for cs in cases if cs["recursive"]}, sched=any(cs["sched"] for cs in cases),
                general_Q=any(cs["general_Q"] for cs in cases), cos_phase=any(cs["dyn"] == "cos_phase" for cs in cases))


def test_every_mode_on_the_persistent_kernel_and_beyond_four_row_passes():
    for name, cases in (("persistent", PERSISTENT), ("NP > 4", BIG_NP)):
        m = _modes(cases)
        print(f"\n{name}: {len(cases)} cases, {m}")
        assert m["hooks"] == set(SC.HOOKS) and m["optimisers"] == {1, 2} and m["sched"] and m["general_Q"] and m["cos_phase"], (name, m)
    assert _modes(PERSISTENT)["update_every"] == {1, 3, 7}
    # each mode at 33 <= r <= 48 too (the hub with LDS-resident matrices)
    m = _modes([cs for cs in PERSISTENT if cs["r"] > 32])
    assert m["hooks"] == set(SC.HOOKS) and m["optimisers"] == {1, 2} and m["sched"] and m["general_Q"], m
    assert any(cs["robust"] and cs["fixed_lambda"] for cs in PERSISTENT) and any(cs["robust"] and cs["alpha"] != 1.0 for cs in PERSISTENT)
    assert any(cs["robust"] for cs in BIG_NP) and any(not cs["robust"] for cs in BIG_NP)
    for robust in (False, True):
        assert any(cs["masked"] and cs["robust"] == robust and SC.instance_of(cs)[1] > 4 for cs in PERSISTENT), robust
    # masked at 17 <= r <= 32 beyond 65 280 rows: the reduce-scatter of the Gram over more than 128 workgroups
    assert any(cs["masked"] and cs["r"] > 16 and SC.plan(cs["d"], cs["r"])["n_row_wg"] > 128 and SC.instance_of(cs)[1] > 4 for cs in PERSISTENT)
    # the marked columns of the mask fall on whole workgroups
    for cs in PERSISTENT:
        if cs["masked"] and SC.plan(cs["d"], cs["r"])["n_row_wg"] >= 2:
            p, M = SC.plan(cs["d"], cs["r"]), SC.problem(cs)["M"]
            R, w = p["rows_per_wg"], p["n_row_wg"] // 2
            assert not M[3].any() and not M[:, 1].any() and not M[w * R:(w + 1) * R, 0].any() and M[:, 0].any()
            last = (p["n_row_wg"] - 1) * R
            assert not M[:last, 2].any() and M[last:, 2].all() and last < cs["d"]
            break
    else:
        raise AssertionError("no masked case with two workgroups")


def test_cuts_at_one_and_at_the_last_step_and_empty_parts():
    cuts = Counter()
    for cs in PERSISTENT:
        for _, b in cs["parts"][:-1]:
            cuts["1"] += b == 1
            cuts["T-1"] += b == cs["T"] - 1
    print("\ncuts:", dict(cuts))
    assert cuts["1"] >= 10 and cuts["T-1"] >= 10, cuts
    assert sum(1 for cs in PERSISTENT if any(a == b for a, b in cs["parts"])) >= 5
    assert {sum(1 for a, b in cs["parts"] if b > a) for cs in PERSISTENT} == {1, 2, 3}
    small = [cs for cs in PERSISTENT if cs["d"] <= SC.BIG_D and not cs["masked"]]
    assert sum(1 for cs in small if cs["second_pass"]) >= len(small) // 6 and not any(cs["second_pass"] for cs in CASES if cs["d"] > SC.BIG_D)
    for n in (4, 8, 12, 16):
        assert any(len(cs["parts"]) > 1 for cs in PERSISTENT if SC.instance_of(cs)[1] == n), n


def test_at_most_a_tenth_of_the_cases_was_shortened_or_replaced():
    print("\nshortened or replaced (case: (salt, times halved)):", SC.RESOLUTION)
    assert len(SC.RESOLUTION) <= SC.N_CASES // 10, len(SC.RESOLUTION)


@pytest.mark.parametrize("i", range(SC.N_CASES))
def test_case_is_admissible_by_the_oracle_alone(i):
    """No LinAlgError, finite, and the oracle's response to a last-bit change of the inputs is at most bar / 16: for the recorded
    resolution of the case, and -- for the cases the table lists -- not for the draw it replaced."""
    (salt, halved), log = SC.resolve(i)
    for line in log:
        print("\nnot admissible:", line)
    assert (salt, halved) == SC.RESOLUTION.get(i, (0, 0)), (i, salt, halved, log)
