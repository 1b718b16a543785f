"""The net of tests/bocpd_net_cases.py is fit to judge the device by: admission and coverage, decided by the references alone.  CPU only.

Admission, per replica of every case (a case that fails is redrawn from its next sub-seed and entered in bocpd_net_cases.REPLACED; at
most 5 % of the list may be replaced):
    (i)   the float64 stable_model is within 1e-11 of extended_model (np.longdouble, mpmath's lgamma) on every live log p -- a tenth of
          the device's bar, the margin tests/test_bocpd_cases_cpu.py keeps between the two float64 models -- and NaN in the same places
    (ii)  every column of the extended R has its maximum clear of the runner-up by 1e-6 relative or more
    (iii) map_run and the change points are equal between the two
Coverage, on the admitted list: the walked dims and time lengths; 0, 1, 2 and >= 3 declared change points; more than max_changepoints
stores; a truncation whose discarded births lie on both sides of a chain-block edge; a truncation at T > 256 from more than 256 live
hypotheses to fewer than 64; a change point under confirm = 0 and one under drop = 0; zeros of drop, settle and confirm.
Wrong models (bocpd_cases.WRONG): every one moves a case of the net by 100 x the device's bar on log p (a log p where NaN is due, or the
reverse, counts as infinitely far) or changes its map_run."""

import numpy as np
import pytest

import bocpd_cases as BC
import bocpd_net_cases as NC

LP_BAR = 1e-10      # tests/test_hip_bocpd_net.py

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: extended_model is no reference without it"


def _replicas():
    for cs in NC.CASES:
        for b in range(cs["batch"]):
            yield cs, b, NC.reference(cs["no"], b)[1]


@pytest.mark.parametrize("cs", NC.CASES, ids=NC.IDS)
def test_admission(cs):
    worst, gap = 0.0, np.inf
    for b in range(cs["batch"]):
        X, ex = NC.reference(cs["no"], b)
        st = NC.stable_reference(cs["no"], b)
        assert ex["logpred"].dtype == np.longdouble and ex["R"].dtype == np.longdouble
        live = ~np.isnan(ex["logpred"])
        assert np.array_equal(live, ~np.isnan(st["logpred"]))
        assert live[np.tril_indices(cs["T"])].any() and not live[np.triu_indices(cs["T"], 1)].any()
        worst = max(worst, float(np.max(np.abs(st["logpred"][live] - ex["logpred"][live]))))
        gap = min(gap, NC.column_gap(ex["R"]))
        assert np.array_equal(st["map_run"], ex["map_run"]) and st["changepoints"] == ex["changepoints"], (cs["name"], b)
        assert np.allclose(np.asarray(ex["R"][1:].sum(axis=1), dtype=float), 1.0, atol=1e-12)
        assert np.isfinite(X).all() and X.shape == (cs["dim"], cs["T"])
    print(f"\n{cs['name']}: float64 model within {worst:.2e} of the extended one on log p; least column gap {gap:.2e}")
    assert worst <= 1e-11, (cs["name"], worst)
    assert gap >= 1e-6, (cs["name"], gap)


def test_at_most_one_case_in_twenty_is_replaced():
    print(f"\n{len(NC.CASES)} cases, {sum(c['batch'] for c in NC.CASES)} series; replaced {sorted(NC.REPLACED)}")
    assert len(NC.REPLACED) <= 0.05 * len(NC.CASES)
    assert all(NC.CASES[no]["sub"] == sub and sub > 0 for no, sub in NC.REPLACED.items())
    assert all(cs["sub"] == 0 for cs in NC.CASES if cs["no"] not in NC.REPLACED)


def test_the_walked_sets():
    seen = {(cs["dim"], cs["T"]) for cs in NC.CASES}
    assert {d for d, _ in seen} == set(range(1, 33))
    assert [NC.lanes(d) for d in (1, 12, 13, 17, 18, 24, 25, 32)] == [256, 256, 128, 128, 64, 64, 32, 32]
    for dim in NC.BOUNDARY_DIMS:
        nl = NC.lanes(dim)
        assert {(dim, nl - 1), (dim, nl), (dim, nl + 1), (dim, 2 * nl + 1)} <= seen, dim
    assert {NC.lanes(d) for d in NC.BOUNDARY_DIMS} == {256, 128, 64, 32}
    for dim in range(1, 33):
        assert any(d == dim and T > NC.lanes(dim) for d, T in seen), dim
    for T in (63, 64, 65, 255, 256, 257):
        assert any(d <= 12 and t == T for d, t in seen), T
    assert max(T for _, T in seen) <= 2 * 256 + 1


def test_the_drawn_ranges():
    C = NC.CASES
    assert {cs["batch"] for cs in C} == {1, 2, 3, 4, 5}
    assert all(1.5 <= cs["lam"] <= 1000 and 0.05 <= cs["kappa0"] <= 20 and 0.05 <= cs["nu0"] - (cs["dim"] - 1) <= 10 for cs in C)
    assert all(0.25 <= cs["sigma0"] / cs["scale"] ** 2 <= 4 for cs in C) and {cs["scale"] for cs in C} == set(NC.SCALES)
    assert min(cs["lam"] for cs in C) < 3 and max(cs["lam"] for cs in C) > 500
    assert min(cs["nu0"] - (cs["dim"] - 1) for cs in C) < 0.2 and min(cs["kappa0"] for cs in C) < 0.1
    for k in ("drop", "settle", "confirm"):
        assert {cs[k] for cs in C} >= {0, 12} and all(0 <= cs[k] <= 12 for cs in C), k
    assert {cs["max_changepoints"] for cs in C} == {0, 1, 16} and {cs["kind"] for cs in C} == set(NC.KINDS)
    assert all(abs(cs["base"]) >= 1.5 for cs in C)      # the means lie away from the prior's 0
    differ = [cs for cs in C if cs["batch"] > 1 and not np.array_equal(NC.series(cs, 0), NC.series(cs, 1))]
    assert len(differ) == sum(cs["batch"] > 1 for cs in C)


def test_the_heuristic_is_covered():
    counts, over, straddle, late, confirm0, drop0, settle0 = set(), [], [], [], [], [], []
    for cs, b, ex in _replicas():
        n = len(ex["changepoints"])
        counts.add(min(n, 3))
        nl = NC.lanes(cs["dim"])
        if n > cs["max_changepoints"]:
            over.append(cs["no"])
        if n and cs["confirm"] == 0:
            confirm0.append(cs["no"])
        if n and cs["drop"] == 0:
            drop0.append(cs["no"])
        if cs["settle"] == 0:
            assert n == 0, "settle = 0 can never confirm"
            settle0.append(cs["no"])
        for (t, lo, hi), gone in zip(NC.truncations(ex), ex["discarded"]):
            assert hi - lo == gone
            if any(lo < k * nl <= hi - 1 for k in range(1, cs["T"] // nl + 1)):
                straddle.append((cs["no"], nl))
            if cs["T"] > 256 and t + 1 - lo > 256 and ex["map_run"][t] < 64:      # live at the step: births lo .. t; after it: m_t
                late.append(cs["no"])
    print(f"\nmore than max_changepoints: cases {sorted(set(over))}\na truncation across a chain-block edge: (case, NL) {sorted(set(straddle))}\n"
          f"> 256 live -> < 64: {sorted(set(late))}; a change point under confirm = 0: {sorted(set(confirm0))}; under drop = 0: {sorted(set(drop0))}; "
          f"settle = 0: {sorted(set(settle0))}")
    assert counts == {0, 1, 2, 3}
    assert over and late and confirm0 and drop0 and settle0
    assert {nl for _, nl in straddle} == {256, 128, 64, 32}, "a truncation straddles a block edge at every lane count"


def _distance(a, b):
    la, lb = ~np.isnan(a["logpred"]), ~np.isnan(b["logpred"])
    if not np.array_equal(la, lb):
        return np.inf
    return float(np.max(np.abs(a["logpred"][la] - b["logpred"][la])))


# the cases a wrong model is tried on: dim 1 / T 64 with one change point, dim 25 / T 65 (three blocks of 32 births), dim 25 / T 32 with
# two change points, dim 32 / T 65 with two
TRIED = (84, 23, 21, 88)


@pytest.mark.parametrize("wrong", BC.WRONG)
def test_a_wrong_model_moves_the_net(wrong):
    moved = []
    for no in TRIED:
        cs = NC.CASES[no]
        X, ex = NC.reference(no, 0)
        bad = BC.extended_model(X, wrong=wrong, nl=NC.lanes(cs["dim"]), **NC.params(cs))
        d, m = _distance(bad, ex), not np.array_equal(bad["map_run"], ex["map_run"])
        print(f"\n{wrong} on {cs['name']}: log p moves by {d:.3g}, map_run {'changes' if m else 'stays'}")
        if d >= 100 * LP_BAR or m:
            moved.append(no)
    assert moved, wrong


def test_the_right_model_does_not_move_it():
    for no in TRIED:
        cs = NC.CASES[no]
        X, ex = NC.reference(no, 0)
        again = BC.extended_model(X, wrong=None, nl=NC.lanes(cs["dim"]), **NC.params(cs))
        assert _distance(again, ex) == 0.0 and np.array_equal(again["map_run"], ex["map_run"])
