"""The cases of tests/bocpd_cases.py are fit to judge the device by: admission conditions on the list itself, met by the two float64
models alone.  CPU only.
    (i)   literal_model (inv, det, linear R) and stable_model (Cholesky factors, log R) agree on log p to 1e-11 absolute on every case:
          the device's bar of 1e-10 (tests/test_hip_bocpd.py) is ten times what separates two float64 formulations at most
    (ii)  the largest entry of every column of R exceeds the runner-up by 1e-6 relative or more: the MAP run length, and everything the
          heuristic derives from it, is then decided far above rounding, and device and model must agree on it exactly
    (iii) the list declares 0, 1 and 2 change points, and a truncation that discards 5 hypotheses or more
    (iv)  in the outlier case the literal model's last column is NaN and the stable model's is finite
    (v)   moving one sample changes map_run: the cases can fail"""

import numpy as np
import pytest

import bocpd_cases as BC

SMALL = [c for c in BC.CASES if c.get("batch", 3) == 3]
SEEDS = (0, 1, 2)


@pytest.mark.parametrize("cs", SMALL, ids=[c["name"] for c in SMALL])
def test_the_two_models_agree_and_every_column_has_a_clear_maximum(cs):
    worst, gap = 0.0, np.inf
    for seed in SEEDS:
        st, lit = BC.reference(cs["name"], seed)[1], BC.literal_reference(cs["name"], seed)
        live = ~np.isnan(st["logpred"])
        assert np.array_equal(live, ~np.isnan(lit["logpred"]))
        assert live[np.tril_indices(cs["T"])].any() and not live[np.triu_indices(cs["T"], 1)].any()
        worst = max(worst, float(np.max(np.abs(st["logpred"][live] - lit["logpred"][live]))))
        gap = min(gap, BC.column_gap(st["R"]))
        assert np.array_equal(st["map_run"], lit["map_run"]) and st["changepoints"] == lit["changepoints"]
        if cs["kind"] != "outlier":
            assert np.max(np.abs(st["R"] - lit["R"])) <= 1e-11
        assert np.allclose(st["R"][1:].sum(axis=1), 1.0, atol=1e-12)
    print(f"\nbocpd {cs['name']}: models differ by {worst:.2e} on log p; least column gap {gap:.2e}")
    assert worst <= 1e-11
    assert gap >= 1e-6


def test_the_many_case_meets_the_same_conditions_on_a_sample_of_its_replicas():
    cs = BC.find("many")
    for seed in (0, 150, 299):
        X = BC.series(cs, seed)
        st, lit = BC.stable_model(X, **BC.params(cs)), BC.literal_model(X, **BC.params(cs))
        live = ~np.isnan(st["logpred"])
        assert np.max(np.abs(st["logpred"][live] - lit["logpred"][live])) <= 1e-11
        assert BC.column_gap(st["R"]) >= 1e-6


def test_the_list_covers_zero_one_and_two_change_points_and_a_real_truncation():
    counts, discarded = set(), []
    for cs in SMALL:
        for seed in SEEDS:
            st = BC.reference(cs["name"], seed)[1]
            counts.add(len(st["changepoints"]))
            discarded += st["discarded"]
    assert {0, 1, 2} <= counts, counts
    assert max(discarded) >= 5
    two = [len(BC.reference("dim3-two", s)[1]["changepoints"]) for s in SEEDS]
    assert 2 in two
    assert max(BC.reference("dim2-long", 0)[1]["map_run"]) > 64      # more live hypotheses than a wave has lanes


def test_the_non_default_constants_matter():
    cs = BC.find("dim3-consts")
    for seed in SEEDS:
        X = BC.series(cs, seed)
        assert len(BC.stable_model(X, **BC.params(cs))["changepoints"]) == 1
        assert BC.stable_model(X, **{**BC.params(cs), "drop": 10, "settle": 10, "confirm": 10})["changepoints"] == []


def test_the_outlier_step_underflows_every_predictive():
    cs = BC.find("dim3-outlier")
    for seed in SEEDS:
        st, lit = BC.reference(cs["name"], seed)[1], BC.literal_reference(cs["name"], seed)
        last = st["logpred"][-1]
        assert np.all(np.exp(last[~np.isnan(last)]) == 0.0)
        assert np.isnan(lit["R_last"][st["R_last"] > 0]).all() and (st["R_last"] > 0).sum() >= 2
        assert np.isfinite(st["R_last"]).all() and abs(st["R_last"].sum() - 1.0) < 1e-12


def test_moving_a_sample_changes_the_map_run():
    cs = BC.find("dim3-shift")
    X = BC.series(cs, 0).copy()
    at = cs["at"][0]
    X[:, [at - 8, at + 2]] = X[:, [at + 2, at - 8]]      # a sample of the second regime moves into the first
    assert not np.array_equal(BC.stable_model(X, **BC.params(cs))["map_run"], BC.reference(cs["name"], 0)[1]["map_run"])
