"""psmf_bocpd_run / rpsmf_amd.changepoint on the device: the batched Bayesian online change-point detection
(rpsmf_amd/csrc/psmf_bocpd.hip) against the Cholesky-factor, log-domain model of tests/bocpd_cases.py (stable_model).

Bars: log p within 1e-10 absolute where live -- 100 x the spread measured between the two float64 formulations on the CPU, 10 x what
tests/test_bocpd_cases_cpu.py admits -- and NaN exactly where not live; R and R_last within 5e-9 in conftest.relerr, the suite's
float64 bar for the one-workgroup engines; map_run, changepoints and n_changepoints exactly (every column of R has a maximum that is
clear by 1e-6 relative or more).  Every case runs once per module, with R and log p returned; the other tests share those runs."""

from functools import lru_cache

import numpy as np
import pytest

import bocpd_cases as BC
from conftest import relerr

pytestmark = pytest.mark.gpu

LP_BAR = 1e-10
R_BAR = 5e-9
ERR_NUMERIC = -4


def _run(X, cs, **kw):
    from rpsmf_amd.changepoint import mvbocpd_batch

    return mvbocpd_batch(X, **{**BC.params(cs), **kw})


@lru_cache(maxsize=None)
def _device(name):
    cs = BC.find(name)
    return _run(BC.batch(cs), cs, want_R=True, want_logpred=True)


def _compare(res, b, ref):
    """worst errors of replica b; asserts the exact quantities"""
    live = ~np.isnan(ref["logpred"])
    assert np.array_equal(~np.isnan(res["logpred"][b]), live), "log p is NaN exactly where the age is not live"
    assert np.array_equal(res["map_run"][b], ref["map_run"])
    assert list(res["changepoints"][b]) == ref["changepoints"] and res["n_changepoints"][b] == len(ref["changepoints"])
    return dict(logpred=float(np.max(np.abs(res["logpred"][b][live] - ref["logpred"][live]))), R=relerr(res["R"][b], ref["R"]),
                R_last=relerr(res["R_last"][b], ref["R_last"]))


@pytest.mark.parametrize("name", [n for n in BC.IDS if n != "many"])
def test_every_case_against_the_stable_model(name):
    res = _device(name)
    cs = BC.find(name)
    assert list(res["status"]) == [0, 0, 0] and res["R"].shape == (3, cs["T"] + 1, cs["T"] + 1)
    worst = {}
    for b in range(3):
        err = _compare(res, b, BC.reference(name, b)[1])
        worst = {k: max(worst.get(k, 0.0), v) for k, v in err.items()}
    print(f"\nbocpd {name}: worst over the replicas {worst}; change points {[list(c) for c in res['changepoints']]}; {res['elapsed_ms']:.3f} ms")
    assert np.isfinite(res["R"]).all() and np.isfinite(res["R_last"]).all()
    assert worst["logpred"] <= LP_BAR and worst["R"] <= R_BAR and worst["R_last"] <= R_BAR, worst


def test_more_workgroups_than_compute_units():
    cs = BC.find("many")
    res = _device("many")
    assert res["status"].shape == (300,) and not res["status"].any()
    for b in (0, 150, 299):
        err = _compare(res, b, BC.stable_model(BC.series(cs, b), **BC.params(cs)))
        print(f"\nbocpd batch of 300, replica {b}: {err}")
        assert err["logpred"] <= LP_BAR and err["R"] <= R_BAR and err["R_last"] <= R_BAR, (b, err)


KEYS = ("map_run", "n_changepoints", "R_last", "R", "logpred")


@pytest.mark.parametrize("name", ["dim3-two", "dim20-shift", "dim32-shift", "dim2-long"])
def test_a_replica_run_alone_and_a_second_run_give_the_same_bits(name):
    cs = BC.find(name)
    res = _device(name)
    alone = _run(BC.series(cs, 1), cs, want_R=True, want_logpred=True)
    assert alone["status"][0] == 0
    assert all(np.array_equal(alone[k][0], res[k][1], equal_nan=True) for k in KEYS), "replica 1 alone differs from replica 1 of the batch"
    again = _run(BC.batch(cs), cs, want_R=True, want_logpred=True)
    assert all(np.array_equal(again[k], res[k], equal_nan=True) for k in KEYS), "the same call twice gives different bits"
    plain = _run(BC.batch(cs), cs)
    assert plain["R"] is None and plain["logpred"] is None
    assert all(np.array_equal(plain[k], res[k]) for k in KEYS[:3]), "the outputs depend on want_R / want_logpred"


def test_a_nan_sample_fails_its_replica_alone():
    cs = BC.find("dim3-shift")
    X = BC.batch(cs)
    X[1, 2, 17] = np.nan
    res = _run(X, cs, want_R=True, want_logpred=True)
    assert list(res["status"]) == [0, ERR_NUMERIC, 0]
    good = _device("dim3-shift")
    for b in (0, 2):
        assert all(np.array_equal(res[k][b], good[k][b], equal_nan=True) for k in KEYS)
        assert list(res["changepoints"][b]) == list(good["changepoints"][b])
    with pytest.raises(np.linalg.LinAlgError, match="replica 1"):
        _run(X, cs, status=None)
    X[1, 2, 17] = np.inf
    assert list(_run(X, cs)["status"]) == [0, ERR_NUMERIC, 0]


def test_the_outlier_step_stays_finite_and_equals_the_stable_model():
    res = _device("dim3-outlier")
    for b in range(3):
        ref = BC.reference("dim3-outlier", b)[1]
        assert np.all(np.exp(res["logpred"][b][-1][~np.isnan(ref["logpred"][-1])]) == 0.0)      # every p_a of the step underflows
        assert np.isfinite(res["R_last"][b]).all() and abs(res["R_last"][b].sum() - 1.0) < 1e-12
        assert relerr(res["R_last"][b], ref["R_last"]) <= R_BAR
        assert np.isnan(BC.literal_reference("dim3-outlier", b)["R_last"]).any()


def test_max_changepoints_caps_what_is_stored_not_what_is_counted():
    cs = BC.find("dim3-two")
    seed = next(s for s in range(3) if len(BC.reference("dim3-two", s)[1]["changepoints"]) == 2)
    ref = BC.reference("dim3-two", seed)[1]
    res = _run(BC.series(cs, seed), cs, max_changepoints=1)
    assert list(res["changepoints"][0]) == ref["changepoints"][:1] and res["n_changepoints"][0] == 2
    none = _run(BC.series(cs, seed), cs, max_changepoints=0)
    assert list(none["changepoints"][0]) == [] and none["n_changepoints"][0] == 2


def experiment_series():
    """one series of the experiment's shape, 20 x 1200: N(2, 1) channels that move to N(-2, 1) at sample 600"""
    Y = np.random.default_rng(4242).standard_normal((20, 1200)) + 2.0
    Y[:, 599:] -= 4.0
    return Y


def test_the_drop_in_on_an_experiment_shaped_series():
    from rpsmf_amd.changepoint import MVBOCPD, mvbocpd_batch

    Y = experiment_series()
    ref = BC.stable_model(Y[:, 399:])
    assert BC.column_gap(ref["R"]) >= 1e-6
    cp = 400 + np.array(ref["changepoints"], dtype=int)
    want = int(np.any((cp > 570) & (cp < 630)))
    res = mvbocpd_batch(Y[:, 399:], max_changepoints=64)
    print(f"\nbocpd drop-in, T = 801, dim = 20: change points {list(res['changepoints'][0])} (model {ref['changepoints']}), "
          f"R_last {relerr(res['R_last'][0], ref['R_last']):.2e}, {res['elapsed_ms']:.3f} ms")
    assert res["map_run"].shape == (1, 801) and np.array_equal(res["map_run"][0], ref["map_run"])
    assert list(res["changepoints"][0]) == ref["changepoints"]
    assert relerr(res["R_last"][0], ref["R_last"]) <= R_BAR
    assert MVBOCPD(Y) == want
    assert want == 1 and MVBOCPD(Y, window=(100, 200)) == 0


@pytest.mark.parametrize("shape, kw, msg", [
    ((1, 33, 8), {}, "dim <= 32"),
    ((1, 2, 4097), {}, "T <= 4096"),
    ((0, 2, 8), {}, "batch >= 1"),
    ((1, 2, 8), dict(lam=1.0), "lambda > 1"),
    ((1, 2, 8), dict(lam=float("nan")), "lambda > 1"),
    ((1, 2, 8), dict(kappa0=0.0), "kappa0 > 0"),
    ((1, 2, 8), dict(nu0=1.0), "nu0 > dim - 1"),
    ((1, 2, 8), dict(sigma0=0.0), "sigma0 > 0"),
    ((64, 2, 4096), dict(want_R=True), "want_R.*2\\^28 doubles"),
    ((128, 2, 2048), dict(want_logpred=True), "want_logpred.*2\\^28 doubles"),
])
def test_refusals_by_message(shape, kw, msg):
    from rpsmf_amd.changepoint import mvbocpd_batch

    with pytest.raises(ValueError, match=msg):
        mvbocpd_batch(np.zeros(shape), **kw)
