"""psmf_bocpd_run on the seeded net of tests/bocpd_net_cases.py: every chain-kernel instance (dim 1 .. 32), both sides of every change of
its lanes per workgroup, time lengths around one and two blocks of births and around the post kernel's wave and workgroup, drawn
priors, hazards, data scales and heuristic constants -- against the extended-precision model (np.longdouble, mpmath's lgamma), which
tests/test_bocpd_net_cases_cpu.py admits.

Bars, those of tests/test_hip_bocpd.py: log p within 1e-10 absolute where live and NaN exactly where not; R and R_last within 5e-9 in
conftest.relerr; map_run, changepoints (the first max_changepoints of them) and n_changepoints exactly; status 0 everywhere."""

from functools import lru_cache

import numpy as np
import pytest

import bocpd_net_cases as NC
from conftest import relerr

pytestmark = pytest.mark.gpu

LP_BAR = 1e-10
R_BAR = 5e-9

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: extended_model is no reference without it"


@lru_cache(maxsize=None)
def _errors(no):
    """worst errors over the replicas of case `no`, one device call; asserts the exact quantities"""
    from rpsmf_amd.changepoint import mvbocpd_batch

    cs = NC.CASES[no]
    T = cs["T"]
    res = mvbocpd_batch(NC.batch(cs), **NC.params(cs), max_changepoints=cs["max_changepoints"], want_R=True, want_logpred=True)
    assert res["status"].shape == (cs["batch"],) and not res["status"].any()
    assert res["R"].shape == (cs["batch"], T + 1, T + 1) and res["logpred"].shape == (cs["batch"], T, T)
    assert np.isfinite(res["R"]).all() and np.isfinite(res["R_last"]).all()
    worst = dict(logpred=0.0, R=0.0, R_last=0.0)
    for b in range(cs["batch"]):
        ref = NC.reference(no, b)[1]
        live = ~np.isnan(ref["logpred"])
        assert np.array_equal(~np.isnan(res["logpred"][b]), live), (cs["name"], b, "log p is NaN exactly where the age is not live")
        assert np.array_equal(res["map_run"][b], ref["map_run"]), (cs["name"], b)
        assert list(res["changepoints"][b]) == ref["changepoints"][:cs["max_changepoints"]], (cs["name"], b)
        assert res["n_changepoints"][b] == len(ref["changepoints"]), (cs["name"], b)
        err = dict(logpred=float(np.max(np.abs(res["logpred"][b][live] - ref["logpred"][live]))), R=relerr(res["R"][b], ref["R"]),
                   R_last=relerr(res["R_last"][b], ref["R_last"]))
        worst = {k: max(worst[k], err[k]) for k in worst}
    return worst


@pytest.mark.parametrize("no", range(len(NC.CASES)), ids=NC.IDS)
def test_every_case_against_the_extended_model(no):
    worst = _errors(no)
    print(f"\nbocpd {NC.IDS[no]} (x{NC.CASES[no]['batch']}): log p {worst['logpred']:.2e}, R {worst['R']:.2e}, R_last {worst['R_last']:.2e}")
    assert worst["logpred"] <= LP_BAR and worst["R"] <= R_BAR and worst["R_last"] <= R_BAR, worst


def test_worst_error_per_lane_count():
    """the summary of the net: per lanes-per-workgroup class of the chain kernel, the worst error as a share of its bar"""
    for nl in (256, 128, 64, 32):
        nos = [cs["no"] for cs in NC.CASES if NC.lanes(cs["dim"]) == nl]
        worst = {k: max(_errors(no)[k] for no in nos) for k in ("logpred", "R", "R_last")}
        print(f"\nbocpd net, NL = {nl} ({len(nos)} cases, dims {min(NC.CASES[n]['dim'] for n in nos)} .. {max(NC.CASES[n]['dim'] for n in nos)}): "
              f"worst error / bar: log p {worst['logpred']:.2e} / {LP_BAR:g} = {worst['logpred'] / LP_BAR:.1e}, "
              f"R {worst['R']:.2e} / {R_BAR:g} = {worst['R'] / R_BAR:.1e}, R_last {worst['R_last']:.2e} / {R_BAR:g} = {worst['R_last'] / R_BAR:.1e}")
        assert nos and worst["logpred"] <= LP_BAR and worst["R"] <= R_BAR and worst["R_last"] <= R_BAR
