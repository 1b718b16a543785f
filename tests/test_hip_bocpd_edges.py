"""psmf_bocpd_run at its edges, directed: the smallest and the largest T, the chunked host loop (PSMF_BOCPD_CHUNK), a failure that only
the device can find, an outlier that hypotheses absorb and carry on, a prior far off the data's scale, and the optional outputs of the C
ABI left out.  The reference is extended_model of tests/bocpd_cases.py (np.longdouble, mpmath's lgamma).

Bars: those of tests/test_hip_bocpd.py (log p within 1e-10 absolute where live, NaN exactly where not; R and R_last within 5e-9 in
conftest.relerr; map_run and the change points exactly) wherever the float64 model is itself good to 1e-11.  Where it is not -- log p
of a hypothesis that has absorbed a 1e100 sample, and data at scale 1e3 under sigma0 = 1 -- the float64 model misses 1e-10 itself, and
the bar on log p is 10 x the distance MEASURED in the test between the float64 stable_model and the extended model on that series (the
device rounds differently -- fma, x rsqrt(x), the carried log-determinant -- but runs the same algebra), floored at 1e-10."""

import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest

import bocpd_cases as BC
import bocpd_net_cases as NC
from conftest import relerr

pytestmark = pytest.mark.gpu

LP_BAR = 1e-10
R_BAR = 5e-9
ERR_NUMERIC = -4
CHUNK = "PSMF_BOCPD_CHUNK"
KEYS = ("map_run", "n_changepoints", "R_last", "R", "logpred", "status")

assert np.finfo(np.longdouble).eps < 1.1e-19, "these tests need an 80-bit long double: extended_model is no reference without it"


def _run(X, **kw):
    from rpsmf_amd.changepoint import mvbocpd_batch

    return mvbocpd_batch(X, **kw)


def _with_chunk(value, fn):
    """fn() with PSMF_BOCPD_CHUNK set to `value` (None: unset); the library reads it at every call"""
    old = os.environ.get(CHUNK)
    if value is None:
        os.environ.pop(CHUNK, None)
    else:
        os.environ[CHUNK] = str(value)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(CHUNK, None)
        else:
            os.environ[CHUNK] = old


def _compare(res, b, ref):
    """worst errors of replica b against a model's result; asserts the exact quantities"""
    live = ~np.isnan(ref["logpred"])
    assert np.array_equal(~np.isnan(res["logpred"][b]), live), "log p is NaN exactly where the age is not live"
    assert np.array_equal(res["map_run"][b], ref["map_run"])
    assert list(res["changepoints"][b]) == ref["changepoints"] and res["n_changepoints"][b] == len(ref["changepoints"])
    return dict(logpred=float(np.max(np.abs(res["logpred"][b][live] - ref["logpred"][live]))), R=relerr(res["R"][b], ref["R"]),
                R_last=relerr(res["R_last"][b], ref["R_last"]))


def _distance(a, b):
    """the worst distance on log p between two models' results that are live in the same places"""
    live = ~np.isnan(b["logpred"])
    assert np.array_equal(~np.isnan(a["logpred"]), live)
    return float(np.max(np.abs(a["logpred"][live] - b["logpred"][live])))


def _identical(a, b, rows=None):
    """every output of two runs, bit for bit (over the replicas `rows`)"""
    rows = range(len(a["status"])) if rows is None else rows
    for k in KEYS:
        assert np.array_equal(a[k][list(rows)], b[k][list(rows)], equal_nan=True), k
    for r in rows:
        assert list(a["changepoints"][r]) == list(b["changepoints"][r])


# ---- the smallest and the largest T ----

@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("dim", [1, 13, 32])
def test_one_and_two_steps(dim, T):
    X = np.random.default_rng([511, dim, T]).standard_normal((2, dim, T)) + 2.0
    prm = dict(lam=20.0, kappa0=0.5, nu0=dim - 0.5, sigma0=2.0, drop=0, settle=1, confirm=0)
    res = _run(X, **prm, want_R=True, want_logpred=True)
    assert list(res["status"]) == [0, 0] and res["R"].shape == (2, T + 1, T + 1) and res["logpred"].shape == (2, T, T)
    for b in range(2):
        ref = BC.extended_model(X[b], **prm)
        err = _compare(res, b, ref)
        print(f"\nbocpd dim {dim}, T = {T}, replica {b}: {err}")
        assert res["map_run"][b][0] == 1 and res["n_changepoints"][b] == 0
        assert err["logpred"] <= LP_BAR and err["R"] <= R_BAR and err["R_last"] <= R_BAR, err


LONG_T, LONG_AT = 4096, 3500


@lru_cache(maxsize=None)
def _long():
    """dim 1, T = 4096 -- slogR[T] is the post kernel's last LDS slot --, N(3, 1) moving to N(-3, 1) at step 3500: 3500 hypotheses are
    live, carried by the chain kernel for up to 3500 steps, when the truncation comes"""
    X = np.random.default_rng(4096).standard_normal((1, LONG_T)) + 3.0
    X[:, LONG_AT:] -= 6.0
    return X, BC.extended_model(X), BC.stable_model(X)


def test_the_longest_series_and_the_carried_log_determinant():
    X, ref, st = _long()
    assert _distance(st, ref) <= 1e-11 and BC.column_gap(ref["R"]) >= 1e-6      # the admission of the net, for this series
    assert len(ref["changepoints"]) == 1 and ref["changepoints"][0] > LONG_AT - 5
    t = ref["declared_at"][0]
    assert t + 1 > 3500 and ref["map_run"][t] < 64      # live before the truncation, and after it
    res = _run(X, want_R=True, want_logpred=True)
    assert list(res["status"]) == [0]
    err = _compare(res, 0, ref)
    live = ~np.isnan(ref["logpred"])
    old = live & (np.arange(LONG_T)[None, :] > 2000)      # [t][age]
    assert old.sum() > 1000000
    drift = float(np.max(np.abs(res["logpred"][0][old] - ref["logpred"][old])))
    print(f"\nbocpd dim 1, T = 4096: {err}; worst log p error at age > 2000 (the carried log-determinant's drift): {drift:.2e}; "
          f"change point {list(res['changepoints'][0])} declared at step {t + 1}; {res['elapsed_ms']:.3f} ms")
    assert res["R"][0][LONG_T, 0] == res["R_last"][0][0] > 0.0
    assert err["logpred"] <= LP_BAR and drift <= LP_BAR and err["R"] <= R_BAR and err["R_last"] <= R_BAR, (err, drift)


# ---- the chunked host loop, and a failure only the device finds ----

CHUNK_CASE = 39      # dim 20, T 65 (two blocks of 64 births), a change point in every replica
HUGE = 1e200         # finite: the host's scan passes it; w^2 overflows in the chain kernel and log p is NaN


@lru_cache(maxsize=None)
def _seven():
    """seven series of a net case: replica 4 holds a NaN (the host finds it), replica 6 a sample of 1e200 at mid-series (only the device does);
    the clean batch, the spoilt batch and the spoilt batch's run with the chunk sized from memory"""
    cs = NC.CASES[CHUNK_CASE]
    assert cs["T"] > NC.lanes(cs["dim"])
    clean = np.stack([NC.series(cs, b) for b in range(7)])
    X = clean.copy()
    X[4, 3, 17] = np.nan
    X[6, 5, cs["T"] // 2] = HUGE
    kw = dict(**NC.params(cs), max_changepoints=16, want_R=True, want_logpred=True)
    return clean, X, kw, _with_chunk(None, lambda: _run(X, **kw))


def test_a_failure_found_on_the_device_fails_its_replica_alone():
    clean, X, kw, res = _seven()
    assert np.isfinite(X[6]).all()
    assert list(res["status"]) == [0, 0, 0, 0, ERR_NUMERIC, 0, ERR_NUMERIC]
    good = _with_chunk(None, lambda: _run(clean, **kw))
    assert not good["status"].any()
    _identical(res, good, rows=(0, 1, 2, 3, 5))
    for b in (0, 3, 5):
        err = _compare(res, b, NC.reference(CHUNK_CASE, b)[1])
        assert err["logpred"] <= LP_BAR and err["R"] <= R_BAR and err["R_last"] <= R_BAR, (b, err)
    assert any(len(c) for c in good["changepoints"])
    for b in (4, 6):      # include/psmf_hip.h: every other output of such a replica is zero
        assert not res["map_run"][b].any() and res["n_changepoints"][b] == 0 and len(res["changepoints"][b]) == 0
        assert not res["R_last"][b].any() and not res["R"][b].any() and not res["logpred"][b].any()
    with pytest.raises(np.linalg.LinAlgError, match="replica 6"):
        _run(X[[0, 1, 2, 3, 5, 5, 6]], **{**kw, "status": None})
    with pytest.raises(np.linalg.LinAlgError, match="replica 4"):
        _run(X, **{**kw, "status": None})


@pytest.mark.parametrize("chunk", [3, 1, 7])
def test_chunks_of_series_give_the_same_bits(chunk):
    clean, X, kw, whole = _seven()
    res = _with_chunk(chunk, lambda: _run(X, **kw))      # 3 + 3 + 1: the NaN in the second chunk, the device's failure in the third
    _identical(res, whole)
    assert list(res["status"]) == [0, 0, 0, 0, ERR_NUMERIC, 0, ERR_NUMERIC]
    assert res["elapsed_ms"] > 0 and whole["elapsed_ms"] > 0
    plain = _with_chunk(chunk, lambda: _run(X, **{k: v for k, v in kw.items() if not k.startswith("want_")}))
    assert plain["R"] is None and plain["logpred"] is None
    assert all(np.array_equal(plain[k], whole[k]) for k in ("map_run", "n_changepoints", "R_last", "status"))
    with pytest.raises(np.linalg.LinAlgError, match="replica 4"):
        _with_chunk(chunk, lambda: _run(X, **{**kw, "status": None}))


def test_the_chunk_switch_is_read_at_every_call():
    X = NC.series(NC.CASES[CHUNK_CASE], 0)
    with pytest.raises(ValueError, match=CHUNK):
        _with_chunk(-1, lambda: _run(X))
    assert _with_chunk(0, lambda: _run(X))["status"][0] == 0 and _with_chunk(None, lambda: _run(X))["status"][0] == 0


# ---- an outlier that hypotheses absorb and carry on ----

@pytest.mark.parametrize("channels", [(1.0, 1.0, 1.0), (1.0, -0.3, 2.0)], ids=["equal", "unequal"])
def test_an_outlier_at_mid_series(channels):
    """Every channel at 1e100 (bocpd_cases.OUTLIER), or at unequal multiples of it, at step `mid`.  Every p_a of that step underflows.  The hypotheses born at or before
    it absorb the sample and are evaluated afterwards with a factor of size 1e100 and a mean of size 1e100 / (kappa + 1): their log p (near
    -231 in exact arithmetic, the log-determinant's share) hangs on a cancellation that neither float64 nor the 80-bit format can carry
    and comes out anywhere between -230 and -7000 in both.  The bar there is 10 x what separates the two models: it says that the device
    stays finite, not more.  Those hypotheses weigh exp(-200) in R, so the ones born after `mid`, R_last and map_run keep the usual bars."""
    dim, T, mid = 3, 60, 30
    X = np.random.default_rng(77).standard_normal((2, dim, T))
    X[:, :, 30:] += 4.0
    X[:, :, mid] = BC.OUTLIER * np.array(channels)
    prm = dict(lam=20.0)
    res = _run(X, **prm, want_R=True, want_logpred=True)
    assert list(res["status"]) == [0, 0]
    for b in range(2):
        ref, st = BC.extended_model(X[b], **prm), BC.stable_model(X[b], **prm)
        assert BC.column_gap(ref["R"]) >= 1e-6 and np.array_equal(st["map_run"], ref["map_run"])
        measured = _distance(st, ref)
        bar = max(10.0 * measured, LP_BAR)
        live = ~np.isnan(ref["logpred"])
        assert np.array_equal(~np.isnan(res["logpred"][b]), live)
        d = np.where(live, np.abs(res["logpred"][b] - ref["logpred"]), 0.0).astype(float)
        birth = np.arange(T)[:, None] - np.arange(T)[None, :]                 # [t][age] -> t - age
        absorbed = live & (birth <= mid) & (np.arange(T)[:, None] > mid)      # evaluated after it has absorbed the outlier
        assert absorbed.sum() > 50 and np.isfinite(res["logpred"][b][live]).all()
        assert float(np.max(np.exp(res["logpred"][b][mid][live[mid]]))) == 0.0      # every p_a of the step underflows
        assert float(np.max(ref["logpred"][absorbed])) < -200.0 and float(np.max(st["logpred"][absorbed])) < -200.0
        print(f"\nbocpd outlier {channels} x 1e100 at mid-series, replica {b}: the float64 model is {measured:.3e} from the extended one on log p (bar {bar:.3e}); the device "
              f"is {d.max():.3e} from it over all live entries, {d[absorbed].max():.3e} over the {absorbed.sum()} that absorbed the outlier, "
              f"{d[live & ~absorbed].max():.3e} over the rest; R_last {relerr(res['R_last'][b], ref['R_last']):.2e}")
        assert d.max() <= bar
        assert d[live & ~absorbed].max() <= LP_BAR
        assert np.isfinite(res["R_last"][b]).all() and abs(res["R_last"][b].sum() - 1.0) < 1e-12
        assert relerr(res["R_last"][b], ref["R_last"]) <= R_BAR and np.array_equal(res["map_run"][b], ref["map_run"])


# ---- a prior far off the data's scale ----

@pytest.mark.parametrize("dim", [5, 32])
def test_an_ill_scaled_prior(dim):
    """Data at scale 1e3 under sigma0 = 1: the first sample moves the factor by six orders of magnitude, and the float64 model, with the
    textbook rank-one update, loses about eight digits of log p (rpsmf_amd/changepoint.py).  The bar on log p is 10 x that model's distance
    from the extended one, measured here.  (The device, with w_i <- (w_i - s L_ik) / c, was measured at 2.7e-12 and 8.3e-12.)"""
    T = 100
    X = 1e3 * (np.random.default_rng(1000 + dim).standard_normal((dim, T)) + 2.0)
    X[:, 50:] -= 4e3
    prm = dict(lam=50.0, sigma0=1.0)
    ref, st = BC.extended_model(X, **prm), BC.stable_model(X, **prm)
    gap = BC.column_gap(ref["R"])
    assert gap >= 1e-6
    measured = _distance(st, ref)
    bar = max(10.0 * measured, LP_BAR)
    res = _run(X, **prm, want_R=True, want_logpred=True)
    assert list(res["status"]) == [0]
    err = _compare(res, 0, ref)      # map_run and the change points exactly: the gap allows it
    print(f"\nbocpd ill-scaled prior, dim {dim}: the float64 model is {measured:.3e} from the extended one on log p (bar {bar:.3e}); the device {err}; "
          f"least column gap {gap:.2e}")
    assert err["logpred"] <= bar, (err, bar)


# ---- the C ABI with its optional outputs left out ----

def test_the_c_abi_without_its_optional_outputs():
    from rpsmf_amd import _capi

    cs = NC.CASES[CHUNK_CASE]
    X = np.stack([NC.series(cs, b) for b in range(3)])
    B, dim, T = X.shape
    full = _run(X, **NC.params(cs), max_changepoints=16)
    assert full["n_changepoints"].any()
    Xt = np.ascontiguousarray(np.transpose(X, (0, 2, 1)))
    map_run, ncp = np.full((B, T), -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    p = NC.params(cs)
    cfg = _capi.PsmfBocpdConfig(abi_version=_capi.ABI_VERSION, dim=dim, T=T, batch=B, device=0, drop=p["drop"], settle=p["settle"], confirm=p["confirm"],
                                max_changepoints=0, want_R=0, want_logpred=0, lam=p["lam"], kappa0=p["kappa0"], nu0=p["nu0"], sigma0=p["sigma0"])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    lib = _capi.load_library()
    rc = lib.psmf_bocpd_run(C.byref(cfg), Xt.ctypes.data_as(C.POINTER(C.c_double)), ip(map_run), None, ip(ncp), None, None, None, None, None)
    assert rc == _capi.OK, lib.psmf_last_error(None).decode()
    assert np.array_equal(map_run, full["map_run"]) and np.array_equal(ncp, full["n_changepoints"])
    # with no status array a failed replica fails the call, whatever else is left out
    Xt[1, T // 2, 0] = HUGE
    rc = lib.psmf_bocpd_run(C.byref(cfg), Xt.ctypes.data_as(C.POINTER(C.c_double)), ip(map_run), None, ip(ncp), None, None, None, None, None)
    assert rc == _capi.ERR_NUMERIC and "replica 1" in lib.psmf_last_error(None).decode()
