"""Per-row observation noise (a diagonal R with unequal entries) in the one-workgroup masked engine: the row-noise instances of
both column loops (psmf_impute_kernel3w<NG>: d <= 80, r <= 14; psmf_impute_kernel2w: d <= 512, r <= 16) against the CPU oracle run
with the same (d,) vector, and the four drop-in functions against what the reference's own functions returned with R = np.diag(rho)
(tests/golden/impute_row_noise.npz).  Problems as in tests/test_hip_impute_small.py.  GPU only: `pytest -m gpu`.

Tolerances are those of the uniform-R tests of this engine (test_hip_impute_small.py, test_hip_host_and_impute.py): C, X, bands 1e-10
(PSMF, MLE-SMF on the shapes psmf_impute_kernel3 serves) / 1e-8 (rPSMF; d > 80 or r > 14), errors 1e-9, coverage exact."""

import os

import numpy as np
import pytest

import netlib
from conftest import ROOT, relerr
from oracle.impute_oracle import impute_filter, mle_smf_filter
from rpsmf_amd import impute

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def _problem(d, n, r, seed, empty_column=True):
    rng = np.random.default_rng(seed)
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, n)), axis=1)
    M = (rng.random((d, n)) > 0.4).astype(int)
    if d > 3:
        M[2] = 0                     # a row that is never observed
    for t in np.flatnonzero(M.sum(axis=0) == 0):
        M[(0 if d <= 3 else 3), t] = 1
    if empty_column and d >= 12:
        M[:, min(17, n - 1)] = 0     # a column with no observation at all
    Mmiss = ((1 - M) * (rng.random((d, n)) > 0.2)).astype(float)
    return Yorig, M, Mmiss, rng.random((d, r)), rng.random((r, n))


def _rho(d):
    return 10.0 * 100.0 ** (np.random.default_rng(d + 1).random(d) - 0.5)


def _err(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return relerr(np.nan_to_num(a), np.nan_to_num(b))


KERNEL3 = [(7, 3), (19, 10), (19, 9), (25, 7), (32, 14), (48, 14), (75, 10), (80, 13), (2, 1)]
KERNEL2 = [(90, 15), (120, 16), (300, 7), (512, 10)]
OUTPUTS = ("Epred", "Efull", "inside", "C", "X", "Yrec", "YrecL", "YrecH", "status")


def _check(res, ep, ef, ib, st, tol, reps, what=""):
    for rep in reps:
        e = dict(Epred=relerr(res["Epred"][rep], ep[0, 1:]), Efull=relerr(res["Efull"][rep], ef[0, 1:]),
                 inside=abs(res["inside"][rep] - ib), C=relerr(res["C"][rep], st["C"]), X=relerr(res["X"][rep], st["X"]))
        for k in ("Yrec", "YrecL", "YrecH"):
            e[k] = _err(res[k][rep], st[k])
        print(what, res["kernel"], "replica", rep, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert e["Epred"] < 1e-9 and e["Efull"] < 1e-9, (what, e)
        assert e["inside"] < 1e-12, (what, e)
        for k in ("C", "X", "Yrec", "YrecL", "YrecH"):
            assert e[k] < tol, (what, k, e)


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
@pytest.mark.parametrize("d,r", KERNEL3 + KERNEL2)
def test_row_noise_vs_oracle(d, r, robust):
    n = 90
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 100 * d + r)
    rho = _rho(d)
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    ep, ef, ib, st = impute_filter(Yorig * M, C0, X0.copy(), M, Mmiss, V, Q, rho, P, 2, 2, Yorig, 0.0, robust=robust,
                                   lambda0=1.8, return_state=True)
    run = lambda: impute.impute_batch(Yorig, np.stack([M] * 3), np.stack([Mmiss] * 3), np.stack([C0] * 3), np.stack([X0] * 3),
                                      V, Q, rho, P, 2, 2, robust=robust, lambda0=1.8, want_bands=True)
    k3 = (d, r) in KERNEL3
    tol = 1e-8 if (robust or not k3) else 1e-10
    res = run()
    assert res["kernel"].startswith("psmf_impute_kernel3w<") if k3 else res["kernel"] == "psmf_impute_kernel2w"
    assert np.all(res["status"] == 0)
    _check(res, ep, ef, ib, st, tol, (0, 2))
    for k in OUTPUTS:
        assert np.array_equal(res[k][0], res[k][2], equal_nan=True), k            # replicas of one problem: the same bits
    with netlib.env({"PSMF_IMPUTE_V3": "0"}):
        res2 = run()
    assert res2["kernel"] == "psmf_impute_kernel2w"
    _check(res2, ep, ef, ib, st, tol, (0, 2), "PSMF_IMPUTE_V3=0")
    if (d, r) in ((19, 10), (7, 3), (75, 10)):
        with netlib.env({"PSMF_IMPUTE_PAR": "0"}):
            res3 = run()
        _check(res3, ep, ef, ib, st, tol, (0, 2), "PSMF_IMPUTE_PAR=0")


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
def test_row_noise_general_Q(robust):
    """Q not a multiple of the identity: wave 0 inverts P + Q and (P + Q)^-1 + G_R in turn."""
    d, n, r = 19, 90, 10
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 100 * d + r)
    rho = _rho(d)
    B = np.random.default_rng(6).standard_normal((r, r))
    V, Q, P = 2 * np.eye(r), 0.05 * np.eye(r) + 0.01 * B @ B.T, np.eye(r)
    ep, ef, ib, st = impute_filter(Yorig * M, C0, X0.copy(), M, Mmiss, V, Q, rho, P, 2, 2, Yorig, 0.0, robust=robust,
                                   lambda0=1.8, return_state=True)
    res = impute.impute_batch(Yorig, M, Mmiss, C0, X0, V, Q, rho, P, 2, 2, robust=robust, lambda0=1.8, want_bands=True)
    _check(res, ep, ef, ib, st, 1e-8 if robust else 1e-10, (0,), "general Q")


@pytest.mark.parametrize("d,r", [(19, 10), (32, 14), (120, 16)])
def test_row_noise_mle_smf(d, r):
    n = 150
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 40 + d, empty_column=False)
    rho = _rho(d)
    Q, P = 0.1 * np.eye(r), np.eye(r)
    ep, ef, ib, st = mle_smf_filter(Yorig * M, C0, X0.copy(), M, Mmiss, Q, rho, P, 2, 2, Yorig, 0.0, return_state=True)
    res = impute.impute_batch(Yorig, M, Mmiss, C0, X0, np.eye(r), Q, rho, P, 2, 2, method="mle_smf", want_bands=True)
    _check(res, ep, ef, ib, st, 1e-10 if d <= 80 else 1e-8, (0,), "MLE-SMF")


def test_tmf_ignores_the_noise_vector():
    d, n, r = 19, 90, 10
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 100 * d + r)
    a = impute.impute_batch(Yorig, M, Mmiss, C0, X0, np.eye(r), np.eye(r), 10.0, np.eye(r), 2, 2, method="tmf")
    b = impute.impute_batch(Yorig, M, Mmiss, C0, X0, np.eye(r), np.eye(r), _rho(d), np.eye(r), 2, 2, method="tmf")
    assert a["kernel"] == b["kernel"]
    for k in ("Epred", "Efull", "C", "X", "status"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("d,r", [(19, 10), (120, 16)])
def test_constant_diagonal_is_the_scalar_call(d, r):
    n = 90
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 100 * d + r)
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    run = lambda R: impute.impute_batch(Yorig, M, Mmiss, C0, X0, V, Q, R, P, 2, 2, robust=True, lambda0=1.8, want_bands=True)
    a = run(10.0)
    for R in (np.full(d, 10.0), 10.0 * np.eye(d)):
        b = run(R)
        assert b["kernel"] == a["kernel"]
        for k in OUTPUTS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("tag", ["a", "b"])
def test_drop_in_functions_return_the_reference_s_numbers(tag):
    """ProbabilisticSequentialMatrixFactorizer / robust_PSMF / stochasticGradientStateSpaceMF with R = np.diag(rho), unequal
    entries, against the return values of the reference's functions on the same arguments."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "impute_row_noise.npz"))
    Yorig, Mmiss, M = G[tag + "_Yorig"], G[tag + "_Mmiss"].astype(float), G[tag + "_M"].astype(int)
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    Y, C0, X0, rho, Einit = YorigInt * M, G[tag + "_C0"], G[tag + "_X0"], G[tag + "_rho"], float(G[tag + "_Einit"])
    d, n = Y.shape
    r = C0.shape[1]
    V, Q, P, R = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r), np.diag(rho)
    calls = {
        "psmf": lambda X: impute.ProbabilisticSequentialMatrixFactorizer(Y, C0.copy(), X, d, n, r, M, Mmiss, 10, V, Q, R, P, 2, 2, YorigInt, Einit),
        "rpsmf": lambda X: impute.robust_PSMF(Y, C0.copy(), X, d, n, r, M, Mmiss, V, Q, R, P, 1.8, 2, 2, YorigInt, Einit),
        "mle": lambda X: impute.stochasticGradientStateSpaceMF(Y, C0.copy(), X, d, n, r, M, Mmiss, 10, Q, R, P, 2, 2, YorigInt, Einit),
    }
    for method, call in calls.items():
        X = X0.copy()
        ep, ef, rt, ib = call(X)
        e = dict(Epred=relerr(ep, G[f"{tag}_{method}_Epred"]), Efull=relerr(ef, G[f"{tag}_{method}_Efull"]),
                 inside=abs(ib - float(G[f"{tag}_{method}_inside"])), X=relerr(X, G[f"{tag}_{method}_X"]))
        print(tag, method, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert ep.shape == (1, 3) and rt.shape == (1, 3) and ep[0, 0] == Einit
        assert e["Epred"] < 1e-9 and e["Efull"] < 1e-9 and e["inside"] < 1e-12 and e["X"] < 1e-8, (tag, method, e)


def test_device_list_with_a_noise_vector():
    d, n, r, B = 19, 90, 10, 7
    Yorig, M, Mmiss, C0, X0 = _problem(d, n, r, 321)
    rng = np.random.default_rng(5)
    Ms = np.stack([(rng.random((d, n)) > 0.3).astype(float) for _ in range(B)])
    Mm = 1.0 - Ms
    Cs = np.stack([rng.random((d, r)) for _ in range(B)])
    Xs = np.stack([rng.random((r, n)) for _ in range(B)])
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    one = impute.impute_batch(Yorig, Ms, Mm, Cs, Xs, V, Q, _rho(d), P, 2, 2, robust=True, lambda0=1.8, want_bands=True)
    three = impute.impute_batch(Yorig, Ms, Mm, Cs, Xs, V, Q, _rho(d), P, 2, 2, robust=True, lambda0=1.8, want_bands=True, device=[0, 0, 0])
    assert three["devices"] == [(0, 0, 3), (0, 3, 5), (0, 5, 7)]
    for k in OUTPUTS:
        assert np.array_equal(one[k], three[k], equal_nan=True), k


def test_c_abi_refuses_what_it_cannot_run():
    """psmf_impute_run_rows itself: unequal entries on a shape of the large-d handle, a negative entry."""
    import ctypes as C

    from rpsmf_amd import _capi

    lib = _capi.load_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    for d, r, rho, word in ((600, 4, np.linspace(1.0, 2.0, 600), "d <= 512 and r <= 16"), (19, 4, -np.linspace(1.0, 2.0, 19), "finite and >= 0")):
        n = 4
        cfg = _capi.PsmfImputeConfig(abi_version=_capi.ABI_VERSION, d=d, n=n, r=r, batch=1, method=0, n_iter=1, sig=2.0)
        Y, Mk, Cm, X, E = np.zeros((n, d)), np.ones((n, d), dtype=np.uint8), np.ones((d, r)), np.ones((n, r)), np.eye(r)
        out = np.zeros(4)
        rc = lib.psmf_impute_run_rows(C.byref(cfg), dp(Y), up(Mk), up(Mk), dp(Cm), dp(X), dp(E), dp(E), dp(E), dp(rho), dp(out), dp(out),
                                      dp(out), None, None, None, None, None)
        assert rc == _capi.ERR_ARG and word in lib.psmf_last_error(None).decode()
