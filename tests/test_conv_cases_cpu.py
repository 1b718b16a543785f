"""The models of tests/conv_cases.py against the reference's stored convergence run (tests/golden/convergence_expdata.npz: d = 4, r = 1,
n = 1000, 10000 iterations), the admission of the net, and what rpsmf_amd.convergence refuses before it looks for a device.  CPU only.

The stored run has reached its fixed point: iteration 10001, started from the stored C, Xps(:,1), Pps(:,:,1) and v = 1, moves avW by
-1.03e-13, CerrI by -8.9e-13, ErM by -3.6e-15, Xps by at most 5.9e-13 and C by at most 1.2e-12 (measured with the float64 model) --
the stored iteration-to-iteration drift.  Matlab's legacy randn('seed', 5) stream cannot be reproduced, so the start of the stored run
(C, X0ps) is lost and this one further iteration is the known answer there is."""

import os

import numpy as np
import pytest

import conv_cases as CC
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "convergence_expdata.npz")
AVW, CERRI, ERM = 0.08244964400063459, 0.6336846011233929, 10.31679111693605      # entry 10000 of the stored avW, CerrI, ErM


def stored():
    g = dict(np.load(GOLDEN))
    assert g["avW_tail"][-1] == AVW and g["CerrI_tail"][-1] == CERRI and g["ErM_tail"][-1] == ERM
    return g


def stored_case(g, n_iter=1):
    """the case that continues the stored run: iteration 10001 and on"""
    return dict(r=1, d=4, n=1000, n_iter=n_iter, B=1, own=False, Y=g["Y"], Ctrue=g["Ctrue"], Q=g["Q"], Rdiag=g["Rdiag"], x0k=g["X0k"][:, 0],
                P0k=g["P0k"], C0=g["C"][None], x0=g["Xps"][None, :, 0], P0=g["Pps"][None, :, :, 0], v=np.ones(1), q_scale=np.ones(1),
                r_scale=np.ones(1))


def test_the_fixture_is_small_and_holds_data_alone():
    g = stored()
    assert os.path.getsize(GOLDEN) < 1695904 and all(a.dtype == np.float64 for a in g.values())
    assert g["Y"].shape == (4, 1000) and g["Ctrue"].shape == (4, 1) and g["Pk"].shape == (1, 1, 1000) and g["W"].shape == (1, 1000)


def test_the_kalman_pass_reproduces_the_stored_path():
    g = stored()
    Xk, Pk = CC.kalman(g["Y"][None], g["Ctrue"][None], g["Q"], np.diag(g["Rdiag"]), g["X0k"][:, 0][None], g["P0k"][None])
    ex, ep = np.max(np.abs(Xk[0] - g["Xk"])), np.max(np.abs(Pk[0] - g["Pk"]))
    print(f"Kalman replay: Xk {ex:.2e}, Pk {ep:.2e}")
    assert ex < 2e-12 and ep < 2e-12


def test_wasserstein2_reproduces_the_stored_distances():
    g = stored()
    mv = lambda a: np.moveaxis(a, -1, 0)                 # (..., n) -> (n, ...): the steps as the batch
    W = CC.wasserstein2(mv(g["Xps"]), mv(g["Xk"]), mv(g["Pps"]), mv(g["Pk"]))
    err = np.max(np.abs(W[1:] - g["W"][0, 1:]))
    print(f"W(2..n) against the stored W: {err:.2e}")
    assert err < 1e-15 and g["W"][0, 0] == 0.0
    assert abs(np.mean(g["W"][0]) - AVW) < 1e-16       # avW is the mean over all n entries, W(1) = 0 included


def test_the_stored_norms_are_spectral_norms():
    g = stored()
    cerr = CC.norm2(g["C"] - g["Ctrue"])
    E = g["Y"] - g["C"] @ g["Xps"]
    erm = CC.norm2(E)
    assert abs(cerr - CERRI) <= 2 * np.spacing(CERRI), (cerr, CERRI)
    assert abs(erm - ERM) < 2e-14, (erm, ERM)
    fro = np.linalg.norm(E)
    assert 17.6 < fro < 17.7                             # the Frobenius norm of the same matrix: another number altogether
    # and the extended-precision route (the largest eigenvalue of the smaller Gram matrix) is the same norm
    assert abs(float(CC.norm2(E.astype(np.longdouble))) - ERM) < 2e-14


def test_iteration_10001_lands_within_the_stored_drift():
    g = stored()
    m = CC.model(stored_case(g))
    drift = dict(avW=m["avW"][0, 0] - AVW, CerrI=m["CerrI"][0, 0] - CERRI, ErM=m["ErM"][0, 0] - ERM,
                 Xps=np.max(np.abs(m["Xps"][0] - g["Xps"])), C=np.max(np.abs(m["C"][0] - g["C"])))
    print("iteration 10001 minus stored:", {k: f"{v:.2e}" for k, v in drift.items()})
    assert abs(drift["avW"] + 1.03e-13) < 2e-14 and abs(drift["CerrI"] + 8.9e-13) < 1e-13 and abs(drift["ErM"] + 3.6e-15) < 4e-15
    assert drift["Xps"] < 5.9e-13 * 1.05 and drift["C"] < 1.2e-12 * 1.05
    assert abs(m["avW"][0, 0] - g["avW_tail"][-1] - (g["avW_tail"][-1] - g["avW_tail"][-2])) < 2e-14      # the stored run's own last step


def test_the_net_reaches_what_it_claims():
    cases = [CC.draw(i) for i in range(len(CC.SPECS))]
    assert {CC.instance(cs) for cs in cases} == {(r, c) for r in (1, 2, 3, 4) for c in (4, 8, 16)}
    assert {cs["d"] for cs in cases} >= {1, 2, 3, 4, 5, 8, 9, 16} and all(cs["r"] <= cs["d"] for cs in cases)
    assert {cs["B"] for cs in cases} >= {1, 63, 64, 65, 129}
    assert {cs["n"] for cs in cases} >= {2, 50} and {cs["n_iter"] for cs in cases} == {2, 3, 4, 5, 6}
    for r in (1, 2, 3, 4):
        assert {cs["own"] for cs in cases if cs["r"] == r} == {False, True}
        assert {cs["n"] == 2 for cs in cases if cs["r"] == r} == {False, True}
    assert any(len(set(cs["Rdiag"])) > 1 for cs in cases) and any(np.any(cs["q_scale"] != 1) and np.any(cs["r_scale"] != 1) for cs in cases)
    assert all(cs["v"].max() / cs["v"].min() > 10 for cs in cases if cs["B"] >= 63)


@pytest.mark.parametrize("i", range(len(CC.SPECS)))
def test_admission(i):
    (sub, _), log = CC.resolve_case(i)
    assert sub == CC.REPLACED.get(i, 0), (i, sub, log)


def test_at_most_a_quarter_of_the_cases_is_redrawn():
    assert len(CC.REPLACED) <= len(CC.SPECS) // 4 and all(0 <= i < len(CC.SPECS) and s > 0 for i, s in CC.REPLACED.items())


def _args(d=4, r=2, n=10, B=3, own=False):
    rng = np.random.default_rng(5)
    lead = (B,) if own else ()
    return dict(Y=rng.standard_normal(lead + (d, n)), Ctrue=rng.standard_normal((d, r)), C0=rng.standard_normal((B, d, r)),
                x0=rng.standard_normal((B, r)), P0=np.eye(r)), dict(Q=0.1 * np.eye(r), R=0.1, n_iter=2, x0_kalman=np.zeros(r), P0_kalman=np.eye(r))


@pytest.mark.parametrize("name, shape, change, match", [
    ("d > 16", dict(d=17), {}, "d <= 16"),
    ("r > 4", dict(d=8, r=5), {}, "r <= 4"),
    ("r > d", dict(d=2, r=3), {}, "r <= d"),
    ("n < 2", dict(n=1), {}, "n >= 2"),
    ("n_iter < 1", {}, dict(n_iter=0), "n_iter >= 1"),
    ("R <= 0", {}, dict(R=np.array([0.1, 0.0, 0.1, 0.1])), "R > 0"),
    ("R not diagonal", {}, dict(R=0.1 * np.eye(4) + 0.01), "diagonal"),
    ("Q not positive definite", {}, dict(Q=np.array([[1.0, 2.0], [2.0, 1.0]])), "positive definite"),
    ("Q not symmetric", {}, dict(Q=np.array([[1.0, 0.1], [0.0, 1.0]])), "positive definite"),
    ("x0 of another batch", {}, dict(x0=np.zeros((2, 2))), "x0 has shape"),
    ("v of another batch", {}, dict(v=np.ones(4)), "v has shape"),
    ("P0_kalman per replica with shared data", {}, dict(P0_kalman=np.zeros((3, 2, 2))), "shared data takes"),
    ("Ctrue of another batch with own data", dict(own=True), dict(Ctrue=np.zeros((2, 4, 2))), "Ctrue has shape"),
    ("v <= 0", {}, dict(v=0.0), "v > 0"),
])
def test_convergence_batch_refuses_before_it_touches_the_library(name, shape, change, match, monkeypatch):
    from rpsmf_amd import _capi, convergence_batch

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_capi, "load_library", no_library)
    pos, kw = _args(**shape)
    for k, v in change.items():
        (pos if k in pos else kw)[k] = v
    before = {k: np.array(v, copy=True) for k, v in {**pos, **kw}.items()}
    with pytest.raises(ValueError, match=match):
        convergence_batch(pos["Y"], pos["Ctrue"], pos["C0"], pos["x0"], pos["P0"], **kw)
    assert all(np.array_equal(before[k], np.asarray(v)) for k, v in {**pos, **kw}.items()), "an argument was modified"


def test_the_unit_is_built_and_exported():
    import rpsmf_amd
    from rpsmf_amd import _capi, build

    assert "psmf_conv.hip" in build.UNITS and "psmf_conv_run" in _capi.SIGNATURES
    assert callable(rpsmf_amd.convergence_batch) and callable(rpsmf_amd.convergence_experiment)
    fields = [f[0] for f in _capi.PsmfConvConfig._fields_]
    assert fields == ["abi_version", "d", "n", "r", "batch", "n_iter", "own_data", "want_moments", "device"]
