"""tests/masked_dyn_cases.py without a GPU: the model of a masked step with dynamics and the conditioning of every case.

(1) With the random walk the model is the ExperimentImpute filter: C and X of oracle.impute_oracle.impute_filter to 1e-12.
(2) With an all-ones mask and the non-robust filter (n_obs = d) the model's state and gradient sum are O.run_epoch's with the same
    dynamics to 1e-12.
(3) The closed-form g_f = n_obs w / N - h / N - ee w / N^2 is the gradient of the reference's masked incremental likelihood
    (pypsmf/psmf/psmf.py:264-270, rpsmf.py:196-200, restated in masked_dyn_cases.reference_ll): central differences of step 1e-6
    agree to 1e-6 relative at d = 12, r = 3, a step without any observation included (both are exactly zero there).
(4) The closed-form F and J_theta of rpsmf_amd/nonlinearities.py that the model differentiates with are the complex-step
    derivatives of the same callables.
(5) Every case is well enough conditioned for the device bars to mean something: a last-bit change of C0 and mu0 moves C, V, P, the
    mean history, y_hat and the gradient sum by at most 1e-11 (the cap of tests/test_masked_noise_cases_cpu.py) and theta of the
    in-loop cases by at most 1e-9 -- conditions on the inputs, not tolerances of the device.
(6) On every case the gradient with n_obs differs from the one with d by more than 1e-3 relative: a kernel that keeps d in the first
    term cannot pass the device test."""

import numpy as np
import pytest

import masked_dyn_cases as D
from oracle import psmf_oracle as O
from oracle.impute_oracle import impute_filter


def test_the_list_is_the_one_the_issue_states():
    shapes = {(c["d"], c["r"], c["T"], c["dyn"]) for c in D.CASES}
    assert shapes == {(40, 3, 30, "cos_phase"), (300, 10, 40, "scaled_walk_bias"), (300, 10, 40, "sinusoid"), (530, 20, 40, "fourier2"),
                      (300, 40, 24, "sinusoid_unscaled")}
    for c in D.CASES:
        same = [x for x in D.CASES if (x["dyn"], x["update_every"]) == (c["dyn"], c["update_every"])]
        assert {(x["robust"], x["storage"]) for x in same} == {(False, "f64"), (False, "f32"), (True, "f64"), (True, "f32")}
        assert c["r"] >= 3 and c["update_every"] in (0, 2, 3)
        # the step without observations is never the only step of an optimiser window
        assert c["update_every"] != 1 and D.EMPTY_STEP <= c["T"]
    loops = {(c["dyn"], c["optim"], c["update_every"]) for c in D.CASES if c["update_every"]}
    assert loops == {("cos_phase", "adam", 2), ("sinusoid", "adam", 3), ("sinusoid_unscaled", "sgd", 2)}
    assert len(D.CASES) == len(set(D.IDS)) == 32


@pytest.mark.parametrize("cs", [c for c in D.CASES if c["storage"] == "f64" and not c["update_every"]][:2], ids=["PSMF", "rPSMF"])
def test_random_walk_model_is_the_impute_filter(cs):
    """(1) f = the random walk: the ExperimentImpute step the masked handle runs today"""
    pb = D.problem(cs)
    d, r, T = cs["d"], cs["r"], cs["T"]
    M = pb["M"].astype(float)
    assert M[D.EMPTY_STEP - 1].sum() == 0 and 0.5 < M.mean() < 0.65
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=2.0, lam=D.LAMBDA0)
    X = np.empty((T, r))
    for k in range(1, T + 1):
        st, _ = D.model_step(st, pb["Y"][k - 1], k, O.Mode(robust=cs["robust"]), O.RandomWalkDyn(), M[k - 1])
        X[k - 1] = st.mu
    X0 = np.zeros((r, T))
    X0[:, T - 1] = pb["mu0"]
    with np.errstate(all="ignore"):
        _, _, _, ref = impute_filter(pb["Y"].T * M.T, pb["C0"], X0, M.T, 1.0 - M.T, pb["V0"], pb["Q"], 2.0, pb["P0"], 2.0, 1, pb["Y"].T, 0.0,
                                     robust=cs["robust"], lambda0=D.LAMBDA0, return_state=True)
    errs = dict(C=D.relerr(st.C, ref["C"]), X=D.relerr(X, ref["X"].T), V=D.relerr(st.V, ref["V"]), P=D.relerr(st.P, ref["P"]))
    print(f"\nrandom-walk model against impute_filter: {errs}")
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("cs", [c for c in D.CASES if c["storage"] == "f64" and not c["robust"] and not c["update_every"]],
                         ids=lambda c: c["dyn"])
def test_all_ones_mask_is_the_unmasked_epoch(cs):
    """(2) m = 1 everywhere, non-robust: n_obs = d, the model is lowrank_step's own want_grad branch"""
    pb = D.problem(cs)
    dyn = D.ClosedFormDyn(pb["nl"])
    n = pb["nl"].n_params
    mk = lambda: O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=1.0, lam=0.0,
                         theta=pb["theta0"].copy(), gradsum=np.zeros(n))
    ref, Yp, _ = O.run_epoch(mk(), pb["Y"], O.Mode(), dyn)
    st = mk()
    yp = np.empty_like(Yp)
    for k in range(1, cs["T"] + 1):
        st, info = D.model_step(st, pb["Y"][k - 1], k, O.Mode(), dyn, np.ones(cs["d"]))
        yp[k - 1] = info.y_pred
    errs = {k: D.relerr(getattr(st, k), getattr(ref, k)) for k in ("C", "V", "P", "mu", "gradsum")}
    errs["yp"] = D.relerr(yp, Yp)
    print(f"\nall-ones mask {cs['dyn']}: {errs}")
    assert np.max(np.abs(ref.gradsum)) > 0 and max(errs.values()) <= 1e-12, errs


def test_closed_form_gf_is_the_gradient_of_the_masked_likelihood():
    """(3) central differences of the restated ll, step 1e-6, 1e-6 relative; d = 12, r = 3; one step has n_obs = 0"""
    d, r = 12, 3
    rng = np.random.default_rng(77)
    B = rng.standard_normal((r, r))
    V = 0.3 * np.eye(r) + 0.05 * B @ B.T
    B = rng.standard_normal((r, r))
    Pbar = np.eye(r) + 0.1 * B @ B.T
    worst = 0.0
    for trial, mask in enumerate([(rng.random(d) > 0.4).astype(float), np.zeros(d), np.ones(d), np.eye(d)[5]]):
        C, mb, y = rng.standard_normal((d, r)), rng.standard_normal(r), rng.standard_normal(d)
        rho = 0.7
        ll, eta = D.reference_ll(C, V, Pbar, mb, y, mask, rho)
        w, s = V @ mb, float(mb @ V @ mb)
        e = mask * (y - C @ mb)
        gf = D.masked_gf(w, C.T @ e, float(e @ e), s + eta, float(mask.sum()))
        fd = np.empty(r)
        for i in range(r):
            hp, hm = mb.copy(), mb.copy()
            hp[i] += 1e-6
            hm[i] -= 1e-6
            fd[i] = (ll(hp) - ll(hm)) / 2e-6
        err = float(np.max(np.abs(gf - fd))) / max(float(np.max(np.abs(fd))), 1e-300)
        print(f"\nmask {trial} (n_obs = {int(mask.sum())}): g_f {gf}, central difference {fd}, relative {err:.2e}")
        if mask.sum() == 0:
            assert np.all(gf == 0.0) and np.all(fd == 0.0)
        else:
            assert err <= 1e-6, (trial, err)
            # ... and not of the likelihood with d in the first term
            assert float(np.max(np.abs(D.masked_gf(w, C.T @ e, float(e @ e), s + eta, d) - fd))) > 1e-3 * float(np.max(np.abs(fd))) or mask.sum() == d
        worst = max(worst, err)
    assert worst > 0.0


@pytest.mark.parametrize("shape", D.SHAPES, ids=[s[3] for s in D.SHAPES])
def test_closed_form_jacobians_are_the_complex_step_ones(shape):
    """(4)"""
    _, r, _, name, make = shape
    nl = make(r)
    rng = np.random.default_rng(5 + r)
    theta, x = D.theta_for(nl, rng, r), 0.3 * rng.standard_normal(r)
    a, b = D.ClosedFormDyn(nl), O.CallableDyn(nl, nl.n_params)
    for t in (1, 17):
        assert D.relerr(a.f(theta, x, t), b.f(theta, x, t)) <= 1e-15
        assert D.relerr(a.jac_x(theta, x, t), b.jac_x(theta, x, t)) <= 1e-13
        assert D.relerr(a.jac_theta(theta, x, t), b.jac_theta(theta, x, t)) <= 1e-13


@pytest.mark.parametrize("cs", D.CASES, ids=D.IDS)
def test_case_by_the_model_alone(cs):
    """(5), (6)"""
    pb, ref = D.reference(cs)
    M = pb["M"]
    assert 0.5 < M.mean() < 0.65 and M[D.EMPTY_STEP - 1].sum() == 0 and not M[:, 3].any()
    assert all(M[k].sum() > 0 for k in range(cs["T"]) if k != D.EMPTY_STEP - 1)
    for k in D.STATE_KEYS + ("gradsum", "theta", "pred"):
        assert np.all(np.isfinite(ref[k])), k
    pert = D.run_model(cs, D.problem(cs, perturb=(cs["d"] + cs["T"], 2.0 ** -52)))
    cond = {k: D.relerr(pert[k], ref[k]) for k in D.STATE_KEYS}
    cond["windows"] = max(D.relerr(a, b) for a, b in zip(pert["windows"], ref["windows"]))
    cond_theta = D.relerr(pert["theta"], ref["theta"])
    with_d = D.run_model(cs, pb, count=cs["d"])
    # the first window: the same theta and the same states on both sides, only the count differs
    differs = D.relerr(with_d["windows"][0], ref["windows"][0])
    moved = float(np.max(np.abs(ref["theta"] - pb["theta0"])))
    print(f"\nmasked dynamics case {D.IDS[D.CASES.index(cs)]}: last bit of C0, mu0 moves {cond}, theta {cond_theta:.2e}; "
          f"gradient with d against n_obs {differs:.2e}; theta moved by {moved:.2e}")
    assert max(cond.values()) <= 1e-11, cond
    assert cond_theta <= 1e-9
    assert differs > 1e-3
    assert moved > 0.0 and np.max(np.abs(ref["windows"][0])) > 0.0
