"""tests/ssm_cases.py without a GPU: every case of the batched PSMF with linear-Gaussian dynamics and an observation map (1) runs to
finite values in the line-for-line model of ExperimentChange/PSMF.m:6-45; (2) admits the r x r algebra the kernel implements:
device_algebra_model agrees with literal_model to 1e-11 on X, C, V, P, x, yhat, (s, eta) before any GPU run; (3) is conditioned well
enough for the device bar (5e-9) to mean something: C0 and x0 moved by 4 * 2^-52 move every compared array by at most 1e-11 -- a
condition on the inputs, 500 x below the device bar, not a tolerance of the device; (4) depends on carry_P: X of the two values
differs by more than 1e-2, so a kernel that ignores the flag cannot pass; (5) depends on H and on the p-dimensional state: the
engine every other entry point of the library is -- x in R^r, y ~ C x, i.e. H dropped and A, Q, P0, x0 cut to their leading r x r
blocks -- gives an X that differs by more than 1e-2 from the first r rows of the case's.  (For the Matern model H = [I 0] selects
exactly those rows, and at p = r the blocks are the matrices themselves: cutting the state is what tells the engines apart in the
first case, dropping H in the second; every case moves.)
Then matern32_state_space against the matrix exponential, and the argument checks of rpsmf_amd/ssm.py that need no device."""

import numpy as np
import pytest

import ssm_cases as SC
from rpsmf_amd import ssm


def test_the_list_is_the_one_the_device_test_runs():
    shapes = [(c["d"], c["n"], c["r"], c["p"], c["kind"]) for c in SC.CASES if c["carry_P"] == 1]
    assert shapes == [(5, 40, 2, 4, "matern"), (5, 40, 2, 4, "dense"), (33, 50, 7, 7, "dense"), (20, 150, 10, 20, "matern"),
                      (200, 40, 12, 24, "matern"), (96, 60, 16, 32, "matern"), (96, 60, 16, 32, "dense"), (512, 30, 3, 7, "dense")]
    assert [c for c in SC.CASES if c["carry_P"] == 0] == [dict(c, carry_P=0) for c in SC.CASES if c["carry_P"] == 1]
    assert max(c["d"] for c in SC.CASES) == ssm.MAX_D and max(c["r"] for c in SC.CASES) == ssm.MAX_R and max(c["p"] for c in SC.CASES) == ssm.MAX_P
    pb = SC.problem(SC.find(5, 2, "matern", 0))
    assert 6e-7 < pb["Q"][0, 0] < 8e-7 and pb["rho"] == 1e-3 and np.array_equal(pb["V"], np.eye(2))
    pb = SC.problem(SC.find(5, 2, "dense", 0))
    assert pb["rho"] == 0.5 and np.array_equal(pb["V"], 0.5 * np.eye(2)) and np.count_nonzero(pb["H"]) == 8
    assert np.array_equal(pb["Q"], pb["Q"].T) and np.linalg.eigvalsh(pb["Q"]).min() >= 0.05


def _r_dimensional_engine(pb, carry_P):
    """the case as an engine with x in R^r and y ~ C x would run it"""
    r = pb["H"].shape[0]
    cut = dict(pb, A=pb["A"][:r, :r], Q=pb["Q"][:r, :r], P0=pb["P0"][:r, :r], x0=pb["x0"][:r], H=np.eye(r))
    return SC.literal_model(cut, carry_P)


@pytest.mark.parametrize("cs", SC.CASES, ids=SC.IDS)
def test_case_by_the_models_alone(cs):
    pb, ref = SC.reference(cs)
    d, n, r, p = cs["d"], cs["n"], cs["r"], cs["p"]
    assert pb["Y"].shape == (d, n) and pb["C0"].shape == (d, r) and pb["x0"].shape == (p,) and pb["H"].shape == (r, p)
    # (1) finite, V positive definite
    for k, v in ref.items():
        assert np.all(np.isfinite(v)), k
    assert np.linalg.eigvalsh(0.5 * (ref["V"] + ref["V"].T)).min() > 0
    # (2) the kernel's algebra
    alg = SC.device_algebra_model(pb, cs["carry_P"])
    algebra = {k: SC.relerr(alg[k], ref[k]) for k in SC.COMPARED}
    # (3) conditioning: a few ulp on C0 and x0
    pert = SC.literal_model(SC.problem(cs, perturb=(d + n, 4 * 2.0 ** -52)), cs["carry_P"])
    cond = {k: SC.relerr(pert[k], ref[k]) for k in SC.COMPARED}
    # (4) carry_P, (5) H and the p-dimensional state
    other = SC.relerr(SC.literal_model(pb, 1 - cs["carry_P"])["X"], ref["X"])
    flat = SC.relerr(_r_dimensional_engine(pb, cs["carry_P"])["X"], ref["X"][:r])
    print(f"\nssm case {SC.IDS[SC.CASES.index(cs)]}: algebra {algebra}; a few ulp on C0, x0 {cond}; other carry_P {other:.3g}; x in R^r, no H {flat:.3g}")
    assert max(algebra.values()) <= 1e-11, algebra
    assert max(cond.values()) <= 1e-11, cond
    assert other > 1e-2
    assert flat > 1e-2


def test_continuing_a_series_is_the_same_recursion():
    """first_step = 0 in the models: n steps at once against n1 + n2 (with carry_P = 0 the second part predicts from P_prev = 0 throughout)"""
    for carry_P in (1, 0):
        cs = SC.find(33, 7, "dense", carry_P)
        pb, ref = SC.reference(cs)
        n1 = 17
        a = SC.literal_model(dict(pb, Y=pb["Y"][:, :n1]), carry_P)
        b = SC.literal_model(dict(pb, Y=pb["Y"][:, n1:], C0=a["C"], V=a["V"], x0=a["x"], P0=a["P"]), carry_P, first_step=False)
        assert np.array_equal(np.concatenate([a["X"], b["X"]], axis=1), ref["X"]) and np.array_equal(b["P"], ref["P"])


def _expm(M):
    try:
        from scipy.linalg import expm
        return expm(M)
    except ImportError:
        out, term = np.eye(M.shape[0]), np.eye(M.shape[0])
        for k in range(1, 31):
            term = term @ M / k
            out = out + term
        return out


@pytest.mark.parametrize("ell,var,dt,r", [(0.1, 0.1, 1e-3, 1), (0.1, 0.1, 1e-3, 10), (2.0, 3.0, 0.5, 3), (0.05, 1.0, 0.02, 2)])
def test_matern32_state_space_is_the_discretised_sde(ell, var, dt, r):
    A, Q, H = ssm.matern32_state_space(ell, var, dt, r)
    lam = np.sqrt(3.0) / ell
    F = np.array([[0.0, 1.0], [-lam * lam, -2.0 * lam]])
    A2 = _expm(F * dt)
    Pinf = np.diag([var, lam * lam * var])
    assert A.shape == (2 * r, 2 * r) and Q.shape == (2 * r, 2 * r) and H.shape == (r, 2 * r)
    assert SC.relerr(A, np.kron(A2, np.eye(r))) <= 1e-13
    assert SC.relerr(Q, np.kron(Pinf - A2 @ Pinf @ A2.T, np.eye(r))) <= 1e-9      # (the difference cancels: Q11 ~ 7e-7 of 0.1 at the experiment's values)
    assert np.array_equal(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    assert np.array_equal(H, np.hstack([np.eye(r), np.zeros((r, r))]))
    # stationary: Pinf = A Pinf A^T + Q
    Pk = np.kron(Pinf, np.eye(r))
    assert SC.relerr(A @ Pk @ A.T + Q, Pk) <= 1e-13
    with pytest.raises(ValueError):
        ssm.matern32_state_space(0.0, 1.0, 0.1)


def test_argument_checks_need_no_device():
    run = ssm.linear_psmf_batch
    I2, I4, H = np.eye(2), np.eye(4), np.ones((2, 4))
    Y, C0, x0 = np.zeros((3, 8, 6)), np.ones((3, 8, 2)), np.zeros((3, 4))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        run(Y, C0[:2], x0, I2, I4, I4, I4, H, 0.5)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        run(Y, C0, x0, I2, I4, I4, I4, H.T, 0.5)
    with pytest.raises(ValueError, match="V0 has shape"):
        run(Y, C0, x0, np.eye(3), I4, I4, I4, H, 0.5)
    with pytest.raises(ValueError, match="P0 has shape"):
        run(Y, C0, x0, I2, np.zeros((2, 4, 4)), I4, I4, H, 0.5)
    with pytest.raises(ValueError, match="single series"):
        run(Y[0], C0, x0[0], I2, I4, I4, I4, H, 0.5)
    with pytest.raises(ValueError, match="rho must be a scalar"):
        run(Y, C0, x0, I2, I4, I4, I4, H, np.ones(8))
    # the limits and the conditions on Q and rho are the library's own (before it looks for a device)
    for kw, msg in ((dict(d=513), "d <= 512"), (dict(r=17, p=20), "r <= 16"), (dict(p=33), "p <= 32"), (dict(r=4, p=3), "p >= r")):
        d, r, p = kw.get("d", 8), kw.get("r", 2), kw.get("p", 4)
        with pytest.raises(ValueError, match=msg):
            run(np.zeros((d, 6)), np.ones((d, r)), np.zeros(p), np.eye(r), np.eye(p), np.eye(p), np.eye(p), np.ones((r, p)), 0.5)
    Q = np.eye(4)
    Q[0, 1] = 0.1
    with pytest.raises(ValueError, match="Q must be symmetric"):
        run(Y, C0, x0, I2, I4, I4, Q, H, 0.5)
    with pytest.raises(ValueError, match="Q must be positive definite"):
        run(Y, C0, x0, I2, I4, I4, np.diag([1.0, 1.0, 0.0, 1.0]), H, 0.5)
    with pytest.raises(ValueError, match="rho must be finite and >= 0"):
        run(Y, C0, x0, I2, I4, I4, I4, H, -1.0)


def test_the_drop_in_refuses_what_the_engine_does_not_model():
    Y, C = np.zeros((8, 6)), np.ones((8, 2))
    args = lambda R: (2, Y, np.eye(4), np.eye(4), R, np.ones((2, 4)), np.eye(2), np.eye(4), C, None, 8, 6)
    R = 0.1 * np.eye(8)
    R[0, 1] = 0.01
    with pytest.raises(NotImplementedError, match="rho \\* I"):
        ssm.PSMF(*args(R), x0=np.zeros(4))
    with pytest.raises(NotImplementedError, match="rho \\* I"):
        ssm.PSMF(*args(np.diag(np.linspace(0.1, 0.2, 8))), x0=np.zeros(4))
    with pytest.raises(ValueError, match="shape mismatch"):
        ssm.PSMF(3, Y, np.eye(4), np.eye(4), 0.1, np.ones((2, 4)), np.eye(2), np.eye(4), C, None, 8, 6, x0=np.zeros(4))
    assert "PSMF.m:30" in ssm.PSMF.__doc__ and "carry_P=True" in ssm.PSMF.__doc__
