"""The cases of the batched PSMF with linear-Gaussian dynamics and an observation map (psmf_ssm_run, rpsmf_amd/ssm.py), the problem each
one runs and two float64 models of it.  Pure Python: tests/test_ssm_cases_cpu.py checks the list without a GPU,
tests/test_hip_ssm.py runs it on the device.

`literal_model` is the recursion of ExperimentChange/PSMF.m:6-45 line for line, the d x d matrix S formed and divided by (with
S = C P_z C^T + (rho + s) I, R = rho I); `device_algebra_model` is the r x r algebra the kernel implements (two symmetric inversions):
    G = C^T C, h = C^T e, kappa = 1 / (rho + s)
    P_z+ = (P_z^-1 + kappa G)^-1,  B = P_z^-1 P_z+,  u = kappa B h,  W = kappa sym(B G)
    x = xbar + Pbar H^T u,  P = Pbar - Pbar H^T W H Pbar,  eta = <G, P_z> / d + rho
(B = I - kappa G P_z+ written as a product: the textbook W = kappa G - kappa^2 G P_z+ G cancels 1e3-fold where rho is small against
C P_z C^T -- the Matern cases with carry_P = 1 -- and misses the 1e-11 of the CPU test by two orders.)
Both take carry_P: 1 is the textbook recursion, 0 is PSMF.m:30 as written (P_prev = P0 at the first step of a series, 0 afterwards).

The cases are the smallest shapes that reach each path of the kernel; each runs with carry_P 1 and 0.
    series   min(4, r) sinusoids sin(0.07 (j + 1) t + j) mixed by a normal d x k matrix, plus 0.3 N(0, 1); the first sinusoid is scaled
             by 2.5 from n / 2 on (the change of regime the experiment looks for).  C0 standard normal, x0 = 0.3 N(0, 1)
    matern   A, Q, H of matern32_state_space(0.1, 0.1, 1e-3, r) (p = 2 r), rho = 1e-3, V = I, P0 = I   (ExperimentChange/main.m)
    dense    A = 0.9 I + 0.05 B / sqrt(p), Q = 0.05 I + 0.02 L L^T / p, H = N(0, 1) / sqrt(p), rho = 0.5, V = 0.5 I, P0 = I"""

from functools import lru_cache

import numpy as np

from netlib import relerr  # noqa: F401  (the tests take it from here)
from rpsmf_amd.ssm import matern32_state_space

# (d, n, r, p, kind)
SHAPES = [
    (5, 40, 2, 4, "matern"),        # smallest; Q11 ~ 7e-7 makes P_z nearly singular when carry_P = 0
    (5, 40, 2, 4, "dense"),         # dense A and H, full Q
    (33, 50, 7, 7, "dense"),        # p = r; odd r; d not a multiple of 4 or 16
    (20, 150, 10, 20, "matern"),    # ExperimentChange's geometry
    (200, 40, 12, 24, "matern"),    # several row groups per wave
    (96, 60, 16, 32, "matern"),     # both upper limits
    (96, 60, 16, 32, "dense"),
    (512, 30, 3, 7, "dense"),       # the d limit; p neither r nor 2 r
]
CASES = [dict(d=d, n=n, r=r, p=p, kind=k, carry_P=c) for d, n, r, p, k in SHAPES for c in (1, 0)]
IDS = [f"{c['d']}x{c['n']}r{c['r']}p{c['p']}-{c['kind']}-carry{c['carry_P']}" for c in CASES]
COMPARED = ("X", "C", "V", "P", "x", "Ypred", "scalars")


def find(d, r, kind, carry_P):
    return next(c for c in CASES if (c["d"], c["r"], c["kind"], c["carry_P"]) == (d, r, kind, carry_P))


def problem(cs, perturb=None, seed=0):
    """dict(Y (d, n), C0 (d, r), x0 (p,), V, P0, A, Q, H, rho) of a case.  `seed` picks another replica (Y, C0, x0; the model is the
    case's).  `perturb` = (seed, eps): C0 and x0 times (1 + eps u), u uniform in [-1, 1]."""
    d, n, r, p = cs["d"], cs["n"], cs["r"], cs["p"]
    mrng = np.random.default_rng(9100 + 7 * d + 3 * r + p)
    if cs["kind"] == "matern":
        assert p == 2 * r
        A, Q, H = matern32_state_space(0.1, 0.1, 1e-3, r)
        rho, V = 1e-3, np.eye(r)
    else:
        B, L = mrng.standard_normal((p, p)), mrng.standard_normal((p, p))
        A = 0.9 * np.eye(p) + 0.05 * B / np.sqrt(p)
        Q = 0.05 * np.eye(p) + 0.02 * (L @ L.T) / p
        Q = 0.5 * (Q + Q.T)
        H = mrng.standard_normal((r, p)) / np.sqrt(p)
        rho, V = 0.5, 0.5 * np.eye(r)
    rng = np.random.default_rng(9200 + 7 * d + 3 * r + p + 1000 * seed)
    k = min(4, r)
    t = np.arange(n, dtype=float)
    S = np.stack([np.sin(0.07 * (j + 1) * t + j) for j in range(k)])
    S[0, n // 2:] *= 2.5
    Y = rng.standard_normal((d, k)) @ S + 0.3 * rng.standard_normal((d, n))
    C0 = rng.standard_normal((d, r))
    x0 = 0.3 * rng.standard_normal(p)
    if perturb is not None:
        prng = np.random.default_rng(perturb[0])
        C0 = C0 * (1.0 + perturb[1] * prng.uniform(-1, 1, C0.shape))
        x0 = x0 * (1.0 + perturb[1] * prng.uniform(-1, 1, x0.shape))
    return dict(Y=Y, C0=C0, x0=x0, V=V, P0=np.eye(p), A=A, Q=Q, H=H, rho=rho)


def _out(X, C, V, P, x, Yp, sc):
    return dict(X=X, C=C, V=V, P=P, x=x.copy(), Ypred=Yp, scalars=sc)


def literal_model(pb, carry_P, first_step=True, H=None):
    """ExperimentChange/PSMF.m:6-45 line for line (S is d x d).  -> dict(X (p, n), C, V, P, x, Ypred (d, n), scalars (n, 2))"""
    Y, A, Q, rho = pb["Y"], pb["A"], pb["Q"], pb["rho"]
    H = pb["H"] if H is None else H
    C, V, x, P0 = pb["C0"].copy(), pb["V"].copy(), pb["x0"].copy(), pb["P0"]
    d, n = Y.shape
    p = A.shape[0]
    X, Yp, sc = np.zeros((p, n)), np.zeros((d, n)), np.zeros((n, 2))
    P = P0.copy()
    for t in range(n):
        if carry_P or (first_step and t == 0):
            Pprev = P
        else:
            Pprev = np.zeros((p, p))
        Xp = A @ x
        PP = A @ Pprev @ A.T + Q
        barR = rho + (H @ Xp) @ V @ (H @ Xp)
        S = C @ (H @ PP @ H.T) @ C.T + barR * np.eye(d)
        K = np.linalg.solve(S.T, (PP @ H.T @ C.T).T).T          # PP * H' * C' / S
        e = Y[:, t] - C @ H @ Xp
        x = Xp + K @ e
        P = PP - K @ C @ H @ PP
        eta = np.trace(C @ (H @ PP @ H.T) @ C.T + rho * np.eye(d)) / d
        s = Xp @ H.T @ V @ H @ Xp
        Nt = s + eta
        Yp[:, t] = C @ H @ Xp
        sc[t] = s, eta
        Cn = C + np.outer(e, Xp @ H.T @ V) / Nt
        V = V - (V @ H @ np.outer(Xp, Xp) @ H.T @ V) / Nt
        C = Cn
        X[:, t] = x
    return _out(X, C, V, P, x, Yp, sc)


def device_algebra_model(pb, carry_P, first_step=True):
    """the r x r algebra of psmf_ssm_kernel (rpsmf_amd/csrc/psmf_ssm.hip), in numpy: no d x d matrix"""
    Y, A, Q, H, rho = pb["Y"], pb["A"], pb["Q"], pb["H"], pb["rho"]
    C, V, x, P = pb["C0"].copy(), pb["V"].copy(), pb["x0"].copy(), pb["P0"].copy()
    d, n = Y.shape
    p = A.shape[0]
    X, Yp, sc = np.zeros((p, n)), np.zeros((d, n)), np.zeros((n, 2))
    for t in range(n):
        xb = A @ x
        Pb = (A @ P) @ A.T + Q if (carry_P or (first_step and t == 0)) else Q.copy()
        z = H @ xb
        PH = Pb @ H.T
        Pz = H @ PH
        Pz = 0.5 * (Pz + Pz.T)
        w = V @ z
        s = z @ w
        yh = C @ z
        e = Y[:, t] - yh
        G, h = C.T @ C, C.T @ e
        kap = 1.0 / (rho + s)
        Pzi = np.linalg.inv(Pz)
        Pp = np.linalg.inv(Pzi + kap * G)
        B = Pzi @ Pp
        u = kap * (B @ h)
        W = kap * (B @ G)
        W = 0.5 * (W + W.T)
        x = xb + PH @ u
        P = Pb - (PH @ W) @ PH.T
        eta = np.sum(G * Pz) / d + rho
        N = s + eta
        C = C + np.outer(e, w) / N
        V = V - np.outer(w, w) / N
        X[:, t], Yp[:, t], sc[t] = x, yh, (s, eta)
    return _out(X, C, V, P, x, Yp, sc)


@lru_cache(maxsize=None)
def _cached(i, seed):
    pb = problem(CASES[i], seed=seed)
    return pb, literal_model(pb, CASES[i]["carry_P"])


def reference(cs, seed=0):
    """(problem, literal_model result) of a case and replica seed, computed once and shared: do not modify either"""
    return _cached(CASES.index(cs), seed)
