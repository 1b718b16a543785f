"""The cases of the robust (rPSMF) and masked forms of the batched PSMF with linear-Gaussian dynamics and an observation map
(psmf_ssm_run_ex, rpsmf_amd/ssm.py), the problem each one runs and two float64 models of it.  Pure Python:
tests/test_ssm_robust_cases_cpu.py checks the list without a GPU, tests/test_hip_ssm_robust.py runs it on the device.

The recursion is the one of ssm_cases.literal_model with the changes of ExperimentImpute/rPSMF.py:75-135 and
pypsmf/psmf/rpsmf.py:125-172.  Per step, m the 0/1 mask column, M = diag(m), Omega the running product of omega, e zero on unobserved
rows:
    Pbar = A P_prev A^T + Omega Q,  rho_t = Omega rho,  e_i = m_i (y_i - yhat_i)
    S = (M C) P_z (M C)^T + diag(rho_t m) + s I                        (rPSMF.py:92-98: s I, not s M)
    x = xbar + Pbar H^T (MC)^T S^-1 e
    omega = (lambda + e^T S^-1 e) / (lambda + d)                                               rob
    P = beta omega (Pbar - Pbar H^T (MC)^T S^-1 (MC) H Pbar)                                   rob: beta omega; else 1
    eta = (rho_t sum m_i + trace((MC) P_z (MC)^T)) / d,  N = s + eta,  C += e w^T / N
    phi = (lambda + sum_i e_i^2 / (s m_i + eta)) / (lambda + d)                                rob
    V = alpha phi (V - w w^T / N)                                                              rob: alpha phi; else 1
    Omega <- omega Omega;  lambda <- lambda + d unless fixed                                   rob
`literal_model` forms and divides by the d x d S; `device_algebra_model` is the r x r algebra of the kernel:
    G = sum m_i c_i c_i^T, h = sum m_i c_i e_i, kappa = 1 / (rho_t + s), P_z+ = (P_z^-1 + kappa G)^-1, B = P_z^-1 P_z+,
    u = kappa B h, W = kappa sym(B G), e^T S^-1 e = kappa e^T e - kappa^2 h^T P_z+ h, eta = (rho_t sum m_i + <G, P_z>) / d

The problems are those of ssm_cases.problem -- the same eight shapes, each with carry_P 1 and 0 -- with n capped at 60 and a
Student-t draw (3 degrees of freedom) added to 5 % of the entries of Y; each shape runs in five variants:
    rob        robust, lambda0 = 1.8, growing             rob-fix       robust, lambda = 10, fixed
    mask       masked only: 80 % observed, every column at least one row
    rob-mask   robust + masked, growing lambda            rob-fix-mask  robust + masked, fixed lambda
(Not admissible, and not here: the experiment's own 1.5 degrees of freedom for the contamination -- two float64 models then differ
by 1e-8 --, and n = 150 with a mask and a fixed lambda -- 2e-4, Omega wanders over five decades.)"""

from functools import lru_cache

import numpy as np

import ssm_cases as SC

N_CAP = 60
# shorter still where the 60 steps miss the admission bounds of tests/test_ssm_robust_cases_cpu.py (the Matern model with carry_P = 0 has
# Q11 ~ 7e-7: P_z is nearly singular, and the error of either float64 model grows with the length of the series)
N_OF = {(20, "matern"): 40, (96, "matern"): 40}
# name -> (robust, lambda0, fixed_lambda, masked)
VARIANTS = {
    "rob": (True, 1.8, False, False),
    "rob-fix": (True, 10.0, True, False),
    "mask": (False, None, False, True),
    "rob-mask": (True, 1.8, False, True),
    "rob-fix-mask": (True, 10.0, True, True),
}
CASES = [dict(d=d, n=min(n, N_OF.get((d, k), N_CAP)), r=r, p=p, kind=k, carry_P=c, variant=v, robust=VARIANTS[v][0], lambda0=VARIANTS[v][1],
              fixed_lambda=VARIANTS[v][2], masked=VARIANTS[v][3])
         for v in VARIANTS for d, n, r, p, k in SC.SHAPES for c in (1, 0)]
IDS = [f"{c['d']}x{c['n']}r{c['r']}p{c['p']}-{c['kind']}-carry{c['carry_P']}-{c['variant']}" for c in CASES]
COMPARED = SC.COMPARED + ("omega", "phi", "robust_state")
relerr = SC.relerr


def find(d, r, kind, carry_P, variant):
    return next(c for c in CASES if (c["d"], c["r"], c["kind"], c["carry_P"], c["variant"]) == (d, r, kind, carry_P, variant))


def problem(cs, perturb=None, seed=0):
    """ssm_cases.problem of the case's shape, Y contaminated, plus `mask` (d, n) uint8 (all ones for a variant without one)"""
    d, n, r, p = cs["d"], cs["n"], cs["r"], cs["p"]
    pb = SC.problem(dict(d=d, n=n, r=r, p=p, kind=cs["kind"], carry_P=cs["carry_P"]), perturb=perturb, seed=seed)
    rng = np.random.default_rng(9300 + 7 * d + 3 * r + p + 1000 * seed)
    hit = rng.uniform(size=(d, n)) < 0.05
    pb["Y"] = pb["Y"] + np.where(hit, rng.standard_t(3, size=(d, n)), 0.0)
    mask = rng.uniform(size=(d, n)) < 0.8
    keep = rng.integers(0, d, size=n)
    mask[keep, np.arange(n)] = True           # every column keeps at least one row
    pb["mask"] = mask.astype(np.uint8) if cs["masked"] else np.ones((d, n), dtype=np.uint8)
    return pb


def _out(X, C, V, P, x, Yp, sc, lam, Om):
    return dict(X=X, C=C, V=V, P=P, x=x.copy(), Ypred=Yp, scalars=sc[:, :2].copy(), omega=sc[:, 2].copy(), phi=sc[:, 3].copy(),
                robust_state=np.array([lam, Om]))


def _start(pb, robust, lambda0, first_step, robust_state):
    if not robust:
        return 0.0, 1.0
    if first_step:
        return float(lambda0), 1.0
    return float(robust_state[0]), float(robust_state[1])


def literal_model(pb, carry_P, robust=False, lambda0=None, fixed_lambda=False, alpha=1.0, beta=1.0, first_step=True, robust_state=None,
                  mask=None):
    """rPSMF.py:75-135 line for line on the recursion of ssm_cases.literal_model (S is d x d).  `mask` None: pb["mask"]"""
    Y, A, Q, H, rho = pb["Y"], pb["A"], pb["Q"], pb["H"], pb["rho"]
    M = (pb["mask"] if mask is None else mask).astype(float)
    C, V, x, P0 = pb["C0"].copy(), pb["V"].copy(), pb["x0"].copy(), pb["P0"]
    d, n = Y.shape
    p = A.shape[0]
    X, Yp, sc = np.zeros((p, n)), np.zeros((d, n)), np.zeros((n, 4))
    P = P0.copy()
    lam, Om = _start(pb, robust, lambda0, first_step, robust_state)
    for t in range(n):
        m = M[:, t]
        Cm = m[:, None] * C
        Pprev = P if (carry_P or (first_step and t == 0)) else np.zeros((p, p))
        xb = A @ x
        Pb = A @ Pprev @ A.T + Om * Q
        z = H @ xb
        Yp[:, t] = C @ H @ xb
        Rm = np.diag(m * (Om * rho))
        s = z @ V @ z
        PHC = Pb @ H.T @ Cm.T
        CPC = Cm @ (H @ Pb @ H.T) @ Cm.T
        S = CPC + np.diag(m * (Om * rho) + s)                         # Rbar = Rm + s * Id
        e = np.where(m > 0, np.where(m > 0, Y[:, t], 0.0) - Cm @ H @ xb, 0.0)
        sol = np.linalg.solve(S.T, np.column_stack([PHC.T, e]))       # as ssm_cases.literal_model: K = Pb H' (MC)' / S
        K, Se = sol[:, :-1].T, sol[:, -1]                                 # (e' S^-1 e = e' S^-T e)
        x = xb + K @ e
        omega = (lam + e @ Se) / (lam + d) if robust else 1.0
        P = (beta * omega if robust else 1.0) * (Pb - K @ Cm @ H @ Pb)
        eta = np.trace(Rm + CPC) / d
        N = xb @ H.T @ V @ H @ xb + eta
        w = xb @ H.T @ V
        Cnew = C + np.outer(e, w) / N
        U = s * m + eta
        phi = (lam + np.sum(e * e / U)) / (lam + d) if robust else 1.0
        V = (alpha * phi if robust else 1.0) * (V - (V @ H @ np.outer(xb, xb) @ H.T @ V) / N)
        C = Cnew
        X[:, t] = x
        sc[t] = N - eta, eta, omega, phi
        if robust:
            Om = omega * Om
            if not fixed_lambda:
                lam = lam + d
    return _out(X, C, V, P, x, Yp, sc, lam, Om)


def device_algebra_model(pb, carry_P, robust=False, lambda0=None, fixed_lambda=False, alpha=1.0, beta=1.0, first_step=True,
                         robust_state=None):
    """the r x r algebra of psmf_ssm_kernel<robust, masked> (rpsmf_amd/csrc/psmf_ssm.hip), in numpy: no d x d matrix"""
    Y, A, Q, H, rho = pb["Y"], pb["A"], pb["Q"], pb["H"], pb["rho"]
    M = pb["mask"].astype(float)
    C, V, x, P = pb["C0"].copy(), pb["V"].copy(), pb["x0"].copy(), pb["P0"].copy()
    d, n = Y.shape
    p = A.shape[0]
    X, Yp, sc = np.zeros((p, n)), np.zeros((d, n)), np.zeros((n, 4))
    lam, Om = _start(pb, robust, lambda0, first_step, robust_state)
    for t in range(n):
        m = M[:, t]
        xb = A @ x
        Pb = (A @ P) @ A.T + Om * Q if (carry_P or (first_step and t == 0)) else Om * Q
        rho_t = Om * rho
        z = H @ xb
        PH = Pb @ H.T
        Pz = H @ PH
        Pz = 0.5 * (Pz + Pz.T)
        w = V @ z
        s = z @ w
        yh = C @ z
        e = np.where(m > 0, np.where(m > 0, Y[:, t], 0.0) - yh, 0.0)
        Cm = m[:, None] * C
        G, h = Cm.T @ Cm, Cm.T @ e
        kap = 1.0 / (rho_t + s)
        Pzi = np.linalg.inv(Pz)
        Pp = np.linalg.inv(Pzi + kap * G)
        B = Pzi @ Pp
        u = kap * (B @ h)
        W = kap * (B @ G)
        W = 0.5 * (W + W.T)
        x = xb + PH @ u
        ee = e @ e
        omega = (lam + kap * (ee - kap * (h @ Pp @ h))) / (lam + d) if robust else 1.0
        P = (beta * omega if robust else 1.0) * (Pb - (PH @ W) @ PH.T)
        eta = (np.sum(G * Pz) + rho_t * m.sum()) / d
        N = s + eta
        C = C + np.outer(e, w) / N
        phi = (lam + ee / N) / (lam + d) if robust else 1.0
        V = (alpha * phi if robust else 1.0) * (V - np.outer(w, w) / N)
        X[:, t], Yp[:, t], sc[t] = x, yh, (s, eta, omega, phi)
        if robust:
            Om = omega * Om
            if not fixed_lambda:
                lam = lam + d
    return _out(X, C, V, P, x, Yp, sc, lam, Om)


def model_kw(cs):
    return dict(robust=cs["robust"], lambda0=cs["lambda0"], fixed_lambda=cs["fixed_lambda"])


@lru_cache(maxsize=None)
def _cached(i, seed):
    pb = problem(CASES[i], seed=seed)
    return pb, literal_model(pb, CASES[i]["carry_P"], **model_kw(CASES[i]))


def reference(cs, seed=0):
    """(problem, literal_model result) of a case and replica seed, computed once and shared: do not modify either"""
    return _cached(CASES.index(cs), seed)
