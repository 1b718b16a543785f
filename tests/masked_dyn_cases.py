"""The cases of the masked per-step engine with built-in dynamics (cfg.masked = 4, PSMF_MASKED_DYNAMICS, with dyn_kind = cos-phase, ScaledWalk, Sinusoid,
FourierBasis; theta learned between epochs or inside the time loop), the problem each one runs and the float64 model of it.  Pure
Python: tests/test_masked_dyn_cases_cpu.py checks the model and the conditioning of every case without a GPU,
tests/test_hip_masked_dynamics.py runs the same list on the device.

The model.  State recursion: oracle.psmf_oracle.lowrank_step(st, y, k, mode, dyn, mask=m, want_grad=False) -- mu_bar = f_theta(mu, k),
P_bar = F P F^T + Q, y_hat stored unmasked, e = m o (y - y_hat), eta divided by d, kappa_i = m_i / (rho + s), the robust scalars
formed with d.  theta gradient: that of the reference's masked incremental likelihood (pypsmf/psmf/psmf.py:264-270,
rpsmf.py:196-200: ll = 1/2 sum_i log(s m_i + eta) + 1/2 e^T e / (s + eta), the Gaussian form for the robust class too),

    g_f = n_obs w / N - h / N - ee w / N^2,      w = V mu_bar, h = C^T e, N = s + eta, n_obs = sum_i m_i of the step
    gradsum += J_theta^T g_f

(`masked_gf`; `reference_ll` restates ll for the finite-difference check).  J_theta and F are the closed forms of
rpsmf_amd/nonlinearities.py, which the CPU test holds against complex-step derivatives of the same callables.

The shapes are the smallest that reach each path of the serial stage (psmf_kernels.hip: serial_body):

    d    r   T   covers
    40   3  30   RPAD 8, cos-phase: the persistent kernel's masked instance (and the launched form under PSMF_STEP_PERSISTENT=0)
    300 10  40   RPAD 16, ScaledWalk(bias), Sinusoid
    530 20  40   RPAD 32, FourierBasis N = 2 (1 760 parameters: more than the 1 024 threads of the stage), two 16-column tiles per wave
                 of the look-ahead Gram, a last slab of two rows
    300 40  24   RPAD 64, the wide serial stage, Sinusoid(scaled=False)

Each with PSMF and rPSMF (lambda0 = 1.8), float64 and float32 storage; two epochs with Adam between them (one shape: SGD), or one pass
with the optimiser inside the loop every `update_every` steps (Adam on two shapes, SGD on one).  About 60 % of the entries are
observed; step EMPTY_STEP has no observation at all (n_obs = 0: it must contribute exactly zero to the gradient) and is never the
only step of an optimiser window."""

from functools import lru_cache

import numpy as np

from netlib import f32_round, relerr  # noqa: F401  (the tests take relerr from here)
from oracle import psmf_oracle as O
from rpsmf_amd import nonlinearities as NL

LAMBDA0 = 1.8
EMPTY_STEP = 7            # 1-based step without any observation
EPOCHS = 2
LR_EPOCH, LR_LOOP, LR_SGD = 1e-3, 2e-3, 1e-7          # (plain SGD steps by lr x the raw gradient sum, which grows with d)

# (d, r, T, name, constructor)
SHAPES = [
    (40, 3, 30, "cos_phase", lambda r: NL.CosPhase(r)),
    (300, 10, 40, "scaled_walk_bias", lambda r: NL.ScaledWalk(r, bias=True)),
    (300, 10, 40, "sinusoid", lambda r: NL.Sinusoid(r)),
    (530, 20, 40, "fourier2", lambda r: NL.FourierBasis(r, N=2)),
    (300, 40, 24, "sinusoid_unscaled", lambda r: NL.Sinusoid(r, scaled=False)),
]
# how theta is learned: (name of the dynamics, optimiser, update_every) -- update_every = 0: between the epochs
LEARNING = [(name, "adam", 0) for _, _, _, name, _ in SHAPES if name != "scaled_walk_bias"] + [("scaled_walk_bias", "sgd", 0)] + [
    ("cos_phase", "adam", 2), ("sinusoid", "adam", 3), ("sinusoid_unscaled", "sgd", 2)]

CASES = []
for _d, _r, _T, _name, _make in SHAPES:
    for _n, _opt, _ue in LEARNING:
        if _n != _name:
            continue
        for _robust in (False, True):
            for _storage in ("f64", "f32"):
                CASES.append(dict(d=_d, r=_r, T=_T, dyn=_name, make=_make, optim=_opt, update_every=_ue, robust=_robust, storage=_storage,
                                  masked=True, seed=0))
IDS = [f"{c['d']}r{c['r']}-{c['dyn']}-{'rPSMF' if c['robust'] else 'PSMF'}-{c['optim']}{c['update_every'] or 'epoch'}-{c['storage']}" for c in CASES]


def find(dyn, robust=False, storage="f64", update_every=0):
    return next(c for c in CASES if (c["dyn"], c["robust"], c["storage"], c["update_every"]) == (dyn, robust, storage, update_every))


class ClosedFormDyn(O.Dynamics):
    """a nonlinearity of rpsmf_amd/nonlinearities.py behind the oracle's Dynamics interface, with its closed-form derivatives"""

    def __init__(self, nl):
        self.nl = nl
        self.n_theta = nl.n_params

    def f(self, theta, x, t):
        return np.asarray(self.nl(np.asarray(theta).reshape(-1, 1), np.asarray(x).reshape(-1, 1), t), dtype=float).reshape(-1)

    def jac_x(self, theta, x, t):
        return np.asarray(self.nl.jac_x(theta, x, t), dtype=float)

    def jac_theta(self, theta, x, t):
        return np.asarray(self.nl.jac_theta(theta, x, t), dtype=float)


def theta_for(nl, rng, r):
    """theta in the regime the experiments use (beijing_psmf.py:117: 0.1 * rand), matrices near a contraction"""
    th = 0.1 * rng.random(nl.n_params)
    if isinstance(nl, NL.ScaledWalk) or getattr(nl, "scaled", False):
        th[:r * r] = (0.8 * np.eye(r) + 0.05 * rng.standard_normal((r, r))).reshape(-1)
    if isinstance(nl, NL.FourierBasis):
        for t in range(2 * nl.N):
            th[t * r * r:(t + 1) * r * r] = (0.5 * np.eye(r) + 0.05 * rng.standard_normal((r, r))).reshape(-1) / nl.N
    return th


def problem(cs, perturb=None):
    """dict(Y (T, d), M (T, d) 0/1, C0, V0, P0, Q, mu0, theta0, nl) of a case.  `perturb` = (seed, eps): C0 and mu0 times
    (1 + eps u), u uniform in [-1, 1]."""
    d, r, T = cs["d"], cs["r"], cs["T"]
    rng = np.random.default_rng([8100 + d + r, cs["seed"], sum(map(ord, cs["dyn"]))])
    Ct = rng.standard_normal((d, r))
    x = rng.standard_normal(r)
    Y = np.empty((T, d))
    for t in range(T):                                   # a seasonal latent path, heavy-tailed noise for the robust filter
        x = 0.9 * np.sin(x + 0.3) + 0.1 * rng.standard_normal(r)
        Y[t] = Ct @ x + 0.3 * (rng.standard_t(3.0, d) if cs["robust"] else rng.standard_normal(d))
    M = (rng.random((T, d)) > 0.4).astype(np.uint8)
    M[:, 3] = 0                                          # a row that is never observed
    M[EMPTY_STEP - 1] = 0                                # a step without any observation
    C0 = 0.1 * rng.standard_normal((d, r))
    mu0 = 0.2 * rng.standard_normal(r)
    nl = cs["make"](r)
    theta0 = theta_for(nl, rng, r)
    if cs["storage"] == "f32":
        Y, C0 = f32_round(Y), f32_round(C0)
    if perturb is not None:
        prng = np.random.default_rng(perturb[0])
        C0 = C0 * (1.0 + perturb[1] * prng.uniform(-1, 1, C0.shape))
        mu0 = mu0 * (1.0 + perturb[1] * prng.uniform(-1, 1, mu0.shape))
    return dict(Y=Y, M=M, C0=C0, V0=0.1 * np.eye(r), P0=np.eye(r), Q=0.1 * np.eye(r), mu0=mu0, theta0=theta0, nl=nl, rho=1.0)


def masked_gf(w, h, ee, N, n_obs):
    """d ll / d mu_bar of the masked incremental likelihood (module docstring)"""
    return n_obs * w / N - h / N - ee * w / N ** 2


def reference_ll(C, V, Pbar, mu_bar, y, m, rho):
    """the reference's masked incremental likelihood (pypsmf/psmf/psmf.py:264-270, rpsmf.py:196-200: U = s diag(m) + eta I,
    ll = 1/2 tr log U + 1/2 diff^T U^-1 diff, diff = m o (y - C mu_bar)) restated as a function of mu_bar, eta held at the step's
    value: 1/2 sum_i log(s m_i + eta) + 1/2 e^T e / (s + eta), s = mu_bar^T V mu_bar (e_i = 0 wherever m_i = 0).  The terms log(eta)
    of the rows with m_i = 0 do not depend on mu_bar and are left out: at a step without any observation eta = 0 and they are -inf.
    Returns (ll, eta)."""
    d = C.shape[0]
    G = (C * m[:, None]).T @ C
    eta = (rho * float(m.sum()) + float(np.sum(G * Pbar))) / d

    def ll(mb):
        s = float(mb @ V @ mb)
        e = m * (y - C @ mb)
        return 0.5 * float(m.sum()) * np.log(s + eta) + 0.5 * float(e @ e) / (s + eta)

    return ll, eta


def model_step(st, y, k, mode, dyn, m, count=None):
    """one masked step with dynamics: lowrank_step(..., mask=m, want_grad=False) plus the masked gradient.  `count`: what stands
    in for n_obs (None: sum m; the CPU test passes d to show that the two differ)."""
    new, info = O.lowrank_step(st, y, k, mode, dyn, mask=m, want_grad=False)
    if dyn.n_theta > 0:
        theta = st.theta
        mf = np.asarray(m, dtype=float)
        w = st.V @ dyn.f(theta, st.mu, k)
        gf = masked_gf(w, info.h, info.ee, info.N, float(mf.sum()) if count is None else float(count))
        g = dyn.jac_theta(theta, st.mu, k).T @ gf
        new.gradsum = g if st.gradsum is None else st.gradsum + g
    return new, info


def run_model(cs, pb, count=None, keep=()):
    """The whole case: EPOCHS passes with the optimiser between them (update_every = 0) or one pass with it inside the loop.
    Returns dict(C, V, P, mu, X (T, r) mean history, yp (T, d), gradsum, theta, pred (3, d) roll-out, windows = [the gradient sum
    that entered each optimiser step], records = [(gradsum, theta after the update) per epoch], snap = {k: dict(gradsum, theta, mu, C)
    after step k of the last pass, for k in `keep`})."""
    d, r, T = cs["d"], cs["r"], cs["T"]
    nl = pb["nl"]
    dyn = ClosedFormDyn(nl)
    mode = O.Mode(robust=cs["robust"])
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=pb["rho"], lam=LAMBDA0,
                 theta=pb["theta0"].copy(), gradsum=np.zeros(nl.n_params))
    am = av = np.zeros(nl.n_params)
    ue = cs["update_every"]
    X, Yp = np.empty((T, r)), np.empty((T, d))
    records, windows, snap = [], [], {}
    for ep in range(1, (1 if ue else EPOCHS) + 1):
        st.gradsum = np.zeros(nl.n_params)
        if cs["robust"]:                       # rpsmf.py:116-131: Q, R, lambda restart every epoch; C, V, P and the mean carry over
            st.Q, st.rho, st.lam = pb["Q"].copy(), pb["rho"], LAMBDA0
        for k in range(1, T + 1):
            st, info = model_step(st, pb["Y"][k - 1], k, mode, dyn, pb["M"][k - 1], count=count)
            X[k - 1], Yp[k - 1] = st.mu, info.y_pred
            if ue and k % ue == 0:
                windows.append(st.gradsum.copy())
                if cs["optim"] == "adam":
                    st.theta, am, av = O.adam_update(st.theta, st.gradsum, am, av, k, lr=LR_LOOP)
                else:
                    st.theta = O.sgd_update(st.theta, st.gradsum, lr=LR_SGD)
                st.gradsum = np.zeros(nl.n_params)
            if k in keep:
                snap[k] = dict(gradsum=st.gradsum.copy(), theta=st.theta.copy(), mu=st.mu.copy(), C=st.C.copy())
        if not ue:
            gs = st.gradsum.copy()
            windows.append(gs)
            if cs["optim"] == "adam":
                st.theta, am, av = O.adam_update(st.theta, gs, am, av, ep, lr=LR_EPOCH)
            else:
                st.theta = O.sgd_update(st.theta, gs, lr=LR_SGD)
            records.append((gs, st.theta.copy()))
    return dict(C=st.C, V=st.V, P=st.P, mu=st.mu, X=X.copy(), yp=Yp.copy(), gradsum=st.gradsum if ue else records[-1][0], theta=st.theta,
                windows=windows, records=records, snap=snap, pred=O.predict_rollout(st.C, st.mu, st.theta, dyn, T, 3))


@lru_cache(maxsize=None)
def _cached(i):
    pb = problem(CASES[i])
    return pb, run_model(CASES[i], pb)


def reference(cs):
    """(problem, model result) of a case, computed once and shared by the tests that need it: do not modify either"""
    return _cached(CASES.index(cs))


STATE_KEYS = ("C", "V", "P", "X", "yp")
