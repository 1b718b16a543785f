"""The cases of the batched Bayesian online change-point detection (psmf_bocpd_run, rpsmf_amd/changepoint.py), the series each one
runs and two float64 models of the detector.  Pure Python: tests/test_bocpd_cases_cpu.py checks the list without a GPU,
tests/test_hip_bocpd.py runs it on the device.

Both models follow the five steps of rpsmf_amd/changepoint.py's docstring, hypotheses indexed by age:
    literal_model   the scatter matrices themselves, c = inv(2 (kappa + 1) Sigma / (nu kappa)) and det(c) per hypothesis and step, and
                    the recursion on R in the linear domain (so a step at which every p_a underflows divides 0 by 0)
    stable_model    the Cholesky factor L of Sigma per hypothesis: L z = delta by forward substitution, delta^T c delta = s |z|^2 with
                    s = nu kappa / (2 (kappa + 1)), log det c = dim log s - 2 sum log L_jj, a rank-one update of L with
                    sqrt(kappa / (2 (kappa + 1))) delta, and log R with a log-sum-exp per column
They share the heuristic and nothing of the algebra.  extended_model is stable_model in np.longdouble (80-bit), every constant formed in
that type and the lgamma difference from mpmath: the reference of tests/bocpd_net_cases.py and tests/test_hip_bocpd_edges.py, which
leave the ranges in which two float64 formulations agree to 1e-11.  Each returns dict(logpred (T, T) [t][age], NaN where not live; R (T + 1, T + 1)
[t][age]; R_last; map_run (T,); changepoints (list); discarded (list: hypotheses dropped by each truncation); declared_at (list: the 0-based step of each declaration)).

A case is a batch of three replicas (seeds 0, 1, 2 of the case's generator), but `many`, which has 300.
    shift   N(base, 1) samples (base = 0 unless given); every channel moves by +shift, then back, ... at the steps of `at`.  At dim 20
            and 32 the prior (nu0 = dim, Sigma0 = I) explains N(0, 1) data better than any learned hypothesis and the MAP run length
            stays at 2: the run only grows, and can only drop, when the segments' means lie away from the prior's 0
    var     N(0, 1) samples; every channel is scaled by `scale` from the step of `at` on
    none    N(0, 1) samples
    outlier as shift, with the LAST sample at 1e100 in every channel: every p_a of that step is exactly 0 in float64 (log p_a < -1300),
            and no hypothesis that absorbed it is ever evaluated, so the two models still agree on log p"""

import math
from functools import lru_cache

import numpy as np

DEFAULTS = dict(lam=200.0, kappa0=1.0, nu0=None, sigma0=1.0, drop=10, settle=10, confirm=10)

CASES = [
    dict(name="dim1-shift", dim=1, T=60, kind="shift", at=(30,), shift=6.0, lam=20.0),
    dict(name="dim3-shift", dim=3, T=60, kind="shift", at=(30,), shift=4.0, lam=20.0),
    dict(name="dim3-two", dim=3, T=128, kind="shift", at=(40, 85), shift=4.0, lam=20.0),
    dict(name="dim3-var", dim=3, T=90, kind="var", at=(45,), scale=6.0, lam=20.0),
    dict(name="dim20-none", dim=20, T=90, kind="none"),
    dict(name="dim20-shift", dim=20, T=64, kind="shift", at=(30,), base=2.0, shift=-4.0, lam=20.0),
    dict(name="dim32-shift", dim=32, T=70, kind="shift", at=(35,), base=3.0, shift=-6.0, lam=20.0, sigma0=2.0, kappa0=0.5, nu0=33.5),
    dict(name="dim3-consts", dim=3, T=48, kind="shift", at=(9,), shift=4.0, lam=20.0, drop=4, settle=5, confirm=3),
    dict(name="dim3-outlier", dim=3, T=50, kind="outlier", at=(25,), shift=4.0, lam=20.0),
    dict(name="dim2-long", dim=2, T=300, kind="shift", at=(100, 210), shift=5.0, lam=50.0),
    dict(name="many", dim=3, T=40, kind="shift", at=(18,), shift=4.0, lam=20.0, batch=300),
]
IDS = [c["name"] for c in CASES]
OUTLIER = 1e100


def find(name):
    return next(c for c in CASES if c["name"] == name)


def params(cs):
    """the detector's arguments of a case (mvbocpd_batch's keywords)"""
    p = {k: cs.get(k, v) for k, v in DEFAULTS.items()}
    p["nu0"] = float(cs["dim"]) if p["nu0"] is None else p["nu0"]
    return p


def series(cs, seed=0):
    """X (dim, T) of a case's replica `seed`"""
    dim, T = cs["dim"], cs["T"]
    rng = np.random.default_rng([7300 + 11 * dim + T, seed])
    X = rng.standard_normal((dim, T)) + cs.get("base", 0.0)
    if cs["kind"] in ("shift", "outlier"):
        for i, at in enumerate(cs["at"]):
            X[:, at:] += cs["shift"] if i % 2 == 0 else -cs["shift"]
    elif cs["kind"] == "var":
        X[:, cs["at"][0]:] *= cs["scale"]
    if cs["kind"] == "outlier":
        X[:, -1] = OUTLIER
    return X


def batch(cs):
    return np.stack([series(cs, s) for s in range(cs.get("batch", 3))])


def _lgam(nu, dim):
    return np.array([math.lgamma(0.5 * (v + dim)) - math.lgamma(0.5 * v) for v in nu])


def _ext(v):
    """an mpmath number as np.longdouble: its float64 rounding plus the float64 rounding of what that leaves (106 bits, then rounded to 64)"""
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - hi))


@lru_cache(maxsize=None)
def _lgam_ext(nu0, dim, n):
    """lgamma((nu + dim) / 2) - lgamma(nu / 2) for nu = nu0 .. nu0 + n - 1, from mpmath at 120 bits, as np.longdouble"""
    import mpmath

    with mpmath.workprec(120):
        out = [_ext(mpmath.loggamma((mpmath.mpf(nu0) + a + dim) / 2) - mpmath.loggamma((mpmath.mpf(nu0) + a) / 2)) for a in range(n)]
    out = np.array(out, dtype=np.longdouble)
    out.setflags(write=False)
    return out


# Ways in which a detector can be subtly wrong (tests/test_bocpd_net_cases_cpu.py: each must move the net of tests/bocpd_net_cases.py).
# `nl` is the chain kernel's lanes per workgroup at the case's dim.
WRONG = ("coef-kappa", "exponent-nu", "keep-m", "block-edge", "map-live", "stale-ld")


def _detect(X, prm, stable, dtype=np.float64, wrong=None, nl=0):
    ext = dtype is not np.float64
    assert stable or not (ext or wrong)
    if ext:
        import mpmath

        assert np.finfo(dtype).eps < 1.1e-19, "the extended model needs an 80-bit (or wider) long double"
        with mpmath.workprec(120):
            pi = _ext(mpmath.pi)
    else:
        pi = np.pi
    F = dtype
    X = np.asarray(X, dtype=F)
    dim, T = X.shape
    h = F(1.0) / F(prm["lam"])
    kappa0, nu0, sigma0 = F(prm["kappa0"]), F(prm["nu0"]), F(prm["sigma0"])
    drop, settle, confirm = prm["drop"], prm["settle"], prm["confirm"]
    sqrt_sigma0 = np.sqrt(sigma0) if ext else math.sqrt(sigma0)
    log_h, log_1mh = (np.log(h), np.log1p(-h)) if ext else (math.log(h), math.log1p(-h))
    lgam = _lgam_ext(float(nu0), dim, T) if ext else None
    mu = np.zeros((1, dim), dtype=F)
    S = sigma0 * np.eye(dim, dtype=F)[None]             # literal: Sigma per hypothesis
    L = sqrt_sigma0 * np.eye(dim, dtype=F)[None]        # stable: its Cholesky factor
    Lstale = L
    col = np.array([0.0 if stable else 1.0], dtype=F)   # column t as stored (log R when stable)
    n = 1
    logpred = np.full((T, T), np.nan, dtype=F)
    R = np.zeros((T + 1, T + 1), dtype=F)
    R[0, 0] = 1.0
    map_run = np.zeros(T, dtype=np.int64)
    cps, discarded, declared_at = [], [], []
    flag = cnt = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            x = X[:, t]
            a = np.arange(n)
            kap, nu = kappa0 + a, nu0 + a
            delta = x[None] - mu
            # 1. predictive
            if stable:
                s = nu * kap / (2.0 * (kap + 1.0))
                z = np.zeros((n, dim), dtype=F)
                u = delta.copy()
                for k in range(dim):                    # L z = delta, column by column
                    z[:, k] = u[:, k] / L[:, k, k]
                    u[:, k + 1:] -= L[:, k + 1:, k] * z[:, k:k + 1]
                quad = s * np.sum(z * z, axis=1)
                Ld = Lstale if wrong == "stale-ld" and t == T // 2 else L
                logdetc = dim * np.log(s) - 2.0 * np.sum(np.log(np.diagonal(Ld, axis1=1, axis2=2)), axis=1)
            else:
                c = np.linalg.inv(2.0 * (kap + 1.0)[:, None, None] * S / (nu * kap)[:, None, None])
                quad = np.einsum("ni,nij,nj->n", delta, c, delta)
                logdetc = np.log(np.linalg.det(c))
            expo = nu if wrong == "exponent-nu" else nu + dim
            logp = (lgam[:n] if ext else _lgam(nu, dim)) + 0.5 * logdetc - 0.5 * dim * np.log(nu * pi) - 0.5 * expo * np.log1p(quad / nu)
            logpred[t, :n] = logp
            # 2. growth and change-point mass
            new = np.empty(n + 1, dtype=F)
            if stable:
                v = col[:n] + logp
                M = v.max()
                new[1:] = v - M - (np.log(np.exp(v - M).sum()) if ext else math.log(np.exp(v - M).sum())) + log_1mh
                new[0] = log_h
                R[t + 1, :n + 1] = np.exp(new)
            else:
                g = col[:n] * np.exp(logp)
                new[1:] = g * (1.0 - h)
                new[0] = np.sum(g * h)
                new = new / new.sum()
                R[t + 1, :n + 1] = new
            # 3. MAP run length of column t (argmax takes the first of equal maxima: the lowest age)
            m = 1 + int(np.argmax(col[:n] if wrong == "map-live" else col))
            map_run[t] = m
            # 4. detection heuristic
            keep = n
            if t > 0:
                dm = m - map_run[t - 1]
                if dm < -drop:
                    flag = 1
                elif flag:
                    if abs(dm) < settle:
                        cnt += 1
                        if cnt > confirm:
                            cps.append((t + 1) - m + 1)
                            declared_at.append(t)
                            flag = cnt = 0
                            keep = min(n, m if wrong == "keep-m" else max(m - 1, 0))
                            discarded.append(n - keep)
                    else:
                        flag = cnt = 0
            mu, S, L, kap, delta = mu[:keep], S[:keep], L[:keep], kap[:keep], delta[:keep]
            # 5. ageing
            coef = kap / (2.0 * (kap if wrong == "coef-kappa" else kap + 1.0))
            prior = sqrt_sigma0 * np.eye(dim, dtype=F)[None]
            aged = (kap[:, None] * mu + x[None]) / (kap[:, None] + 1.0)
            if stable:
                Ln = L.copy()
                w = np.sqrt(coef)[:, None] * delta
                for k in range(dim):                    # rank-one update, column by column
                    r = np.sqrt(Ln[:, k, k] ** 2 + w[:, k] ** 2)
                    c_, s_ = r / Ln[:, k, k], w[:, k] / Ln[:, k, k]
                    Ln[:, k, k] = r
                    Ln[:, k + 1:, k] = (Ln[:, k + 1:, k] + s_[:, None] * w[:, k + 1:]) / c_[:, None]
                    w[:, k + 1:] = c_[:, None] * w[:, k + 1:] - s_[:, None] * Ln[:, k + 1:, k]
                if wrong == "block-edge" and keep > 0 and t > 0 and t % nl == 0:      # the birth at a block's first step misses that step's sample
                    Ln[0], aged[0] = L[0], mu[0]
                Lstale = np.concatenate([prior, L])
                L = np.concatenate([prior, Ln])
            else:
                S = np.concatenate([sigma0 * np.eye(dim)[None], S + coef[:, None, None] * delta[:, :, None] * delta[:, None, :]])
            mu = np.concatenate([np.zeros((1, dim), dtype=F), aged])
            col = new
            n = keep + 1
    return dict(logpred=logpred, R=R, R_last=R[T].copy(), map_run=map_run, changepoints=cps, discarded=discarded, declared_at=declared_at)


def literal_model(X, **prm):
    return _detect(X, {**params(dict(dim=np.shape(X)[0])), **prm}, stable=False)


def stable_model(X, **prm):
    return _detect(X, {**params(dict(dim=np.shape(X)[0])), **prm}, stable=True)


def extended_model(X, wrong=None, nl=0, **prm):
    """stable_model one precision up: np.longdouble (80-bit: asserted, not assumed) with pi, log h, log1p(-h) and sqrt(sigma0) formed in that
    type and the lgamma difference from mpmath at 120 bits.  Its logpred, R and R_last are np.longdouble arrays.  `wrong` (one of WRONG)
    runs a detector with that mistake instead."""
    return _detect(X, {**params(dict(dim=np.shape(X)[0])), **prm}, stable=True, dtype=np.longdouble, wrong=wrong, nl=nl)


@lru_cache(maxsize=None)
def reference(name, seed=0):
    """(X, stable_model's result) of a case's replica, computed once per process"""
    cs = find(name)
    X = series(cs, seed)
    X.setflags(write=False)
    return X, stable_model(X, **params(cs))


@lru_cache(maxsize=None)
def literal_reference(name, seed=0):
    cs = find(name)
    return literal_model(series(cs, seed), **params(cs))


def column_gap(R):
    """the least relative gap between the largest entry of a column and its runner-up, over the columns with two entries or more"""
    worst = np.inf
    for t in range(1, R.shape[0]):
        c = np.sort(R[t, :t + 1])[::-1]
        if c[0] > 0:
            worst = min(worst, (c[0] - c[1]) / c[0])
    return worst
