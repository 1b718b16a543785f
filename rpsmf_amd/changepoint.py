"""The change-point experiment's detectors (ExperimentChange/main.m): the multivariate Bayesian online change-point detection
baseline on the device, and the single change-point search on the host.

`mvbocpd_batch` runs ExperimentChange/MVBOCPD.m -- a normal-inverse-Wishart model per run length, Student-t predictive, constant
hazard h = 1 / lambda and the reference's detection heuristic -- for a batch of independent series (psmf_bocpd_run,
include/psmf_hip.h: dim <= 32, T <= 4096), float64 throughout.  Time is 1-based, t = 1 .. T; a hypothesis of age a has absorbed the a
most recent samples, kappa = kappa0 + a, nu = nu0 + a, and absorbing x moves it by

    delta = x - mu,   mu <- (kappa mu + x) / (kappa + 1),   Sigma <- Sigma + kappa / (2 (kappa + 1)) delta delta^T

Age 0 is always the prior (mu = 0, Sigma = sigma0 I).  With n_t live hypotheses at step t (n_1 = 1), in this order:

    1. log p_a = lgamma((nu + dim) / 2) - lgamma(nu / 2) + log det(c) / 2 - dim / 2 log(nu pi) - (nu + dim) / 2 log1p(delta^T c delta / nu),
       c = [2 (kappa + 1) Sigma / (nu kappa)]^-1
    2. R(a + 1, t + 1) = R(a, t) p_a (1 - h),  R(0, t + 1) = sum_a R(a, t) p_a h  over a < n_t; the column is normalised to sum 1
       (mass that column t still holds at ages >= n_t after a truncation is dropped)
    3. m_t = 1 + argmax_a R(a, t), over column t as stored, the lowest age on a tie
    4. for t > 1: m_t - m_{t-1} < -drop sets a flag.  Otherwise, with the flag set: |m_t - m_{t-1}| < settle counts up, and a count
       above `confirm` declares the change point cp = t - m_t + 1, clears flag and count and discards the hypotheses of age
       >= m_t - 1, so that n_{t+1} = m_t; |m_t - m_{t-1}| >= settle clears flag and count
    5. every remaining hypothesis absorbs x_t and ages by one; a fresh prior enters at age 0

The device keeps the Cholesky factor of Sigma per hypothesis (one forward substitution and one rank-one update per step; no inverse,
no determinant) and carries R in the log domain: a step at which every p_a underflows in float64, where the reference's linear
recursion turns into NaN, leaves it finite.  There is no CPU fallback.

Accuracy: with a prior on the data's scale (sigma0 within a few powers of ten of the data's variance) log p is good to about 1e-12
absolute and R to 1e-13 of its largest entry, at any dim and T the library takes. With a prior far off that scale -- data at 1e3
under sigma0 = 1 -- the first sample moves the factor by six orders of magnitude, and a float64 formulation with the textbook
rank-one update (w_i <- c w_i - s L_ik', the difference of two products a million times its result) loses about eight digits of log p:
the numpy model of the tests is 4e-9 (dim 5) and 3e-8 (dim 32) off there. The device updates w_i <- (w_i - s L_ik) / c and stays
within 1e-11 (2.7e-12 and 8.3e-12 measured); map_run and the change points are not affected either way as long as the columns of R
have a clear maximum. A hypothesis that has absorbed a sample beyond about 1e15 times the data's scale (1e100, say) stays finite,
but float64 no longer holds the later samples beside it and its log p is not meaningful (it is strongly negative: such a hypothesis
weighs nothing in R); a sample whose square overflows (about 1e154 and beyond) fails its replica. tests/test_hip_bocpd_edges.py
measures all three.

A batch whose scratch does not fit half of the free device memory is processed in chunks of series; PSMF_BOCPD_CHUNK=n (read at every
call) caps a chunk at n series, which changes no output bit.

`MVBOCPD` keeps the Matlab function's signature.  `find_changepoint` is the single change-point search of the experiment's other two
columns, host numpy: two cumulative sums per row.
"""

import ctypes as C

import numpy as np

from . import _capi

__all__ = ["mvbocpd_batch", "MVBOCPD", "find_changepoint"]

MAX_DIM, MAX_T = 32, 4096               # psmf_bocpd_run's limits
MAX_TABLE_DOUBLES = 1 << 28             # want_R / want_logpred: 2 GiB of output each


def mvbocpd_batch(X, *, lam=200.0, kappa0=1.0, nu0=None, sigma0=1.0, drop=10, settle=10, confirm=10, max_changepoints=16,
                  want_R=False, want_logpred=False, device=0, status=True):
    """Run the detector of the module docstring on `batch` independent series in one call.

    X is (batch, dim, T) or (dim, T), a row per channel as the reference holds it; a single series is a batch of one.  The prior is
    mu0 = 0, kappa0, nu0 (default: dim), Sigma0 = sigma0 I; the hazard is 1 / lam.  No argument is modified.

    Returns a dict: map_run (batch, T) int32, the m_t; changepoints, a list of `batch` int arrays with the declared cp values in
    order (1-based, at most `max_changepoints` of them; the reference's leading 0 is omitted); n_changepoints (batch,) int32, how
    many were declared, stored or not; R_last (batch, T + 1), column T + 1 of R by age; R (batch, T + 1, T + 1) with R[:, t - 1] =
    column t by age (zero where nothing is stored) or None; logpred (batch, T, T) with logpred[:, t - 1, a] = log p_a of step t, NaN
    where age a is not live, or None; status (batch,) int32 -- 0, or PSMF_ERR_NUMERIC (-4) for a replica with a non-finite sample, a
    non-finite state or a non-positive pivot; the others are untouched by it -- and elapsed_ms of the kernels.  `status=None` asks
    for no per-replica status: a failed replica then fails the call (numpy.linalg.LinAlgError, naming the replica)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[None]
    if X.ndim != 3:
        raise ValueError("X must be (batch, dim, T) or (dim, T)")
    B, dim, T = X.shape
    nu0 = float(dim) if nu0 is None else nu0
    for name, v in (("lam", lam), ("kappa0", kappa0), ("nu0", nu0), ("sigma0", sigma0)):
        if np.ndim(v) != 0:
            raise ValueError(f"{name} must be a scalar")
    want_R, want_logpred = bool(want_R), bool(want_logpred)
    if 1 <= dim <= MAX_DIM and 1 <= T <= MAX_T:      # (the library words the refusal of a bad shape)
        if want_R and B * (T + 1) * (T + 1) > MAX_TABLE_DOUBLES:
            raise ValueError("psmf_bocpd_run: want_R: batch x (T + 1) x (T + 1) exceeds the limit of 2^28 doubles (2 GiB)")
        if want_logpred and B * T * T > MAX_TABLE_DOUBLES:
            raise ValueError("psmf_bocpd_run: want_logpred: batch x T x T exceeds the limit of 2^28 doubles (2 GiB)")
    else:
        want_R = want_logpred = False
    maxcp = int(max_changepoints)
    Xt = np.ascontiguousarray(np.transpose(X, (0, 2, 1)))       # time-major: column t of the reference's (dim, T) is row t
    map_run = np.zeros((B, T), dtype=np.int32)
    cps = np.zeros((B, max(maxcp, 1)), dtype=np.int32)
    ncp = np.zeros(B, dtype=np.int32)
    R_last = np.zeros((B, T + 1))
    R = np.zeros((B, T + 1, T + 1)) if want_R else None
    lp = np.zeros((B, T, T)) if want_logpred else None
    st = np.zeros(B, dtype=np.int32) if status is not None and status is not False else None
    cfg = _capi.PsmfBocpdConfig(abi_version=_capi.ABI_VERSION, dim=dim, T=T, batch=B, device=int(device), drop=int(drop), settle=int(settle),
                                confirm=int(confirm), max_changepoints=maxcp, want_R=int(want_R), want_logpred=int(want_logpred),
                                lam=float(lam), kappa0=float(kappa0), nu0=float(nu0), sigma0=float(sigma0))
    ms = C.c_float()
    ptr = _capi._ptr
    lib = _capi.load_library()
    rc = lib.psmf_bocpd_run(C.byref(cfg), ptr(Xt), ptr(map_run), ptr(cps), ptr(ncp), ptr(R_last), ptr(R), ptr(lp), ptr(st), C.byref(ms))
    _capi.raise_for(lib, rc, f"psmf_bocpd_run failed ({rc})")
    found = [cps[b, :min(int(ncp[b]), maxcp)].copy() for b in range(B)]
    return dict(map_run=map_run, changepoints=found, n_changepoints=ncp, R_last=R_last, R=R, logpred=lp, status=st, elapsed_ms=ms.value)


def MVBOCPD(Y, start=400, window=(570, 630)):
    """ExperimentChange/MVBOCPD.m on the device: the detector runs on Y[:, start - 1:] (Matlab's Y(:, start:end)) with the
    reference's constants and returns 1 if a declared change point, moved back by `start`, lies strictly inside `window`, else 0."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] < start or start < 1:
        raise ValueError("MVBOCPD takes a (channels, n) array with n >= start >= 1")
    res = mvbocpd_batch(Y[:, start - 1:], max_changepoints=64, status=None)
    cp = start + res["changepoints"][0]
    return int(np.any((cp > window[0]) & (cp < window[1])))


def find_changepoint(x, statistic="rms", min_distance=1):
    """The single change point of a series: the 1-based index k in 2 .. n of the first sample of the second segment that minimises

        sum over channels of  (k - 1) log ms(1 .. k-1) + (n - k + 1) log ms(k .. n)

    where ms is the mean square of a segment, floored at the smallest normal double (a constant-zero segment costs a finite amount).
    This is the 'rms' statistic with one change as MathWorks documents it for findchangepts(x, 'Statistic', 'rms'); the toolbox
    routine is not available to compare against.  Ties go to the lowest k.  `min_distance` is the least length of either segment.

    x is (n,), (channels, n) or (batch, channels, n): with a leading batch axis an int64 array of `batch` indices is returned,
    otherwise an int.  Host numpy, O(channels n) from two cumulative sums per row."""
    if statistic != "rms":
        raise ValueError(f"statistic {statistic!r} is not supported: only 'rms'")
    x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (1, 2, 3):
        raise ValueError("x must be (n,), (channels, n) or (batch, channels, n)")
    batched = x.ndim == 3
    x3 = x.reshape((1,) * (3 - x.ndim) + x.shape)
    n = x3.shape[2]
    md = int(min_distance)
    if md < 1:
        raise ValueError("min_distance must be >= 1")
    if x3.shape[1] < 1 or n < 2 * md:
        raise ValueError(f"need at least one channel and n >= 2 * min_distance samples (n = {n})")
    if not np.all(np.isfinite(x3)):
        raise ValueError("x must be finite")
    tiny = np.finfo(np.float64).tiny
    sq = x3 * x3
    head = np.cumsum(sq, axis=2)[:, :, :-1]                          # sum over 1 .. k-1, k = 2 .. n
    tail = np.cumsum(sq[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:]   # sum over k .. n
    n1 = np.arange(1, n, dtype=np.float64)                           # k - 1
    n2 = n - n1
    cost = (n1 * np.log(np.maximum(head / n1, tiny)) + n2 * np.log(np.maximum(tail / n2, tiny))).sum(axis=1)
    cost = cost[:, md - 1:n - md]                                    # k - 1 >= md and n - k + 1 >= md
    k = np.argmin(cost, axis=1) + md + 1                             # (argmin takes the first of equal minima: the lowest k)
    return k.astype(np.int64) if batched else int(k[0])
