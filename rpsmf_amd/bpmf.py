"""The BPMF baseline of the imputation experiment (ExperimentImpute/BPMF.py:121-302) on the device: Bayesian probabilistic matrix
factorisation, a Gibbs sampler over the factors and their Gaussian-Wishart hyper-parameters, for a batch of independent replicas in
one call (psmf_bpmf_run, include/psmf_hip.h: 2 <= d <= 512, 2 <= r <= 16, n >= 2), float64 throughout.

Per replica, with mu, v = (y - mu) / mu and mbar as in rpsmf_amd.pmf:

    warm start   W (n x r), P (d x r) = pmf_batch's recursion with `epochs` epochs, epsilon 50, lmd 0.01, momentum 0.8, 9 batches
    avg = w_j . p_i + mbar at the probe entries (Mmiss_ij = 1),  c = 1
    epoch e = 1 .. epochs:
      for (F, N) = (W, n) and then (P, d), b0 = 2:   xbar = column mean of F,  S = numpy.cov(F, rowvar=False)
        WI = sym(inv(I + N S + N b0 / (b0 + N) xbar xbar^T)),   alpha = (C A)(C A)^T,  C = cholesky(WI),  A a standard Bartlett factor
        mu_h = cholesky(inv((b0 + N) alpha)).T z + N xbar / (b0 + N)
      twice:  every column j:  Lambda = alpha_m + beta sum_{i in obs(j)} p_i p_i^T,  b = beta sum (v_ij - mbar) p_i + alpha_m mu_m,
                               w_j = cholesky(inv Lambda).T z_j + inv(Lambda) b
              every row i likewise over its observed columns, with the new W
      avg = (c avg + w_j . p_i + mbar) / (c + 1),  c += 1,   Efull[e] = RMSEM(avg mu + mu, YorgInt, Mmiss)

The device factors every precision matrix Lambda = U U^T from the last row upwards and samples U^-1 z + U^-T U^-1 b, which is the
same thing without an inverse (U^-T is the lower Cholesky factor of inv(Lambda)); the hyper step likewise.

THE DRAW PROTOCOL.  No draw of the sampler depends on the data, so the host makes them all up front, with the legacy numpy calls the
reference and scipy.stats.wishart.rvs make, in their order (`draw_bpmf`), per replica:

    epochs x numpy.random.permutation(N)                              the warm start (N = training entries)
    per epoch:  Bartlett(r + n), numpy.random.randn(r, 1), Bartlett(r + d), numpy.random.randn(r, 1),
                then per sweep numpy.random.randn(n, r) and numpy.random.randn(d, r)
    Bartlett(df) = numpy.random.normal(size=r (r - 1) / 2) below the diagonal (numpy.tril_indices(r, -1)), then
                   numpy.random.chisquare(df - i, size=1) ** 0.5 for i = 0 .. r - 1 on it

(the reference's n calls of randn(r, 1) of a sweep are, in stream order, one randn(n, r)).  The reference's stored results are
reproduced that way.  There is no device-side random number generator and no CPU fallback.

One difference from the reference: its "simple fit" in front of the first epoch (BPMF.py:197-201) is dead code -- every value is
overwritten before it is used -- and is not computed.  The reference could in principle raise numpy.linalg.LinAlgError from
`inv(np.cov(w1_P1_sample))` there; this port cannot.

`bpmf` keeps the reference function's signature and consumes the global numpy RNG as the reference does.
"""

import numpy as np

from . import _capi
from . import pmf as _pmf

__all__ = ["bpmf_batch", "bpmf", "draw_bpmf"]

MAX_D, MAX_R = 512, 16                          # psmf_bpmf_run's limits
WARM_START = dict(epsilon=50, lmd=0.01, momentum=0.8, num_batches=9)      # BPMF.py:43-55
DRAW_KEYS = ("perms", "bartlett", "hyper_normals", "normals")


def _bartlett(df, r):
    """the standard Bartlett factor scipy.stats.wishart.rvs(df, scale) draws before it looks at the scale, with its calls in its order"""
    A = np.zeros((r, r))
    A[np.tril_indices(r, k=-1)] = np.random.normal(size=r * (r - 1) // 2)
    A[np.diag_indices(r)] = np.r_[[np.random.chisquare(df - i, size=1) ** 0.5 for i in range(r)]].reshape(r)
    return A


def draw_bpmf(d, n, r, N, epochs):
    """One replica's draws from the global numpy RNG, by the protocol of the module docstring.  A dict: perms, a list of `epochs`
    permutations of 0 .. N-1; bartlett (epochs, 2, r, r), the factor of the W side (df = r + n) and of the P side (df = r + d);
    hyper_normals (epochs, 2, r); normals (epochs, 2, n + d, r), per sweep the n rows of the columns' normals and then the d of the
    rows'."""
    perms = [np.random.permutation(N) for _ in range(epochs)]
    bart = np.zeros((epochs, 2, r, r))
    hz = np.zeros((epochs, 2, r))
    Z = np.zeros((epochs, 2, n + d, r))
    for e in range(epochs):
        for side, N_side in enumerate((n, d)):
            bart[e, side] = _bartlett(r + N_side, r)
            hz[e, side] = np.random.randn(r, 1)[:, 0]
        for s in range(2):
            Z[e, s, :n] = np.random.randn(n, r)
            Z[e, s, n:] = np.random.randn(d, r)
    return dict(perms=perms, bartlett=bart, hyper_normals=hz, normals=Z)


def _shapes(YorgInt, M, Mmiss, C0, X0):
    """pmf_batch's shape refusals, then this engine's limits.  Returns the arrays with the batch dimension in front and (d, n, r, B)."""
    YorgInt, M, Mmiss, C0, X0, (d, n, r, B) = _pmf._shapes(YorgInt, M, Mmiss, C0, X0)
    if d > MAX_D or r > MAX_R:
        raise ValueError(f"the device engine takes d <= {MAX_D} and r <= {MAX_R} (one workgroup holds P on chip); d = {d}, r = {r}")
    if d < 2 or n < 2:
        raise ValueError(f"d >= 2 and n >= 2 are needed (numpy.cov of the factors needs two rows); d = {d}, n = {n}")
    if r < 2:
        raise ValueError(f"r >= 2 is needed (at r = 1 the reference itself fails: numpy.cov returns a 0-d array); r = {r}")
    return YorgInt, M, Mmiss, C0, X0, (d, n, r, B)


def _check_draws(dr, b, d, n, r, epochs):
    if not isinstance(dr, dict) or any(k not in dr for k in DRAW_KEYS):
        raise ValueError(f"draws[{b}] must be a dict with the keys {DRAW_KEYS} (what draw_bpmf returns)")
    for key, shape in (("bartlett", (epochs, 2, r, r)), ("hyper_normals", (epochs, 2, r)), ("normals", (epochs, 2, n + d, r))):
        if np.shape(dr[key]) != shape:
            raise ValueError(f"draws[{b}][{key!r}] must have the shape {shape}, got {np.shape(dr[key])}")


def bpmf_batch(YorgInt, M, Mmiss, C0, X0, draws=None, *, epochs=2, beta=2, device=0, want_rec=False, warm_start=None):
    """Run the sampler of the module docstring on `batch` replicas in one call: pmf_batch's recursion for the warm start, then
    psmf_bpmf_run.

    Layouts are those of pmf_batch: YorgInt (d, n); M, Mmiss (batch, d, n) or (d, n), 0 / 1; C0 (batch, d, r); X0 (batch, r, n).
    `draws`: a list, one record per replica, of what `draw_bpmf(d, n, r, N, epochs)` returns (N the replica's training entries);
    None draws them from the global numpy RNG, replica by replica.  `warm_start` overrides keywords of the warm start's pmf_batch
    (epsilon, lmd, momentum, num_batches; the reference's 50, 0.01, 0.8, 9 otherwise) -- a tiny problem diverges at epsilon = 50 and
    has fewer than 9 training entries.  No argument is modified.

    Returns a dict: Efull (batch, epochs); C (batch, d, r) = P and X (batch, r, n) = W^T, the last sample of the factors in
    standardised units; mean and mean_rating (batch,), mu and mbar; status (batch,) int32 -- 0, or PSMF_ERR_NUMERIC (-4) for a
    replica in which a precision matrix was not positive definite (numpy.linalg.LinAlgError in the reference) or that left the
    finite range (a warm start that diverged does), the others being untouched by it; elapsed_ms of the kernels, warm start plus
    sweeps; with want_rec, Yrec (batch, d, n): the reference's Yrec2 of the last epoch (the averaged prediction at the probe entries,
    0 elsewhere).

    ValueError before any device work: what pmf_batch refuses (inconsistent shapes; M or Mmiss not 0 / 1; fewer training entries
    than batches of the warm start; a replica without a probe entry; mu == 0; d > 512 or r > 16), d < 2, r < 2, n < 2, and draws of
    the wrong shapes."""
    YorgInt, M, Mmiss, C0, X0, (d, n, r, B) = _shapes(YorgInt, M, Mmiss, C0, X0)
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError("epochs must be >= 1")
    ws = dict(WARM_START)
    if warm_start:
        if set(warm_start) - set(WARM_START):
            raise ValueError(f"warm_start takes the keywords {sorted(WARM_START)}, got {sorted(warm_start)}")
        ws.update(warm_start)
    Mb = _pmf._zero_one(M, "M")
    _pmf._zero_one(Mmiss, "Mmiss")
    if draws is None:
        draws = [draw_bpmf(d, n, r, int(np.count_nonzero(Mb[b])), epochs) for b in range(B)]
    elif len(draws) != B:
        raise ValueError(f"draws must have one record per replica ({B}), got {len(draws)}")
    for b, dr in enumerate(draws):
        _check_draws(dr, b, d, n, r, epochs)
    h = _pmf._prepare(YorgInt, M, Mmiss, C0, X0, [dr["perms"] for dr in draws], epochs, ws["num_batches"])
    h["Mt"] = np.ascontiguousarray(np.transpose(Mb, (0, 2, 1)).astype(np.uint8))      # time-major, as the probe mask
    warm = _pmf._launch(h, ws["epsilon"], ws["lmd"], ws["momentum"], device, False)
    return _sweeps(h, warm, draws, beta, device, want_rec)


def _sweeps(h, warm, draws, beta, device, want_rec):
    """psmf_bpmf_run on what pmf's `_prepare` made (with the training mask, time-major, under "Mt"), the warm start `warm` that
    pmf's `_launch` returned for it, and the draws"""
    bart, hz, Z = (np.ascontiguousarray(np.stack([np.asarray(dr[k], dtype=np.float64) for dr in draws])) for k in ("bartlett", "hyper_normals", "normals"))
    Pb = warm["C"]                                                              # (batch, d, r): h's own buffer, overwritten below
    Wb = np.ascontiguousarray(np.transpose(warm["X"], (0, 2, 1)))               # (batch, n, r)
    mean, mbar = warm["mean"], warm["mean_rating"]
    cfg = _capi.PsmfBpmfConfig(abi_version=_capi.ABI_VERSION, d=h["d"], n=h["n"], r=h["r"], batch=h["B"], epochs=h["epochs"], device=int(device),
                               want_rec=int(bool(want_rec)), beta=float(beta))
    return _pmf._native_run("psmf_bpmf_run", cfg, [h["Yt"], h["Mt"], h["Mmt"], mean, mbar, bart, hz, Z], Pb, Wb, mean, mbar, warm["elapsed_ms"])


def bpmf(Y, C, X, num_p, num_m, num_feat, M, Mmiss, YorigInt, Einit, epochs=50, beta=2):
    """ExperimentImpute/BPMF.py:121-302 on the device.  Returns (Epred, Efull, RunTime) like the reference, each (1, epochs + 1):
    column 0 is Einit, Epred is NaN beyond it (BPMF predicts nothing online), RunTime spreads the kernels' time evenly over the
    epochs.  Every draw comes from the global numpy RNG in the reference's order (`draw_bpmf`): a script that saves and restores
    the RNG state around the call (BPMF.py:361-375) gets the same repeats.  Raises numpy.linalg.LinAlgError where the reference
    would (a precision matrix that is not positive definite), which is what that script catches.  Requires Y == YorigInt * M."""
    YorigInt = _pmf._reference_args(Y, C, X, num_p, num_m, num_feat, M, YorigInt)
    res = bpmf_batch(YorigInt, M, Mmiss, C, X, None, epochs=epochs, beta=beta)
    if res["status"][0] != 0:
        raise np.linalg.LinAlgError("a precision matrix of the sampler is not positive definite, or the factors left the finite range")
    return _pmf._reference_result(res, Einit, epochs)
