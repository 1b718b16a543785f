"""The convergence experiment (Convergence/main.m, the appendix experiment behind the paper's Figure 1) on the device: the PSMF filter
swept `n_iter` times over one series, every sweep restarted from the first filtered state of the one before, and every filtered
posterior compared in Wasserstein-2 distance with that of the optimal Kalman filter, which knows the true C.

`convergence_batch` runs it for a batch of independent replicas in one call (psmf_conv_run, include/psmf_hip.h: 1 <= r <= 4,
r <= d <= 16), float64 throughout, R diagonal, one lane per replica with the whole state in registers.  The Kalman pass, from
x = x0_kalman, P = P0_kalman, for t = 1 .. n:

    Pp = P + Q,  S = (R + Ctrue Pp Ctrue^T)^-1,  x <- x + Pp Ctrue^T S (y_t - Ctrue x),  P <- Pp - Pp Ctrue^T S Ctrue Pp

One iteration, with V = v I at its top and (xp, Pprev) = (x0, P0) at t = 1, the step before's (Xps_t-1, Pps_t-1) after that:

    Pp = Pprev + q_scale Q                  s = xp^T V xp                    eta = trace(r_scale R + C Pp C^T) / d
    S = (r_scale R + s I + C Pp C^T)^-1     Xps_t = xp + Pp C^T S (y_t - C xp)    Pps_t = Pp - Pp C^T S C Pp
    C <- C + (y_t - C xp) xp^T V / (s + eta)                                 V <- V - V xp xp^T V / (s + eta)
    Cerr_t = ||C - Ctrue||_2                W_t = W2(N(Xps_t, Pps_t), N(Xk_t, Pk_t)) for t >= 2,  W_1 = 0

and after the sweep avW = mean(W) over all n entries, CerrI = ||C - Ctrue||_2, ErM = ||Y - C Xps||_2 (both Matlab's `norm` of a
matrix: the largest singular value).  The next iteration starts from x0 = Xps_1, P0 = Pps_1, keeps C and resets V.

Departures from the reference, each on purpose: main.m:54 restarts P0 from `Pps(:,1)`, which is Pps(:,:,1) at r = 1 -- the reference's
only shape -- and a column vector broadcast against Q, no covariance, at r > 1: P0 = Pps(:,:,1) is what runs here.  KL.m is never
called upstream and is not provided.  A W2^2 that cancellation makes negative is returned as 0 (Matlab: a complex number).  q_scale and
r_scale are the `R = 1 * R; Q = 1 * Q` knobs of main.m:44-45: the filter uses q_scale Q and r_scale R, the Kalman pass Q and R.

The 10^7 serial steps of the reference's run (n = 1000, 10000 iterations) are split into launches of at most 2^20 steps; the state
crosses them in device memory as float64, so a run gives the same bits however it is split (PSMF_CONV_ITERS=k: at most k iterations
per launch), in whatever chunks of replicas the batch is taken (PSMF_CONV_CHUNK=n), and in two calls of k iterations as in one of 2 k.
There is no CPU fallback.
"""

import ctypes as C

import numpy as np

from . import _capi

__all__ = ["convergence_batch", "convergence_experiment"]

MAX_D, MAX_R = 16, 4                    # psmf_conv_run's limits


def _tri(r):
    return np.tril_indices(r)


def _unpack(P, r):
    """(..., nt) packed lower triangles by rows -> (..., r, r) symmetric"""
    out = np.zeros(P.shape[:-1] + (r, r))
    i, j = _tri(r)
    out[..., i, j] = P
    out[..., j, i] = P
    return out


def _spectral(A):
    """largest singular value of the trailing (p, q) matrices"""
    return np.linalg.norm(A, ord=2, axis=(-2, -1))


def _broadcast(a, B, shape, name):
    a = np.asarray(a, dtype=np.float64)
    if a.shape == shape:
        a = np.broadcast_to(a, (B,) + shape)
    if a.shape != (B,) + shape:
        raise ValueError(f"{name} has shape {a.shape}, expected {shape} or {(B,) + shape}")
    return np.array(a, dtype=np.float64, order="C", copy=True)


def _diag_R(R, d):
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 0:
        R = np.full(d, float(R))
    elif R.shape == (d, d):
        if np.any(R != np.diag(np.diag(R))):
            raise ValueError("R must be diagonal: a scalar, a (d,) vector or a diagonal (d, d) matrix")
        R = np.diag(R).copy()
    if R.shape != (d,):
        raise ValueError(f"R has shape {R.shape}, expected a scalar, ({d},) or a diagonal ({d}, {d})")
    if not (np.all(np.isfinite(R)) and np.all(R > 0)):
        raise ValueError("need a finite R > 0 in every row")
    return np.ascontiguousarray(R)


def convergence_batch(Y, Ctrue, C0, x0, P0, *, Q, R, v=1.0, q_scale=1.0, r_scale=1.0, n_iter, x0_kalman, P0_kalman, want_moments=False,
                      device=0, status=True):
    """Run `n_iter` iterations of the module docstring for `batch` replicas in one call.

    Shared data: Y (d, n), Ctrue (d, r), x0_kalman (r,), P0_kalman (r, r) -- one series and one Kalman path for all replicas, which
    differ in C0 (batch, d, r), x0 (batch, r), P0 (batch, r, r), v, q_scale and r_scale (batch,).  Own data: Y (batch, d, n), with
    Ctrue, x0_kalman and P0_kalman per replica as well.  Every per-replica argument may be given once and is broadcast; with shared
    data the batch is that of the first per-replica argument with a batch axis, 1 if there is none.  Q (r, r) symmetric positive
    definite; R a scalar, a (d,) vector or a diagonal (d, d) matrix, positive.  Limits: 1 <= r <= 4, r <= d <= 16 (for d < r the
    factorisation is not identifiable and the recursion amplifies rounding without bound), n >= 2, n_iter >= 1.  The restart is
    P0 = Pps(:,:,1) (module docstring).  No argument is modified.

    Returns a dict: avW, CerrI, ErM (batch, n_iter) -- ErM is NaN without `want_moments`, but for the last iteration, which the host
    forms from Xps and C; with it the device returns the sums the E E^T of every iteration is formed from --; Xk (r, n) and Pk (r, r, n), the Kalman path
    (own data: (batch, r, n), (batch, r, r, n)); Xps (batch, r, n), Pps (batch, r, r, n), W (batch, n), Cerr (batch, n) of the last
    iteration; C (batch, d, r), x0 (batch, r), P0 (batch, r, r), the final C and the restart -- what a continuing call takes: two
    calls of k iterations give the bits of one call of 2 k --; status (batch,) int32 -- 0, or PSMF_ERR_NUMERIC (-4) for a replica with
    a non-finite input, a non-positive pivot or a non-finite state; it stops there and the others are untouched by it -- and elapsed_ms
    of the kernels.  `status=None` asks for no per-replica status: a failed replica then fails the call (numpy.linalg.LinAlgError)."""
    Y = np.asarray(Y, dtype=np.float64)
    Ctrue = np.asarray(Ctrue, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    if Y.ndim not in (2, 3):
        raise ValueError("Y must be (d, n), shared by the replicas, or (batch, d, n)")
    own = Y.ndim == 3
    d, n = Y.shape[-2:]
    if C0.ndim not in (2, 3) or C0.shape[-2] != d:
        raise ValueError(f"C0 must be (d, r) or (batch, d, r) with d = {d}; it has shape {C0.shape}")
    r = C0.shape[-1]
    if not 1 <= r <= MAX_R:
        raise ValueError(f"need 1 <= r <= {MAX_R} (the r x r state lives in a lane's registers; r = {r})")
    if d > MAX_D:
        raise ValueError(f"need d <= {MAX_D} (C lives in a lane's registers; d = {d})")
    if r > d:
        raise ValueError(f"need r <= d (for d < r the factorisation is not identifiable; d = {d}, r = {r})")
    if n < 2:
        raise ValueError(f"need n >= 2 (n = {n})")
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError(f"need n_iter >= 1 (n_iter = {n_iter})")
    if own:
        B = Y.shape[0]
    else:
        per = [(C0, 3), (x0, 2), (P0, 3), (v, 1), (q_scale, 1), (r_scale, 1)]
        B = next((np.shape(a)[0] for a, nd in per if np.ndim(a) == nd), 1)
    if B < 1:
        raise ValueError("need batch >= 1")
    Rd = _diag_R(R, d)
    Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
    if Q.shape != (r, r):
        raise ValueError(f"Q has shape {Q.shape}, expected {(r, r)}")
    if not np.all(np.isfinite(Q)) or np.any(Q != Q.T) or np.any(np.linalg.eigvalsh(Q) <= 0):
        raise ValueError("Q must be symmetric positive definite")
    Cb = _broadcast(C0, B, (d, r), "C0")
    xb = _broadcast(x0, B, (r,), "x0")
    Pb = _broadcast(P0, B, (r, r), "P0")
    vb = _broadcast(v, B, (), "v")
    qb = _broadcast(q_scale, B, (), "q_scale")
    rb = _broadcast(r_scale, B, (), "r_scale")
    if np.any(vb <= 0) or np.any(qb < 0) or np.any(rb <= 0):        # (a NaN passes: it fails its replica)
        raise ValueError("need v > 0, q_scale >= 0 and r_scale > 0")
    if own:
        Ct = _broadcast(Ctrue, B, (d, r), "Ctrue")
        xk0 = _broadcast(x0_kalman, B, (r,), "x0_kalman")
        Pk0 = _broadcast(P0_kalman, B, (r, r), "P0_kalman")
        Yt = np.ascontiguousarray(np.transpose(Y, (0, 2, 1)))       # time-major: column t of the reference's (d, n) is row t
        lead = (B,)
    else:
        Ct = np.ascontiguousarray(Ctrue)
        xk0 = np.ascontiguousarray(np.asarray(x0_kalman, dtype=np.float64))
        Pk0 = np.ascontiguousarray(np.asarray(P0_kalman, dtype=np.float64))
        if Ct.shape != (d, r) or xk0.shape != (r,) or Pk0.shape != (r, r):
            raise ValueError(f"shared data takes Ctrue {(d, r)}, x0_kalman {(r,)} and P0_kalman {(r, r)}; got {Ct.shape}, {xk0.shape}, {Pk0.shape}")
        if not all(np.all(np.isfinite(a)) for a in (Y, Ct, xk0, Pk0)):
            raise ValueError("the shared Y, Ctrue, x0_kalman and P0_kalman must be finite")
        Yt = np.ascontiguousarray(Y.T)
        lead = ()
    nt = r * (r + 1) // 2
    want_moments = bool(want_moments)
    Xk, Pk = np.zeros(lead + (n, r)), np.zeros(lead + (n, nt))
    avW, CerrI = np.zeros((B, n_iter)), np.zeros((B, n_iter))
    Cit = np.zeros((B, n_iter, d, r)) if want_moments else None
    Sxy = np.zeros((B, n_iter, r, d)) if want_moments else None
    Sxx = np.zeros((B, n_iter, nt)) if want_moments else None
    Xps, Pps, W, Cerr = np.zeros((B, n, r)), np.zeros((B, n, nt)), np.zeros((B, n)), np.zeros((B, n))
    st = np.zeros(B, dtype=np.int32) if status is not None and status is not False else None
    cfg = _capi.PsmfConvConfig(abi_version=_capi.ABI_VERSION, d=d, n=n, r=r, batch=B, n_iter=n_iter, own_data=int(own),
                               want_moments=int(want_moments), device=int(device))
    ms = C.c_float()
    ptr = _capi._ptr
    lib = _capi.load_library()
    rc = lib.psmf_conv_run(C.byref(cfg), ptr(Yt), ptr(Ct), ptr(Q), ptr(Rd), ptr(xk0), ptr(Pk0), ptr(vb), ptr(qb), ptr(rb), ptr(Cb), ptr(xb),
                           ptr(Pb), ptr(Xk), ptr(Pk), ptr(avW), ptr(CerrI), ptr(Cit), ptr(Sxy), ptr(Sxx), ptr(Xps), ptr(Pps), ptr(W), ptr(Cerr),
                           ptr(st), C.byref(ms))
    _capi.raise_for(lib, rc, f"psmf_conv_run failed ({rc})")
    Xps_c = np.transpose(Xps, (0, 2, 1))                            # (batch, r, n)
    Yb = Y if own else Y[None]
    if not want_moments:
        ErM = np.full((B, n_iter), np.nan)
        ErM[:, -1] = _spectral(Yb - Cb @ Xps_c)
    else:
        YY = Yb @ np.transpose(Yb, (0, 2, 1))
        CS = Cit @ Sxy                                              # (batch, n_iter, d, d)
        EE = YY[:, None] - CS - np.transpose(CS, (0, 1, 3, 2)) + Cit @ _unpack(Sxx, r) @ np.transpose(Cit, (0, 1, 3, 2))
        top = np.linalg.eigvalsh(0.5 * (EE + np.transpose(EE, (0, 1, 3, 2))))[..., -1]
        ErM = np.sqrt(np.maximum(top, 0.0))
    ax = tuple(range(len(lead))) + tuple(len(lead) + k for k in (1, 0))
    return dict(avW=avW, CerrI=CerrI, ErM=ErM, Xk=np.transpose(Xk, ax), Pk=np.moveaxis(_unpack(Pk, r), len(lead), -1),
                Xps=Xps_c, Pps=np.moveaxis(_unpack(Pps, r), 1, -1), W=W, Cerr=Cerr, C=Cb, x0=xb, P0=Pb, status=st, elapsed_ms=ms.value)


def convergence_experiment(Y, Ctrue, Q, R, *, n_iter=10000, repeats=1, seed=None, device=0):
    """Convergence/main.m on the device, `repeats` random starts at once: per repeat it draws X0k = 5 randn(r), X0ps = 5 randn(r) and
    C = 10 |randn(d, r)|, in that order, from numpy.random.default_rng(seed) (Matlab's legacy stream cannot be reproduced), and uses
    P0k = 5 I, P0 = 25 I, v = 1.  Y is (d, n), Ctrue (d, r), Q (r, r), R as in `convergence_batch`.

    Returns what Figure 1 plots, per repeat: avW and CerrI (repeats, n_iter), Xk and Xps (repeats, r, n) -- and ErM of the last
    iteration (repeats,), C (repeats, d, r), status and elapsed_ms."""
    Y = np.asarray(Y, dtype=np.float64)
    Ctrue = np.asarray(Ctrue, dtype=np.float64)
    if Y.ndim != 2 or Ctrue.ndim != 2 or Ctrue.shape[0] != Y.shape[0]:
        raise ValueError("convergence_experiment takes Y (d, n) and Ctrue (d, r)")
    d, r = Ctrue.shape
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError("need repeats >= 1")
    rng = np.random.default_rng(seed)
    x0k, x0, C0 = np.zeros((repeats, r)), np.zeros((repeats, r)), np.zeros((repeats, d, r))
    for k in range(repeats):
        x0k[k] = 5.0 * rng.standard_normal(r)
        x0[k] = 5.0 * rng.standard_normal(r)
        C0[k] = 10.0 * np.abs(rng.standard_normal((d, r)))
    res = convergence_batch(np.broadcast_to(Y, (repeats,) + Y.shape), Ctrue, C0, x0, 25.0 * np.eye(r), Q=Q, R=R, v=1.0, n_iter=n_iter,
                            x0_kalman=x0k, P0_kalman=5.0 * np.eye(r), device=device)
    return dict(avW=res["avW"], CerrI=res["CerrI"], Xk=res["Xk"], Xps=res["Xps"], ErM=res["ErM"][:, -1], C=res["C"], status=res["status"],
                elapsed_ms=res["elapsed_ms"])
