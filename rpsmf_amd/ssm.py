"""PSMF with linear-Gaussian dynamics and an observation map, on the device: the filter of the change-point experiment
(ExperimentChange/PSMF.m:6-45, driven by ExperimentChange/main.m).

The latent state x has its own dimension p >= r, moves by a linear map A with process noise Q and reaches the dictionary through an
observation map H (r x p), so y ~ C H x.  Per step, float64 throughout:

    xbar = A x                      Pbar = A P_prev A^T + Q
    z = H xbar, w = V z, s = z^T w, yhat = C z, e = y - yhat
    P_z = H Pbar H^T                S = C P_z C^T + (rho + s) I
    x  = xbar + Pbar H^T C^T S^-1 e
    P  = Pbar - Pbar H^T C^T S^-1 C H Pbar
    eta = trace(C P_z C^T + rho I) / d,  N = s + eta
    C += e w^T / N,  V -= w w^T / N

`carry_P=True` is the textbook recursion, P_prev = P_{t-1}.  `carry_P=False` is PSMF.m:30 as written: that line reads P(:,:,t),
which is still zero at that point, so P_prev is P0 at the first step of a series and 0 at every later step.

The robust form (rPSMF: a t-distributed likelihood, ExperimentImpute/rPSMF.py:75-135 and pypsmf/psmf/rpsmf.py:125-172) and missing
observations run in the same step loop (`robust=`, `mask=`; psmf_ssm_run_ex).  m is the 0/1 mask column of the step (all ones
without a mask), M = diag(m), Omega the running product of omega (1 at the start of a series, and always when not robust), e_i zero
on unobserved rows:

    xbar = A x                         Pbar = A P_prev A^T + Omega Q
    z = H xbar, w = V z, s = z^T w     yhat = C z                               (Ypred: all rows, observed or not)
    e_i = m_i (y_i - yhat_i)           y_i is not read where m_i = 0 (it may be NaN)
    P_z = H Pbar H^T                   rho_t = Omega rho
    S = (M C) P_z (M C)^T + diag(rho_t m) + s I                                 (rPSMF.py:92-98: s I, not s M)
    x = xbar + Pbar H^T (MC)^T S^-1 e
    omega = (lambda + e^T S^-1 e) / (lambda + d)                           rob  (d, not the observed count)
    P = beta omega (Pbar - Pbar H^T (MC)^T S^-1 (MC) H Pbar)               rob: beta omega; else 1
    eta = (rho_t sum m_i + trace((MC) P_z (MC)^T)) / d,   N = s + eta
    C += e w^T / N                                                              (unobserved rows do not move)
    phi = (lambda + e^T e / N) / (lambda + d)                              rob
    V = alpha phi (V - w w^T / N)                                          rob: alpha phi; else 1
    Omega <- omega Omega;  lambda <- lambda + d unless fixed_lambda        rob

A step without an observed row is refused (ValueError): eta = 0 and phi = 0 / 0 there.

Conditioning: the engine never forms the d x d matrix S; it forms P_z^-1 (r x r), so its error against the d x d recursion grows with
cond(P_z) ~ cond(H)^2 cond(Pbar).  With a plain Gaussian H and p = r at 15 / 16 two float64 models of the recursion differ by 7e-10
(d = 127, r = p = 15) and 1.1e-9 (d = 63, r = p = 16); with the singular values of H in [0.5, 1.5] (tests/ssm_net_cases.py) they agree to
1e-11 and the device is within 1e-11 of the d x d model.

`linear_psmf_batch` runs many independent series in one launch, one workgroup per replica (psmf_ssm_run and psmf_ssm_run_ex,
include/psmf_hip.h: d <= 512, r <= 16, r <= p <= 32); `PSMF` and `rPSMF` keep the Matlab function's signature;
`matern32_state_space` builds the (A, Q, H) of the experiment's Matern-3/2 prior from the closed form.  There is no CPU fallback.
"""

import ctypes as C

import numpy as np

from . import _capi

__all__ = ["linear_psmf_batch", "PSMF", "rPSMF", "matern32_state_space"]

MAX_D, MAX_R, MAX_P = 512, 16, 32      # psmf_ssm_run's limits (one workgroup per replica)


def matern32_state_space(lengthscale, variance, dt, r=1):
    """(A, Q, H) of r independent Matern-3/2 Gaussian processes sampled every `dt`: state (position, velocity) per factor, p = 2 r.

        lambda = sqrt(3) / lengthscale
        A2 = exp(-lambda dt) [[1 + lambda dt, dt], [-lambda^2 dt, 1 - lambda dt]]        (= expm(F dt), F = [[0, 1], [-lambda^2, -2 lambda]])
        Pinf = diag(variance, lambda^2 variance),  Q2 = Pinf - A2 Pinf A2^T,  H2 = [1 0]

    each Kronecker-multiplied with I_r (as ExperimentChange/main.m does): the positions come first, then the velocities."""
    lengthscale, variance, dt, r = float(lengthscale), float(variance), float(dt), int(r)
    if not (lengthscale > 0 and variance > 0 and dt > 0 and r >= 1):
        raise ValueError("matern32_state_space needs lengthscale > 0, variance > 0, dt > 0 and r >= 1")
    lam = np.sqrt(3.0) / lengthscale
    A2 = np.exp(-lam * dt) * np.array([[1.0 + lam * dt, dt], [-lam * lam * dt, 1.0 - lam * dt]])
    Pinf = np.diag([variance, lam * lam * variance])
    Q2 = Pinf - A2 @ Pinf @ A2.T
    Q2 = 0.5 * (Q2 + Q2.T)
    I = np.eye(r)
    return np.kron(A2, I), np.kron(Q2, I), np.kron(np.array([[1.0, 0.0]]), I)


def _per_replica(a, B, shape, name):
    """`a` as a (B,) + shape float64 array of its own: given once (shape) it is broadcast over the replicas"""
    a = np.asarray(a, dtype=np.float64)
    if a.shape == shape:
        a = np.broadcast_to(a, (B,) + shape)
    if a.shape != (B,) + shape:
        raise ValueError(f"{name} has shape {a.shape}, expected {shape} or {(B,) + shape}")
    return np.array(a, dtype=np.float64, order="C", copy=True)


def _mask_bytes(mask, B, d, n):
    """`mask` (batch, d, n) or (d, n), bool or 0/1 -> (batch, n, d) uint8, time-major like Y; every column needs an observed row"""
    m = np.asarray(mask)
    if m.ndim == 2 and B == 1:
        m = m[None]
    if m.shape != (B, d, n):
        raise ValueError(f"mask has shape {np.shape(mask)}, expected {(B, d, n)}" + (f" or {(d, n)}" if B == 1 else ""))
    if m.dtype != np.bool_:
        if m.dtype.kind not in "iuf" or not np.all((m == 0) | (m == 1)):
            raise ValueError("mask must be bool or hold 0 and 1 only (1 = observed)")
    m = np.ascontiguousarray(np.transpose(m != 0, (0, 2, 1))).astype(np.uint8)
    empty = np.argwhere(m.sum(axis=2) == 0)
    if len(empty):
        raise ValueError(f"no observed row in replica {empty[0][0]}, step {empty[0][1]}: every step needs at least one")
    return m


def linear_psmf_batch(Y, C0, x0, V0, P0, A, Q, H, rho, *, carry_P=True, first_step=True, want_pred=False, device=0, status=True,
                      mask=None, robust=False, lambda0=None, fixed_lambda=False, alpha=1.0, beta=1.0, robust_state=None):
    """Run `batch` independent series through the filter of the module docstring in one launch.

    Reference layouts: Y (batch, d, n) or (d, n) -- a single series is a batch of one --, C0 (batch, d, r), x0 (batch, p); V0 (r, r)
    and P0 (p, p) per replica or given once and broadcast; A (p, p), Q (p, p) symmetric positive definite, H (r, p) and rho >= 0
    (R = rho I) shared by the replicas.  `first_step=False` continues a series: with `carry_P=False` every step of such a call uses
    P_prev = 0.  No argument is modified.

    Returns a dict: X (batch, p, n) the filtered states, C (batch, d, r), V (batch, r, r), P (batch, p, p), x (batch, p) the final
    state (what a continuing call takes), Ypred (batch, d, n) the one-step predictions C z or None, scalars (batch, n, 2) the (s, eta)
    of every step, status (batch,) int32 -- 0, or PSMF_ERR_NUMERIC (-4) for a replica whose r x r system lost positive definiteness or
    whose state is not finite; the others are untouched by it -- and elapsed_ms of the kernel.  `status=None` asks for no per-replica
    status: a failed replica then fails the call (numpy.linalg.LinAlgError).

    With none of `mask`, `robust`, `lambda0`, `fixed_lambda`, `alpha`, `beta`, `robust_state` given the call is psmf_ssm_run.  Otherwise
    it is psmf_ssm_run_ex, the recursion of the module docstring: `mask` (batch, d, n) or (d, n), bool or 0/1, 1 = observed -- Y may hold
    anything, NaN included, where it is 0, and every column needs an observed row; `robust=True` is rPSMF with `lambda0` > 0 degrees
    of freedom at the start of the series (`fixed_lambda=True` keeps them there) and the factors `alpha` of V and `beta` of P;
    `robust_state` (batch, 2) is the (lambda, Omega) a call with `first_step=False` continues from.  Such a call also returns omega
    and phi, each (batch, n) (ones when not robust), and robust_state (batch, 2), (0, 1) when not robust."""
    ex = not (mask is None and robust is False and lambda0 is None and fixed_lambda is False and alpha == 1.0 and beta == 1.0
              and robust_state is None)
    Y = np.asarray(Y, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    if Y.ndim == 2:
        if C0.ndim != 2 or x0.ndim != 1:
            raise ValueError("a single series (2-D Y) takes a (d, r) C0 and a (p,) x0")
        Y, C0, x0 = Y[None], C0[None], x0[None]
    if Y.ndim != 3 or C0.ndim != 3 or x0.ndim != 2:
        raise ValueError("Y must be (batch, d, n) or (d, n), C0 (batch, d, r), x0 (batch, p)")
    B, d, n = Y.shape
    r, p = C0.shape[2], x0.shape[1]
    A, Q, H = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (A, Q, H))
    if C0.shape != (B, d, r) or x0.shape != (B, p) or A.shape != (p, p) or Q.shape != (p, p) or H.shape != (r, p):
        raise ValueError(f"inconsistent shapes: Y {Y.shape}, C0 {C0.shape}, x0 {x0.shape}, A {A.shape}, Q {Q.shape}, H {H.shape} "
                         "(need C0 (batch, d, r), x0 (batch, p), A and Q (p, p), H (r, p))")
    if np.ndim(rho) != 0:
        raise ValueError("rho must be a scalar (R = rho I)")
    Yt = np.ascontiguousarray(np.transpose(Y, (0, 2, 1)))       # time-major: column t of the reference's (d, n) is row t
    Cb = np.array(C0, dtype=np.float64, order="C", copy=True)
    xb = np.array(x0, dtype=np.float64, order="C", copy=True)
    Vb = _per_replica(V0, B, (r, r), "V0")
    Pb = _per_replica(P0, B, (p, p), "P0")
    Xb = np.zeros((B, n, p))
    Yp = np.zeros((B, n, d)) if want_pred else None
    sc = np.zeros((B, n, 4 if ex else 2))
    st = np.zeros(B, dtype=np.int32) if status is not None and status is not False else None
    cfg = _capi.PsmfSsmConfig(abi_version=_capi.ABI_VERSION, d=d, n=n, r=r, p=p, batch=B, device=int(device), carry_P=int(bool(carry_P)),
                              first_step=int(bool(first_step)), want_pred=int(bool(want_pred)))
    ms = C.c_float()
    dp = _capi._ptr
    if ex:
        robust = bool(robust)
        if robust:
            if lambda0 is None or not (np.ndim(lambda0) == 0 and np.isfinite(lambda0) and lambda0 > 0):
                raise ValueError("robust=True needs a finite lambda0 > 0 (the degrees of freedom at the start of the series)")
            if not (np.isfinite(alpha) and alpha > 0 and np.isfinite(beta) and beta > 0):
                raise ValueError("alpha and beta must be finite and > 0")
            if not first_step and robust_state is None:
                raise ValueError("a robust call with first_step=False needs robust_state, the (lambda, Omega) of the previous call")
        elif lambda0 is not None or fixed_lambda or alpha != 1.0 or beta != 1.0 or robust_state is not None:
            raise ValueError("lambda0, fixed_lambda, alpha, beta and robust_state belong to robust=True")
        Mb = None if mask is None else _mask_bytes(mask, B, d, n)
        rs = np.zeros((B, 2))
        rs[:] = (float(lambda0) if robust else 0.0, 1.0)
        if robust and robust_state is not None:
            rs = _per_replica(robust_state, B, (2,), "robust_state")
        cfx = _capi.PsmfSsmConfigEx(abi_version=_capi.ABI_VERSION, d=d, n=n, r=r, p=p, batch=B, device=int(device),
                                    carry_P=int(bool(carry_P)), first_step=int(bool(first_step)), want_pred=int(bool(want_pred)),
                                    robust=int(robust), fixed_lambda=int(bool(fixed_lambda)), lambda0=float(lambda0) if robust else 0.0,
                                    alpha=float(alpha), beta=float(beta))
        name, args = "psmf_ssm_run_ex", (C.byref(cfx), dp(Yt), dp(Mb), dp(Cb), dp(Vb), dp(xb), dp(Pb), dp(A), dp(Q), dp(H), float(rho),
                                         dp(rs) if robust else None, dp(Xb), dp(Yp), dp(sc), dp(st), C.byref(ms))
    else:
        name, args = "psmf_ssm_run", (C.byref(cfg), dp(Yt), dp(Cb), dp(Vb), dp(xb), dp(Pb), dp(A), dp(Q), dp(H), float(rho), dp(Xb), dp(Yp), dp(sc),
                                      dp(st), C.byref(ms))
    lib = _capi.load_library()
    rc = getattr(lib, name)(*args)
    _capi.raise_for(lib, rc, f"{name} failed ({rc})")
    out = dict(X=np.transpose(Xb, (0, 2, 1)), C=Cb, V=Vb, P=Pb, x=xb, Ypred=None if Yp is None else np.transpose(Yp, (0, 2, 1)),
               scalars=sc, status=st, elapsed_ms=ms.value)
    if ex:
        out.update(scalars=np.ascontiguousarray(sc[:, :, :2]), omega=sc[:, :, 2].copy(), phi=sc[:, :, 3].copy(), robust_state=rs)
    return out


def _drop_in(Y, Q, A, R, H, V, P0, C, r, m, n, x0, rng, name, **kw):
    """the Matlab function's arguments -> linear_psmf_batch -> X (p x n)"""
    Y = np.asarray(Y, dtype=np.float64)
    Cm = np.asarray(C, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if Y.shape != (m, n) or Cm.shape != (m, r) or A.ndim != 2:
        raise ValueError("shape mismatch with r, m, n: Y must be (m, n) and C (m, r)")
    if np.ndim(R) == 0:
        rho = float(R)
    else:
        Rm = np.asarray(R, dtype=np.float64)
        if Rm.shape != (m, m) or not np.array_equal(Rm, Rm[0, 0] * np.eye(m)):
            raise NotImplementedError(f"{name} on the device takes R = rho * I (a scalar, or an (m, m) matrix rho * eye(m)): "
                                      "a dense or non-uniform R needs the d x d system this engine never forms")
        rho = float(Rm[0, 0])
    p = A.shape[0]
    if x0 is None:
        rng = np.random.default_rng() if rng is None else rng
        x0 = np.linalg.cholesky(Q) @ rng.standard_normal(p)
    x0 = np.asarray(x0, dtype=np.float64).reshape(p)
    res = linear_psmf_batch(Y, Cm, x0, V, P0, A, Q, H, rho, status=None, **kw)
    return res["X"][0]


def PSMF(r, Y, Q, A, R, H, V, P0, C, X, m, n, x0=None, rng=None, carry_P=False, mask=None):
    """ExperimentChange/PSMF.m:6-45 on the device, with the Matlab function's arguments: Y (m x n), Q and A (p x p), H (r x p),
    V (r x r), P0 (p x p), C (m x r); returns X (p x n), the filtered states.  `X` (the preallocated output of the Matlab call) is not
    read.  The Matlab function draws x0 = chol(Q)' * randn inside; here `x0` is an argument, or is drawn that way from `rng` (a
    numpy Generator; a fresh default_rng() when both are None).  R is the scalar rho or rho * I: the model is S = C P_z C^T + (rho + s) I.

    The default `carry_P=False` is PSMF.m:30 as written -- it predicts from P(:,:,t), which is still zero at that point, so after the
    first step Pbar = Q; `carry_P=True` is the textbook recursion Pbar = A P_{t-1} A^T + Q.  `mask` (m x n, bool or 0/1, 1 = observed)
    marks the entries of Y that exist: the recursion of the module docstring."""
    return _drop_in(Y, Q, A, R, H, V, P0, C, r, m, n, x0, rng, "PSMF", carry_P=carry_P, mask=mask)


def rPSMF(r, Y, Q, A, R, H, V, P0, C, X, m, n, lambda0, x0=None, rng=None, carry_P=False, fixed_lambda=False, mask=None):
    """The robust form of `PSMF(...)`, with the same arguments and conventions and `lambda0` > 0, the degrees of freedom of the
    t-distributed likelihood at the start of the series (`fixed_lambda=True` keeps them; otherwise they grow by m per step):
    the lines marked rob in the module docstring, with alpha = beta = 1.  Returns X (p x n)."""
    return _drop_in(Y, Q, A, R, H, V, P0, C, r, m, n, x0, rng, "rPSMF", carry_P=carry_P, mask=mask, robust=True, lambda0=lambda0,
                    fixed_lambda=fixed_lambda)
