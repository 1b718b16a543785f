"""What kind of R and Q a filter object was given, as the device sees them: functions of (R, Q, d, r, T), no state.  psmf.py calls them
once per object (the structure of R) or once per epoch (the schedules)."""

import numpy as np


def diag_of(R, d):
    """diag(R) as scalar or (d,) vector, or None if R is a non-diagonal d x d matrix.  Accepted shapes: scalar, (1,),
    (1, 1), (d,), (d, 1), (1, d), (d, d); anything else raises (a silently broadcast R would give wrong numbers)."""
    if np.ndim(R) == 0:
        return float(R)
    R = np.asarray(R)
    if R.size == 1:
        return float(R.reshape(()))
    if R.shape in ((d,), (d, 1), (1, d)):
        return R.reshape(-1).astype(float)
    if R.shape != (d, d):
        raise ValueError(f"R has shape {R.shape}: expected a scalar, a (d,) diagonal or a (d, d) matrix with d = {d}")
    dg = np.diagonal(R)
    if np.count_nonzero(R) != np.count_nonzero(dg):
        return None
    return dg.astype(float)


def as_scalar_if_uniform(rho):
    if np.ndim(rho) == 0:
        return float(rho)
    rho = np.asarray(rho)
    return float(rho[0]) if np.all(rho == rho[0]) else None


def structure_of(R, d):
    """(dense, rows) of the R a handle is given whole.
    dense: (lam, U) of a NON-DIAGONAL R = U diag(lam) U^T (the reference's dense branch, psmf.py:150-152) or None.  The device
    keeps the series and C in the eigenbasis of R, where the step is the non-uniform-diagonal one (psmf_set_noise_rotation);
    the O(d^3) symmetric eigen-decomposition is done once, here, by LAPACK.
    rows: diag(R) as a (d,) vector when R is a NON-uniform diagonal (the device then weights every row, per-step engine), else None;
    a non-diagonal R is diagonal in its eigenbasis, where the device works: lam."""
    dg = diag_of(R, d)
    if dg is not None:
        return None, (None if (np.ndim(dg) == 0 or as_scalar_if_uniform(dg) is not None) else np.asarray(dg, dtype=float))
    R = np.asarray(R, dtype=float)          # (diag_of: a d x d matrix with entries off the diagonal)
    if not np.allclose(R, R.T, rtol=1e-12, atol=1e-14 * np.max(np.abs(R))):
        raise NotImplementedError("the device path needs a symmetric R (a covariance); use backend='numpy'")
    lam, U = np.linalg.eigh(0.5 * (R + R.T))
    if lam[0] < -1e-12 * max(lam[-1], 0.0) or not lam[-1] > 0.0:
        raise NotImplementedError("the device path needs a positive semi-definite R (a covariance); use backend='numpy'")
    lam = np.maximum(lam, 0.0)
    return (lam, np.ascontiguousarray(U)), lam


def rho_of(Rk, d, first_R, dense, rows):
    """The scalar rho the device takes for R_k: R_k = rho I, or 1.0 in front of the ONE constant matrix the handle was given whole
    (`first_R`, and its `dense`, `rows` = structure_of(first_R, d))."""
    dg = diag_of(Rk, d)
    rho = None if dg is None else as_scalar_if_uniform(dg)
    if rho is None:
        if dg is not None and dense is None and np.array_equal(dg, rows):
            return 1.0          # the scalar in front of diag(rho_rows) (psmf_set_row_noise)
        if dg is None and dense is not None and (Rk is first_R or np.array_equal(Rk, first_R)):
            return 1.0          # the scalar in front of U diag(lam) U^T (psmf_set_noise_rotation)
        raise NotImplementedError("the device path needs R_k = rho_k * I, or ONE constant matrix R (a non-uniform diagonal or a "
                                  "symmetric positive semi-definite dense matrix); use backend='numpy'")
    return rho


def q_matrix(Qk, r):
    Q = np.asarray(Qk, dtype=float)
    return float(Q) * np.eye(r) if Q.ndim == 0 else Q.reshape(r, r)


def rho_q_schedules(R, Q, T, r, off, rho_of_R):
    """(rho, Q, rho_sched, q_sched) for the device from R[k], Q[k] of step k (psmf.py:115,123,141); `rho_of_R(R_k)` as rho_of above.
    Constant dictionaries give (rho, Q, None, None); R_k = rho_k I and Q_k = q_k Q_1 give per-step scalar schedules
    (index k, entry 0 unused); a Q[k] that is not a multiple of Q[1] returns q_sched = "host" (the host-stepped mode
    forms P_bar itself and takes any Q[k]).  `off`: which R a step reads: 0 = the full filter's R[k] (psmf.py:123,141); 1 = the
    simplified hooks' R[k - 1] (synthetic_psmf.py:86-87: eta = tr(R[k-1]) / d).  The device applies rho_sched[k] at step k either way."""
    ks = list(range(1, (T or 0) + 1))
    if not isinstance(R, dict):
        R = {k: R for k in [0] + ks}
    if not isinstance(Q, dict):
        Q = {k: Q for k in [0] + ks}
    k1 = (1 - off) if (1 - off) in R else min(R.keys())
    rho1 = rho_of_R(R[k1])
    kq1 = 1 if 1 in Q else min(Q.keys())
    Q1 = q_matrix(Q[kq1], r)
    rho_s = q_s = None
    seen_R, seen_Q = {id(R[k1]): rho1}, {}
    for k in ks:
        Rk = R.get(k - off, R[k1])    # (a dictionary without the step's key: the constant it was built from)
        if id(Rk) not in seen_R:
            seen_R[id(Rk)] = rho_of_R(Rk)
        rk = seen_R[id(Rk)]
        if rk != rho1 and rho_s is None:
            rho_s = np.full(len(ks) + 1, rho1)
        if rho_s is not None:
            rho_s[k] = rk
        Qk = Q.get(k, Q[kq1])
        if id(Qk) not in seen_Q:
            Qm = q_matrix(Qk, r)
            if np.array_equal(Qm, Q1):
                seen_Q[id(Qk)] = 1.0
            else:
                nz = np.flatnonzero(Q1)
                c = Qm.reshape(-1)[nz[0]] / Q1.reshape(-1)[nz[0]] if nz.size else np.nan
                seen_Q[id(Qk)] = float(c) if np.isfinite(c) and np.allclose(Qm, c * Q1, rtol=1e-14, atol=0.0) else "host"
        qk = seen_Q[id(Qk)]
        if qk == "host":
            q_s = "host"
        elif not isinstance(q_s, str):
            if qk != 1.0 and q_s is None:
                q_s = np.ones(len(ks) + 1)
            if q_s is not None:
                q_s[k] = qk
    return rho1, Q1, rho_s, q_s


def q_matrices(Q, T, r):
    """Q[k], k = 0..T, as one [T + 1, r, r] stack (entry 0 = Q[1], unused by the device): psmf_set_q_matrix_schedule."""
    k1 = 1 if 1 in Q else min(Q.keys())
    out = np.empty((T + 1, r, r))
    out[0] = q_matrix(Q[k1], r)
    for k in range(1, T + 1):
        out[k] = q_matrix(Q.get(k, Q[k1]), r)
    return out
