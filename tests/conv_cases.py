"""Models and cases of the convergence experiment (psmf_conv_run, rpsmf_amd/convergence.py; rpsmf_amd/csrc/psmf_conv.hip).  Pure
numpy: tests/test_conv_cases_cpu.py checks the models against the reference's stored run and admits the net without a GPU,
tests/test_hip_convergence.py runs it on the device.

`model(cs, np.float64)` is Convergence/main.m line for line, for all replicas of a case at once (a leading batch axis on every
array): the d x d inverse as the reference writes it (numpy.linalg.inv for Matlab's eye(d) / A), Wasserstein2.m with its two matrix
square roots (of symmetric matrices: through eigh), Matlab's norm of a matrix as the largest singular value.  `model(cs,
np.longdouble)` is the same recursion in extended precision with nothing of LAPACK in it: a Gauss-Jordan inverse, a Cholesky factor
and cyclic Jacobi eigenvalues of its own; trace sqrtm(S1^1/2 S2 S1^1/2) as sum sqrt(eig(L^T S2 L)), S1 = L L^T, and a spectral norm
as sqrt(lambda_max) of the smaller Gram matrix.  The restart is P0 = Pps(:,:,1) (main.m:54 as written is that at r = 1 only).  A W^2
below zero counts as 0 in both (the device's convention; Matlab: a complex W).

The net: SPECS walks the twelve instances (r = 1 .. 4 under the capacities 4, 8, 16) with d at 1, r, 4 | 5, 8 | 9 and 16, n = 2 (only
W(2) exists) and n around 50, 2 .. 6 iterations, batches of 1, 63, 64, 65 (one past the workgroup of 64 lanes) and 129, shared and own
data; every odd case has a non-uniform diagonal R, two cases in three per-replica q_scale and r_scale away from 1, and v spans two
decades over the replicas of every case.  A case is ADMITTED when the float64 model agrees with the extended one to 1e-10 relative
(netlib.relerr) on avW, CerrI, ErM of every iteration and on the final C, Xps, Pps; otherwise it is redrawn from the next sub-seed and
listed in REPLACED (at most a quarter of the cases)."""

from functools import lru_cache

import numpy as np

from netlib import relerr, resolve

SEED = 7301
ADMIT = 1e-10          # float64 model against the extended model
BAR = 1e-9             # the device against the extended model: ten times that -- the device differs from the float64 model in the
#                        order of its operations alone, and the admitted cases bound what an order can do
ADMIT_KEYS = ("avW", "CerrI", "ErM", "C", "Xps", "Pps")

# r, d, n, iterations, batch, own data
SPECS = (
    (1, 1, 2, 2, 1, False), (1, 4, 51, 6, 63, False), (1, 5, 7, 3, 64, True), (1, 8, 50, 2, 2, False), (1, 9, 2, 4, 65, False),
    (1, 16, 12, 2, 3, True), (2, 2, 49, 3, 65, True), (2, 4, 2, 2, 129, False), (2, 5, 50, 4, 1, False), (2, 8, 9, 3, 64, False),
    (2, 9, 50, 2, 4, True), (2, 16, 5, 3, 63, False), (3, 3, 2, 5, 64, False), (3, 4, 50, 2, 5, True), (3, 5, 11, 3, 129, True),
    (3, 8, 52, 3, 2, False), (3, 9, 6, 2, 65, False), (3, 16, 50, 2, 1, True), (4, 4, 50, 3, 63, False), (4, 5, 2, 6, 1, True),
    (4, 8, 50, 2, 65, False), (4, 9, 8, 3, 64, True), (4, 16, 48, 2, 129, False), (4, 16, 2, 2, 65, True),
)

# case number -> sub-seed of the admitted draw (the sub-seeds before it failed the admission of tests/test_conv_cases_cpu.py)
REPLACED = {}


# ---- small dense algebra in any float type, batched over the leading axis
def _t(A):
    return np.swapaxes(A, -1, -2)


def _mv(A, x):
    return np.einsum("...ij,...j->...i", A, x)


def gauss_jordan(A):
    """inverse of the trailing (m, m) matrices, symmetric positive definite (no pivoting), in A's own precision"""
    m = A.shape[-1]
    M = np.concatenate([A.copy(), np.broadcast_to(np.eye(m, dtype=A.dtype), A.shape).copy()], axis=-1)
    for k in range(m):
        M[..., k, :] = M[..., k, :] / M[..., k, k:k + 1]
        for i in range(m):
            if i != k:
                M[..., i, :] = M[..., i, :] - M[..., i, k:k + 1] * M[..., k, :]
    return M[..., m:]


def cholesky(A):
    m = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(m):
        L[..., j, j] = np.sqrt(A[..., j, j] - np.sum(L[..., j, :j] ** 2, axis=-1))
        for i in range(j + 1, m):
            L[..., i, j] = (A[..., i, j] - np.sum(L[..., i, :j] * L[..., j, :j], axis=-1)) / L[..., j, j]
    return L


def jacobi_eigvals(A, sweeps=30):
    """eigenvalues of the trailing symmetric (m, m) matrices by cyclic Jacobi, in A's own precision, ascending"""
    A = A.copy()
    m = A.shape[-1]
    tiny = 100 * np.finfo(A.dtype).eps ** 2        # off-diagonal norm below 10 eps of the diagonal's: the eigenvalues are then exact to eps^2
    for _ in range(sweeps):
        dg = np.sum(np.diagonal(A, axis1=-2, axis2=-1) ** 2, axis=-1)
        off = np.sum(A ** 2, axis=(-2, -1)) - dg
        if np.all(off <= tiny * dg):
            break
        for p in range(m):
            for q in range(p + 1, m):
                apq = A[..., p, q]
                nz = apq != 0
                safe = np.where(nz, apq, 1)
                with np.errstate(over="ignore"):          # (a huge theta: t = 0, the rotation is the identity)
                    theta = (A[..., q, q] - A[..., p, p]) / (2 * safe)
                    t = np.where(theta >= 0, 1, -1) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                t = np.where(nz, t, 0)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                c, s = c[..., None], s[..., None]
                rp, rq = A[..., p, :].copy(), A[..., q, :].copy()
                A[..., p, :], A[..., q, :] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[..., :, p].copy(), A[..., :, q].copy()
                A[..., :, p], A[..., :, q] = c * cp - s * cq, s * cp + c * cq
    return np.sort(np.diagonal(A, axis1=-2, axis2=-1), axis=-1)


def sqrtm_sym(S):
    """sqrtm of symmetric positive semi-definite matrices, float64"""
    w, U = np.linalg.eigh(0.5 * (S + _t(S)))
    return (U * np.sqrt(np.maximum(w, 0.0))[..., None, :]) @ _t(U)


def w2_parts(m1, m2, S1, S2):
    """Wasserstein2.m: (K2, its scale |m1 - m2|^2 + tr S1 + tr S2).  float64: as written; otherwise through the eigenvalue form"""
    dm = m1 - m2
    head = np.sum(dm * dm, axis=-1) + np.trace(S1, axis1=-2, axis2=-1) + np.trace(S2, axis1=-2, axis2=-1)
    if S1.dtype == np.float64:
        S1sq = sqrtm_sym(S1)
        cross = np.trace(sqrtm_sym(S1sq @ S2 @ S1sq), axis1=-2, axis2=-1)
    else:
        L = cholesky(S1)
        cross = np.sum(np.sqrt(np.maximum(jacobi_eigvals(_t(L) @ S2 @ L), 0)), axis=-1)
    return head - 2 * cross, head


def wasserstein2(m1, m2, S1, S2):
    return np.sqrt(np.maximum(w2_parts(m1, m2, S1, S2)[0], 0))


def norm2(A):
    """Matlab's norm of a matrix: the largest singular value"""
    if A.dtype == np.float64:
        return np.linalg.norm(A, ord=2, axis=(-2, -1))
    G = A @ _t(A) if A.shape[-2] <= A.shape[-1] else _t(A) @ A
    return np.sqrt(np.maximum(jacobi_eigvals(G)[..., -1], 0))


def inverse(A):
    return np.linalg.inv(A) if A.dtype == np.float64 else gauss_jordan(A)


# ---- the experiment
def kalman(Y, Ct, Q, R, x0, P0):
    """main.m:15-34.  Y (B, d, n), Ct (B, d, r), Q (r, r), R (d, d), x0 (B, r), P0 (B, r, r) -> Xk (B, r, n), Pk (B, r, r, n)"""
    B, d, n = Y.shape
    r = Ct.shape[-1]
    Xk, Pk = np.zeros((B, r, n), dtype=Y.dtype), np.zeros((B, r, r, n), dtype=Y.dtype)
    x, P = x0, P0
    for t in range(n):
        Pp = P + Q
        S = inverse(R + Ct @ Pp @ _t(Ct))
        G = Pp @ _t(Ct) @ S
        x = x + _mv(G, Y[:, :, t] - _mv(Ct, x))
        P = Pp - G @ Ct @ Pp
        Xk[:, :, t], Pk[:, :, :, t] = x, P
    return Xk, Pk


def iterate(Y, Ct, Q, R, C, X0, P0, v, qs, rs, Xk, Pk, n_iter):
    """main.m:49-108, n_iter times.  Per-replica v, q_scale, r_scale (B,); returns the record of the module docstring's quantities
    (V: that of the end of the last iteration)"""
    B, d, n = Y.shape
    r = C.shape[-1]
    ft = Y.dtype
    I_r, I_d = np.eye(r, dtype=ft), np.eye(d, dtype=ft)
    Qs, Rs = qs[:, None, None] * Q, rs[:, None, None] * R
    avW, CerrI, ErM = (np.zeros((B, n_iter), dtype=ft) for _ in range(3))
    W, W2, W2s, Cerr = (np.zeros((B, n), dtype=ft) for _ in range(4))
    Xps, Pps = np.zeros((B, r, n), dtype=ft), np.zeros((B, r, r, n), dtype=ft)
    for it in range(n_iter):
        V = v[:, None, None] * I_r
        xp, Pv = X0, P0
        for t in range(n):
            Pp = Pv + Qs
            s = np.sum(xp * _mv(V, xp), axis=-1)
            CPC = C @ Pp @ _t(C)
            eta = np.trace(Rs + CPC, axis1=-2, axis2=-1) / d
            S = inverse(Rs + I_d * s[:, None, None] + CPC)
            e = Y[:, :, t] - _mv(C, xp)
            G = Pp @ _t(C) @ S
            x = xp + _mv(G, e)
            P = Pp - G @ C @ Pp
            N = (s + eta)[:, None, None]
            C = C + (e[:, :, None] * _mv(V, xp)[:, None, :]) / N              # (V is symmetric: xp^T V = (V xp)^T)
            V = V - (V @ (xp[:, :, None] * xp[:, None, :]) @ V) / N
            Cerr[:, t] = norm2(C - Ct)
            if t >= 1:
                W2[:, t], W2s[:, t] = w2_parts(x, Xk[:, :, t], P, Pk[:, :, :, t])
                W[:, t] = np.sqrt(np.maximum(W2[:, t], 0))
            Xps[:, :, t], Pps[:, :, :, t] = x, P
            xp, Pv = x, P
        ErM[:, it] = norm2(Y - C @ Xps)
        avW[:, it] = np.mean(W, axis=-1)
        CerrI[:, it] = norm2(C - Ct)
        X0, P0 = Xps[:, :, 0].copy(), Pps[:, :, :, 0].copy()
    return dict(avW=avW, CerrI=CerrI, ErM=ErM, W=W, W2=W2, W2scale=W2s, Cerr=Cerr, Xps=Xps, Pps=Pps, C=C, x0=X0, P0=P0, V=V)


def model(cs, ft=np.float64, n_iter=None):
    """the whole run of a case (Kalman pass, then the iterations) in the float type `ft`"""
    a = {k: np.asarray(cs[k], dtype=ft) for k in ("Y", "Ctrue", "Q", "Rdiag", "C0", "x0", "P0", "x0k", "P0k", "v", "q_scale", "r_scale")}
    B = cs["B"]
    full = lambda x, shape: np.broadcast_to(x, (B,) + shape).copy()
    Y, Ct = full(a["Y"], (cs["d"], cs["n"])), full(a["Ctrue"], (cs["d"], cs["r"]))
    R = np.diag(a["Rdiag"])
    Xk, Pk = kalman(Y, Ct, a["Q"], R, full(a["x0k"], (cs["r"],)), full(a["P0k"], (cs["r"], cs["r"])))
    out = iterate(Y, Ct, a["Q"], R, a["C0"], a["x0"], a["P0"], a["v"], a["q_scale"], a["r_scale"], Xk, Pk, n_iter or cs["n_iter"])
    out.update(Xk=Xk, Pk=Pk)
    return out


# ---- the net
def draw(i, sub=0):
    r, d, n, n_iter, B, own = SPECS[i]
    rng = np.random.default_rng([SEED, i, sub])
    nser = B if own else 1
    Qh = rng.standard_normal((r, r))
    Q = 0.02 * (np.eye(r) + 0.3 * Qh @ Qh.T / r)
    Q = 0.5 * (Q + Q.T)
    Rdiag = 0.1 * np.exp(rng.uniform(-1.0, 1.0, d)) if i % 2 else np.full(d, 0.1)
    Ctrue = 2.0 * np.abs(rng.standard_normal((nser, d, r))) + 0.5
    X = np.cumsum(np.linalg.cholesky(Q) @ rng.standard_normal((nser, r, n)), axis=2) + rng.standard_normal((nser, r, 1))
    Y = Ctrue @ X + np.sqrt(Rdiag)[None, :, None] * rng.standard_normal((nser, d, n))
    x0k = rng.standard_normal((nser, r))
    P0k = 2.0 * np.exp(rng.uniform(-0.5, 0.5, (nser, 1, 1))) * np.eye(r)
    C0 = 3.0 * np.abs(rng.standard_normal((B, d, r))) + 0.2
    x0 = 2.0 * rng.standard_normal((B, r))
    P0 = 5.0 * np.exp(rng.uniform(-0.5, 0.5, (B, 1, 1))) * np.eye(r)
    v = 10.0 ** rng.uniform(-1.0, 1.0, B)
    scaled = i % 3 != 0
    q_scale = np.exp(rng.uniform(-1.0, 1.0, B)) if scaled else np.ones(B)
    r_scale = np.exp(rng.uniform(-1.0, 1.0, B)) if scaled else np.ones(B)
    sq = (lambda a: a) if own else (lambda a: a[0])
    return dict(i=i, sub=sub, r=r, d=d, n=n, n_iter=n_iter, B=B, own=own, Q=Q, Rdiag=Rdiag, Ctrue=sq(Ctrue), Y=sq(Y), x0k=sq(x0k), P0k=sq(P0k),
                C0=C0, x0=x0, P0=P0, v=v, q_scale=q_scale, r_scale=r_scale)


def describe(cs):
    return f"r={cs['r']} d={cs['d']} n={cs['n']} iters={cs['n_iter']} batch={cs['B']} {'own' if cs['own'] else 'shared'}"


def admissible(cs):
    m64, mx = model(cs, np.float64), model(cs, np.longdouble)
    worst = max((relerr(m64[k], mx[k]), k) for k in ADMIT_KEYS)
    finite = all(np.all(np.isfinite(np.asarray(mx[k], dtype=float))) for k in ADMIT_KEYS)
    return finite and worst[0] <= ADMIT, f"float64 against extended: {worst[0]:.2e} on {worst[1]}"


def resolve_case(i):
    """((sub-seed, 0), the log of the draws that were not admitted) of case i, computed"""
    return resolve(i, draw, None, admissible, describe)


@lru_cache(maxsize=None)
def device_case(i):
    """case i as the device runs it, with its extended-precision record under "ref" (as float64)"""
    cs = draw(i, REPLACED.get(i, 0))
    cs["ref"] = {k: np.asarray(a, dtype=np.float64) for k, a in model(cs, np.longdouble).items()}
    return cs


def instance(cs):
    """(r, capacity) of the kernel that runs the case"""
    return cs["r"], next(c for c in (4, 8, 16) if cs["d"] <= c)
