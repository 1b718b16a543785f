"""numpy restatement of ExperimentImpute/BPMF.py:121-302 on pre-drawn numbers, the model every test of rpsmf_amd.bpmf is judged against.

`bpmf_model` with algebra="reference" is the reference's arithmetic line for line -- the same expressions in the same order, `inv` and
`cholesky` included -- with three changes that move no bit: every random number is an argument (rpsmf_amd.bpmf.draw_bpmf makes them
with the reference's numpy calls in the reference's order; the Wishart draw is scipy's C A A^T C^T on the pre-drawn standard Bartlett
factor A); the warm start is tests/pmf_model.py, which is BPMF.py:43-105; and the "simple fit" of BPMF.py:197-201 is left out, every
value of it being overwritten before use.

algebra="device" is the factor form the kernels use, the hyper step included: a precision matrix is factored L = U U^T from the last
row upwards (U upper triangular: the Cholesky factor of the matrix with rows and columns reversed, reversed back), and
cholesky(inv L).T z + inv(L) b becomes U^-1 z + U^-T U^-1 b -- U^-T is the lower Cholesky factor of inv(L) -- with no inverse
anywhere; the Grams of all columns (rows) of a sweep are one matrix product.  order="reversed" sums every Gram and right-hand side
over the observed entries in the opposite order.  How far the four combinations part measures what the result owes to the algebra
and to the order of its sums, which is all that a device implementation is free to choose.

dtype=np.longdouble (algebra="device" only: numpy.linalg takes no long doubles, and that form needs no inverse) is the
extended-precision model: the same steps on the same float64 inputs with every array, constant and accumulator a long double, the
reverse Cholesky factorisation and the two triangular solves written out below as loops over the <= 16 features, vectorised over
the columns (rows) of a sweep.  dtype=float moves no bit of what the functions gave before they had the argument.

factors=(W, P), (n, r) and (d, r): the sampler alone -- the warm start is skipped and the sweeps start from these; mean and
mean_rating are still taken from the data."""

import numpy as np

import pmf_model

B0 = 2      # b0_u = b0_m, BPMF.py:152-158


def _rmsem(Yrec2, YorigInt, Mmiss):
    """common.py:79-84"""
    nMissing = np.sum(Mmiss)
    R2 = (Yrec2.dtype.type(1) / nMissing) * np.sum(np.power(np.multiply(Yrec2, Mmiss) - np.multiply(YorigInt, Mmiss), 2))
    return np.sqrt(R2)


def revchol(L):
    """U, upper triangular with L = U U^T (stacks of matrices too); numpy.linalg.LinAlgError where L is not positive definite"""
    if L.dtype == np.longdouble:
        return _revchol_loops(L)
    return np.linalg.cholesky(L[..., ::-1, ::-1])[..., ::-1, ::-1]


def _revchol_loops(L):
    """revchol by hand, for the dtypes numpy.linalg does not take: column k of U from the last one upwards, then the rank-one
    update of the leading k x k block"""
    A = np.array(L, copy=True)
    r = A.shape[-1]
    U = np.zeros_like(A)
    for k in range(r - 1, -1, -1):
        piv = A[..., k, k]
        if not np.all(piv > 0):
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        ukk = np.sqrt(piv)
        col = A[..., :k, k] / ukk[..., None]
        U[..., :k, k] = col
        U[..., k, k] = ukk
        A[..., :k, :k] -= col[..., :, None] * col[..., None, :]
    return U


def _solve_upper(U, B):
    """X with U X = B for upper triangular U (..., r, r) and B (..., r, c), from the last row upwards"""
    if U.dtype != np.longdouble:
        return np.linalg.solve(U, B)
    r = U.shape[-1]
    X = np.zeros_like(B)
    for k in range(r - 1, -1, -1):
        X[..., k, :] = (B[..., k, :] - np.sum(U[..., k, k + 1:, None] * X[..., k + 1:, :], axis=-2)) / U[..., k, k, None]
    return X


def _solve_upper_t(U, B):
    """X with U^T X = B, from the first row downwards"""
    if U.dtype != np.longdouble:
        return np.linalg.solve(np.swapaxes(U, -1, -2), B)
    r = U.shape[-1]
    X = np.zeros_like(B)
    for i in range(r):
        X[..., i, :] = (B[..., i, :] - np.sum(U[..., :i, i, None] * X[..., :i, :], axis=-2)) / U[..., i, i, None]
    return X


def _hyper(F, A, z, algebra):
    """BPMF.py:209-225 (= 228-243) for one side: (alpha, mu)"""
    num_feat = F.shape[1]
    WI = np.eye(num_feat)
    mu0 = np.zeros((num_feat, 1))
    b0 = B0
    N = F.shape[0]
    x_bar = np.mean(F, axis=0).reshape(num_feat, 1)
    S_bar = np.cov(F, rowvar=False)
    T = (np.linalg.inv(WI) if F.dtype != np.longdouble else WI) + N / 1 * S_bar + N * b0 * (mu0 - x_bar) @ (mu0 - x_bar).T / (1 * (b0 + N))
    mu_temp = (b0 * mu0 + N * x_bar) / (b0 + N)
    if algebra == "reference":
        WI_post = np.linalg.inv(T)
        WI_post = (WI_post + WI_post.T) / 2
        CA = np.dot(np.linalg.cholesky(WI_post), A)      # scipy.stats.wishart.rvs(df, WI_post) on its standard factor A
        alpha = np.dot(CA, CA.T)
        lam = np.linalg.cholesky(np.linalg.inv((b0 + N) * alpha))
        lam = lam.T
        mu = lam @ z + mu_temp
    else:
        U = revchol(T)
        CA = _solve_upper_t(U, A)
        alpha = CA @ CA.T
        V = revchol((b0 + N) * alpha)
        mu = _solve_upper(V, z) + mu_temp
    return alpha, mu


def _sweep_reference(F_out, F_in, obs, resid, alpha, mu, beta, Z, order):
    """BPMF.py:249-262 (= 266-279): F_out[k] for every k, from the rows of F_in that obs[:, k] selects; resid[:, k] = count - mean_rating"""
    num_feat = F_in.shape[1]
    for k in range(F_out.shape[0]):
        ff = np.nonzero(obs[:, k])[0]
        if order == "reversed":
            ff = ff[::-1]
        MM = F_in[ff, :]
        rr = np.expand_dims(resid[ff, k], 1)
        covar = np.linalg.inv(alpha + beta * MM.T @ MM)
        mean = covar @ (beta * MM.T @ rr + alpha @ mu)
        lam = np.linalg.cholesky(covar).T
        F_out[k, :] = (lam @ Z[k].reshape(num_feat, 1) + mean).squeeze()


def _sweep_device(F_out, F_in, obs, resid, alpha, mu, beta, Z, order):
    num_feat = F_in.shape[1]
    if order == "reversed":
        F_in, obs, resid = F_in[::-1], obs[::-1], resid[::-1]
    o = obs.astype(F_in.dtype)
    outer = (F_in[:, :, None] * F_in[:, None, :]).reshape(F_in.shape[0], num_feat * num_feat)
    gram = (o.T @ outer).reshape(-1, num_feat, num_feat)
    rhs = (o * resid).T @ F_in
    L = alpha[None] + beta * gram
    b = beta * rhs + (alpha @ mu).T
    U = revchol(L)
    t = _solve_upper(U, np.stack([Z, b], axis=2))                         # U^-1 z and U^-1 b
    x = _solve_upper_t(U, t[:, :, 1:2])                                   # U^-T U^-1 b
    F_out[:, :] = t[:, :, 0] + x[:, :, 0]


def bpmf_model(YorigInt, M, Mmiss, C, X, draws, epochs=2, beta=2, algebra="reference", order="reference", warm_start=None, dtype=float,
               factors=None):
    """Returns dict(Efull (epochs,), P (d, r), W (n, r), Yrec (d, n) of the last epoch, mean, mean_rating).  `draws`: what
    rpsmf_amd.bpmf.draw_bpmf returns; warm_start: keywords of pmf_model (epsilon, lmd, momentum, num_batches); dtype and factors:
    the module docstring (with factors, C, X and the permutations of `draws` are not used).  Raises numpy.linalg.LinAlgError where
    the reference does."""
    assert algebra in ("reference", "device") and order in ("reference", "reversed")
    assert dtype is float or algebra == "device", "the extended model is the factor form: numpy.linalg takes no long doubles"
    YorigInt = np.asarray(YorigInt, dtype=dtype)
    M, Mmiss = np.asarray(M), np.asarray(Mmiss)
    Y = YorigInt * M
    num_p, num_m = Y.shape
    tr_p, tr_m = pmf_model.training_set(M)
    if factors is None:
        ws = pmf_model.pmf_model(YorigInt, M, Mmiss, C, X, draws["perms"], epochs=epochs, dtype=dtype, **(warm_start or {}))
        w1_M1_sample, w1_P1_sample = np.array(ws["W"]), np.array(ws["P"])
        old_mean = old_std = ws["mean"]
        mean_rating = ws["mean_rating"]
    else:
        w1_M1_sample, w1_P1_sample = np.array(factors[0], dtype=dtype), np.array(factors[1], dtype=dtype)
        rating_all = Y[tr_p, tr_m]                                            # pmf_model's mu and mbar
        old_mean = old_std = np.mean(rating_all)
        mean_rating = ((rating_all - old_mean) / old_std).mean()
    beta = dtype(beta)
    pr_p, pr_m = np.nonzero((Mmiss > 0.95) & (Mmiss < 1.05))
    count = np.zeros((num_p, num_m), dtype=dtype)
    count[tr_p, tr_m] = (Y[tr_p, tr_m] - old_mean) / old_std
    resid = count - mean_rating
    obs = M > 0
    sweep = _sweep_reference if algebra == "reference" else _sweep_device
    bart, hz, Z = (np.asarray(draws[k], dtype=dtype) for k in ("bartlett", "hyper_normals", "normals"))

    def pred():
        return np.sum(w1_M1_sample[pr_m, :] * w1_P1_sample[pr_p, :], axis=1) + mean_rating

    probe_rat_all = pred()
    counter_prob = 1
    Efull = np.zeros(epochs, dtype=dtype)
    Yrec2 = np.zeros_like(Y)
    for epoch in range(epochs):
        alpha_m, mu_m = _hyper(w1_M1_sample, bart[epoch, 0], hz[epoch, 0].reshape(-1, 1), algebra)
        alpha_u, mu_u = _hyper(w1_P1_sample, bart[epoch, 1], hz[epoch, 1].reshape(-1, 1), algebra)
        for gibbs in range(2):
            sweep(w1_M1_sample, w1_P1_sample, obs, resid, alpha_m, mu_m, beta, Z[epoch, gibbs, :num_m], order)
            sweep(w1_P1_sample, w1_M1_sample, obs.T, resid.T, alpha_u, mu_u, beta, Z[epoch, gibbs, num_m:], order)
        probe_rat = pred()
        probe_rat_all = (counter_prob * probe_rat_all + probe_rat) / (counter_prob + 1)
        counter_prob += 1
        pred_out = probe_rat_all * old_std + old_mean
        Yrec2 = np.zeros_like(Y)
        Yrec2[pr_p, pr_m] = pred_out
        Efull[epoch] = _rmsem(Yrec2, YorigInt, Mmiss)
    return dict(Efull=Efull, P=w1_P1_sample, W=w1_M1_sample, Yrec=Yrec2, mean=old_mean, mean_rating=mean_rating)
