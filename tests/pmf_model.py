"""numpy restatement of ExperimentImpute/PMF.py:43-159, the model every test of rpsmf_amd.pmf is judged against.

`pmf_model` is the reference's arithmetic line for line -- the same expressions in the same order -- with two changes that move no
bit: the permutation of an epoch is an index drawn as np.random.permutation(N) and applied to the list of entries (the reference
shuffles the N x 3 array of triplets, which draws the same index), and the scatter loop over the entries of a batch (PMF.py:128-130) is
np.add.at, which adds the rows in the same order.  The permutations are an argument.

order="sorted" is a second summation order: the entries of a batch sorted by their position in the training set, and the penalty
pulled out of the sum (lmd c w instead of c times + lmd w).  How far the two part measures how much the result depends on the order
of its sums, which is all that a device implementation is free to choose."""

import numpy as np


def training_set(M):
    """(rows, columns) of the entries with M == 1 in row-major order, as the reference's double loop collects them"""
    return np.nonzero(np.asarray(M) == 1)


def draw_perms(N, epochs):
    """the permutations pmf() draws from the global RNG, in its order"""
    return [np.random.permutation(N) for _ in range(epochs)]


def pmf_model(YorigInt, M, Mmiss, C, X, perms, epochs=2, epsilon=50, lmd=0.01, momentum=0.8, num_batches=9, order="reference", dtype=float):
    """Returns dict(Efull (epochs,), P (d, r), W (n, r), Yrec (d, n) of the last epoch, mean, mean_rating).  dtype=np.longdouble is
    the extended-precision model: the same expressions on the same (float64) inputs, with every array, constant and accumulator a
    long double -- the data, the 0.1 of the scaling, lmd, momentum, epsilon, the means, the scatter and the error.  dtype=float
    moves no bit of what the function gave before it had the argument."""
    YorigInt = np.asarray(YorigInt, dtype=dtype)
    M, Mmiss = np.asarray(M), np.asarray(Mmiss)
    C, X = np.asarray(C, dtype=dtype), np.asarray(X, dtype=dtype)
    epsilon, lmd, momentum = dtype(epsilon), dtype(lmd), dtype(momentum)
    Y = YorigInt * M
    num_p, num_m = Y.shape
    num_feat = C.shape[1]
    w1_M1 = dtype(0.1) * X.T
    w1_P1 = dtype(0.1) * C
    w1_M1_inc = np.zeros_like(w1_M1)
    w1_P1_inc = np.zeros_like(w1_P1)
    tr_p, tr_m = training_set(M)
    rating_all = Y[tr_p, tr_m]
    pr_p, pr_m = np.nonzero((Mmiss > 0.95) & (Mmiss < 1.05))

    old_mean = np.mean(rating_all)
    old_std = np.mean(rating_all)
    rating_all = (rating_all - old_mean) / old_std
    mean_rating = rating_all.mean()

    Efull = np.zeros(epochs, dtype=dtype)
    Yrec2 = np.zeros_like(Y)
    order_idx = np.arange(rating_all.size)
    with np.errstate(all="ignore"):
        for epoch in range(epochs):
            order_idx = order_idx[np.asarray(perms[epoch])]
            for batch_idx in np.array_split(order_idx, num_batches):
                if order == "sorted":
                    batch_idx = np.sort(batch_idx)
                N = batch_idx.shape[0]
                aa_p = tr_p[batch_idx]
                aa_m = tr_m[batch_idx]
                rating = rating_all[batch_idx] - mean_rating
                pred_out = np.sum(w1_M1[aa_m, :] * w1_P1[aa_p, :], axis=1)
                IO = np.tile(2 * (pred_out - rating).reshape(N, 1), (1, num_feat))
                dw1_M1 = np.zeros((num_m, num_feat), dtype=dtype)
                dw1_P1 = np.zeros((num_p, num_feat), dtype=dtype)
                if order == "sorted":
                    np.add.at(dw1_M1, aa_m, IO * w1_P1[aa_p, :])
                    np.add.at(dw1_P1, aa_p, IO * w1_M1[aa_m, :])
                    dw1_M1 += (lmd * np.bincount(aa_m, minlength=num_m))[:, None] * w1_M1
                    dw1_P1 += (lmd * np.bincount(aa_p, minlength=num_p))[:, None] * w1_P1
                else:
                    Ix_m = IO * w1_P1[aa_p, :] + lmd * w1_M1[aa_m, :]
                    Ix_p = IO * w1_M1[aa_m, :] + lmd * w1_P1[aa_p, :]
                    np.add.at(dw1_M1, aa_m, Ix_m)
                    np.add.at(dw1_P1, aa_p, Ix_p)
                w1_M1_inc = momentum * w1_M1_inc + epsilon * dw1_M1 / N
                w1_M1 = w1_M1 - w1_M1_inc
                w1_P1_inc = momentum * w1_P1_inc + epsilon * dw1_P1 / N
                w1_P1 = w1_P1 - w1_P1_inc
            pred_out = np.sum(w1_M1[pr_m, :] * w1_P1[pr_p, :], axis=1) + mean_rating
            pred_out = pred_out * old_std + old_mean
            Yrec2 = np.zeros_like(Y)
            Yrec2[pr_p, pr_m] = pred_out
            # RMSEM(Yrec2, YorigInt, Mmiss), common.py:79-84
            nMissing = np.sum(Mmiss)
            R2 = (dtype(1) / nMissing) * np.sum(np.power(np.multiply(Yrec2, Mmiss) - np.multiply(YorigInt, Mmiss), 2))
            Efull[epoch] = np.sqrt(R2)
    return dict(Efull=Efull, P=w1_P1, W=w1_M1, Yrec=Yrec2, mean=old_mean, mean_rating=mean_rating)
