"""The PMF baseline of the imputation experiment (ExperimentImpute/PMF.py:43-159) on the device: probabilistic matrix factorisation by
mini-batch gradient descent with momentum on the observed entries, for a batch of independent replicas in one call (psmf_pmf_run,
include/psmf_hip.h: d <= 512, r <= 16, n unlimited), float64 throughout.

Per replica, with T = {(i, j): M_ij = 1} the training entries in row-major order and N = |T|:

    mu = mean over T of y_ij,   v_ij = (y_ij - mu) / mu   (the reference divides by the mean, PMF.py:93-95),   mbar = mean over T of v_ij
    P = 0.1 C0 (d x r),   W = 0.1 X0^T (n x r),   incP = incW = 0
    epoch e = 1 .. epochs:   order_e = order_{e-1}[pi_e],  order_0 = 0 .. N-1,  pi_e = numpy.random.permutation(N); the batches are
        numpy.array_split(order_e, num_batches)
      batch b with N_b entries, everything from the W, P at the start of the batch:
        g_ij = 2 (w_j . p_i - (v_ij - mbar)),   dW_j = sum_i g_ij p_i + lmd c_j w_j,   dP_i = sum_j g_ij w_j + lmd c_i p_i
        incW = momentum incW + epsilon dW / N_b,  W -= incW   (the same for P; c_j, c_i = batch entries of column j / row i)
      end of the epoch, over the probe entries (Mmiss_ij = 1):   yhat_ij = (w_j . p_i + mbar) mu + mu,
        Efull[e] = sqrt(sum (yhat_ij - YorgInt_ij)^2 / sum Mmiss)

The only random input is the permutation of every epoch, which the host draws (or is given); mu and mbar are taken with numpy, so
they carry the reference's bits.  What the device is handed per replica and epoch is a batch map -- n x d bytes, the batch index of a
training entry and 255 elsewhere: the order inside a batch only orders sums.  There is no CPU fallback.

`pmf` keeps the reference function's signature and consumes the global numpy RNG as the reference does.  BPMF (BPMF.py) is
rpsmf_amd.bpmf: its pmf() warm start is this recursion, and `pmf_batch` returns the factors.
"""

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _capi

__all__ = ["pmf_batch", "pmf"]

MAX_D, MAX_R, MAX_BATCHES = 512, 16, 254        # psmf_pmf_run's limits
NO_ENTRY = 255                                  # the batch map's byte of an entry outside the training set
PREPARE_THREADS = 8                             # host threads that build the maps of the replicas


def _zero_one(a, name):
    a = np.asarray(a)
    if not np.all((a == 0) | (a == 1)):
        raise ValueError(f"{name} must hold 0 and 1 only")
    return a != 0


def _batch_sizes(N, nb):
    """the lengths numpy.array_split gives: the first N mod nb batches hold one entry more"""
    return np.full(nb, N // nb, dtype=np.int64) + (np.arange(nb) < N % nb)


def _shapes(YorgInt, M, Mmiss, C0, X0):
    """The arrays with the batch dimension in front, and (d, n, r, B); ValueError where the shapes do not fit each other."""
    YorgInt = np.asarray(YorgInt, dtype=np.float64)
    M, Mmiss = np.asarray(M), np.asarray(Mmiss)
    C0, X0 = np.asarray(C0, dtype=np.float64), np.asarray(X0, dtype=np.float64)
    if YorgInt.ndim != 2:
        raise ValueError("inconsistent shapes: YorgInt must be (d, n)")
    d, n = YorgInt.shape
    if M.ndim == 2:
        M, Mmiss, C0, X0 = M[None], Mmiss[None], C0[None], X0[None]
    if M.ndim != 3 or C0.ndim != 3 or X0.ndim != 3:
        raise ValueError("inconsistent shapes: M, Mmiss (batch, d, n); C0 (batch, d, r); X0 (batch, r, n)")
    B, r = M.shape[0], C0.shape[2]
    if B < 1 or d < 1 or n < 1 or M.shape != (B, d, n) or Mmiss.shape != (B, d, n) or C0.shape != (B, d, r) or X0.shape != (B, r, n):
        raise ValueError("inconsistent shapes: YorgInt (d, n); M, Mmiss (batch, d, n); C0 (batch, d, r); X0 (batch, r, n)")
    return YorgInt, M, Mmiss, C0, X0, (d, n, r, B)


def _prepare(YorgInt, M, Mmiss, C0, X0, perms, epochs, num_batches):
    """The host work in front of the launch: every refusal, mu and mbar with numpy, the batch maps, the sizes of the batches and their
    entries by row, and the arrays in the device's layouts.  Returns the dict `_launch` takes."""
    YorgInt, M, Mmiss, C0, X0, (d, n, r, B) = _shapes(YorgInt, M, Mmiss, C0, X0)
    epochs, nb = int(epochs), int(num_batches)
    if not 1 <= nb <= MAX_BATCHES:
        raise ValueError(f"num_batches must be 1 .. {MAX_BATCHES} (the batch map is bytes, {NO_ENTRY} = no training entry); got {nb}")
    if epochs < 1:
        raise ValueError("epochs must be >= 1")
    if d > MAX_D or r > MAX_R or r < 1:
        raise ValueError(f"the device engine takes d <= {MAX_D} and 1 <= r <= {MAX_R} (one workgroup holds P on chip); d = {d}, r = {r}")
    Mb, Mmb = _zero_one(M, "M"), _zero_one(Mmiss, "Mmiss")
    if perms is not None and len(perms) != B:
        raise ValueError(f"perms must have one entry per replica ({B}), got {len(perms)}")

    mean, mbar = np.zeros(B), np.zeros(B)
    sizes = np.zeros((B, nb), dtype=np.int32)
    counts = np.zeros((B, epochs, nb, d), dtype=np.int32)
    maps = np.full((B, epochs, n, d), NO_ENTRY, dtype=np.uint8)
    flat_map = maps.reshape(B, epochs, n * d)       # (a view)
    def one(b, pm):
        """replica b with its permutations: its means, sizes, maps and row counts (a slice of each array, nobody else's)"""
        ii, jj = np.nonzero(Mb[b])                  # row-major: the order in which the reference collects its triplets
        N = ii.size
        if N < nb:
            raise ValueError(f"replica {b} has {N} training entries, fewer than num_batches = {nb}: the reference divides by the size of an empty batch")
        if not Mmb[b].any():
            raise ValueError(f"replica {b} has no probe entry (Mmiss is all zero): the error is 0 / 0")
        y = YorgInt[ii, jj]
        mu = np.mean(y)
        if mu == 0 or not np.isfinite(mu):
            raise ValueError(f"the mean of replica {b}'s training entries is {mu}: the data is divided by it")
        mean[b] = mu
        mbar[b] = ((y - mu) / mu).mean()
        sz = _batch_sizes(N, nb)
        sizes[b] = sz
        of_pos = np.repeat(np.arange(nb), sz)       # the batch of a position in the permuted list
        flat = jj * d + ii                          # where the entry stands in the time-major map
        if len(pm) != epochs:
            raise ValueError(f"perms[{b}] must hold one permutation per epoch ({epochs}), got {len(pm)}")
        order = np.arange(N)
        for e in range(epochs):
            pi = np.asarray(pm[e])
            if pi.shape != (N,) or pi.dtype.kind not in "iu" or not np.array_equal(np.bincount(pi.clip(0, N - 1), minlength=N), np.ones(N, dtype=np.int64)):
                raise ValueError(f"perms[{b}][{e}] is not a permutation of 0 .. {N - 1}")
            order = order[pi]                       # every epoch permutes the already permuted list (PMF.py:102)
            flat_map[b, e, flat[order]] = of_pos
            counts[b, e] = np.bincount(of_pos * d + ii[order], minlength=nb * d).reshape(nb, d)

    # The replicas are independent and numpy drops the interpreter lock in the gathers and scatters above, so they run side by side;
    # the draws stay in this thread, replica by replica and epoch by epoch, and a refusal is raised for the lowest replica first.
    workers = min(PREPARE_THREADS, B)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        pending = []
        for b in range(B):
            if perms is None:
                N = int(np.count_nonzero(Mb[b]))
                pm = [np.random.permutation(N) for _ in range(epochs)]
            else:
                pm = perms[b]
            pending.append(pool.submit(one, b, pm))
            if len(pending) > 2 * workers:          # (bounds the permutations alive at a time)
                pending.pop(0).result()
        for f in pending:
            f.result()

    Yt = np.ascontiguousarray(YorgInt.T)            # time-major: column t of the reference's (d, n) arrays is row t
    Mmt = np.ascontiguousarray(np.transpose(Mmb, (0, 2, 1)).astype(np.uint8))
    Pb = np.array(0.1 * C0, dtype=np.float64, order="C")
    Wb = np.array(0.1 * np.transpose(X0, (0, 2, 1)), dtype=np.float64, order="C")
    return dict(d=d, n=n, r=r, B=B, epochs=epochs, nb=nb, Yt=Yt, maps=maps, Mmt=Mmt, sizes=sizes, counts=counts, mean=mean, mbar=mbar, Pb=Pb, Wb=Wb)


def _native_run(entry, cfg, inputs, Pb, Wb, mean, mbar, elapsed_before=0.0):
    """The native call `entry` (psmf_pmf_run or psmf_bpmf_run: the configuration, `inputs`, then P, W, Efull, Yrec, status, elapsed_ms)
    and the dict a batch function returns.  Pb (batch, d, r) and Wb (batch, n, r) are overwritten with the final factors."""
    Efull = np.zeros((cfg.batch, cfg.epochs))
    rec = np.zeros((cfg.batch, cfg.n, cfg.d)) if cfg.want_rec else None
    status = np.zeros(cfg.batch, dtype=np.int32)
    ms = C.c_float()
    ptr = _capi._ptr
    lib = _capi.load_library()
    rc = getattr(lib, entry)(C.byref(cfg), *(ptr(a) for a in inputs), ptr(Pb), ptr(Wb), ptr(Efull), ptr(rec), ptr(status), C.byref(ms))
    _capi.raise_for(lib, rc, f"{entry} failed ({rc})")
    out = dict(Efull=Efull, C=Pb, X=np.ascontiguousarray(np.transpose(Wb, (0, 2, 1))), mean=mean, mean_rating=mbar, status=status,
               elapsed_ms=elapsed_before + ms.value)
    if cfg.want_rec:
        out["Yrec"] = np.ascontiguousarray(np.transpose(rec, (0, 2, 1)))
    return out


def _launch(h, epsilon, lmd, momentum, device, want_rec):
    """psmf_pmf_run on what `_prepare` made (P and W of `h` are overwritten with the final factors)"""
    cfg = _capi.PsmfPmfConfig(abi_version=_capi.ABI_VERSION, d=h["d"], n=h["n"], r=h["r"], batch=h["B"], epochs=h["epochs"], num_batches=h["nb"],
                              device=int(device), want_rec=int(bool(want_rec)), epsilon=float(epsilon), lmd=float(lmd), momentum=float(momentum))
    return _native_run("psmf_pmf_run", cfg, [h[k] for k in ("Yt", "maps", "Mmt", "sizes", "counts", "mean", "mbar")], h["Pb"], h["Wb"], h["mean"], h["mbar"])


def pmf_batch(YorgInt, M, Mmiss, C0, X0, perms=None, *, epochs=2, epsilon=50, lmd=0.01, momentum=0.8, num_batches=9, device=0,
              want_rec=False):
    """Run the recursion of the module docstring on `batch` replicas in one call.

    Layouts are those of impute_batch: YorgInt (d, n); M, Mmiss (batch, d, n) or (d, n), 0 / 1; C0 (batch, d, r); X0 (batch, r, n).
    `perms`: a list, one entry per replica, of `epochs` index arrays (permutations of 0 .. N-1, N the replica's training entries);
    None draws them from the global numpy RNG, replica by replica and epoch by epoch, as the reference's loop would.  No argument
    is modified.

    Returns a dict: Efull (batch, epochs); C (batch, d, r) = P and X (batch, r, n) = W^T, the factors in standardised units; mean and
    mean_rating (batch,), mu and mbar; status (batch,) int32 -- 0, or PSMF_ERR_NUMERIC (-4) for a replica whose factors or error are
    not finite, the others being untouched by it; elapsed_ms of the kernels; with want_rec, Yrec (batch, d, n): the reference's Yrec2
    of the last epoch (the prediction at the probe entries, 0 elsewhere).

    ValueError before any device work: inconsistent shapes; M or Mmiss not 0 / 1; fewer training entries than num_batches in a
    replica (the reference divides by an empty batch's size); a replica without a probe entry; mu == 0; num_batches outside
    1 .. 254; d > 512 or r > 16."""
    h = _prepare(YorgInt, M, Mmiss, C0, X0, perms, epochs, num_batches)
    return _launch(h, epsilon, lmd, momentum, device, want_rec)


def _reference_args(Y, C, X, num_p, num_m, num_feat, M, YorigInt):
    """the checks of a function with the reference's signature; returns YorigInt as an array"""
    Y = np.asarray(Y, dtype=float)
    YorigInt = np.asarray(YorigInt, dtype=float)
    C, X = np.asarray(C), np.asarray(X)
    if Y.shape != (num_p, num_m) or C.shape != (num_p, num_feat) or X.shape != (num_feat, num_m):
        raise ValueError("shape mismatch with num_p, num_m, num_feat")
    if np.shape(M) != Y.shape or not np.array_equal(Y, YorigInt * (np.asarray(M) != 0)):
        raise ValueError("the device path requires Y == YorigInt * M (as the experiment constructs it)")
    return YorigInt


def _reference_result(res, Einit, epochs):
    """(Epred, Efull, RunTime), each (1, epochs + 1), of the first replica of a batch function's result"""
    Epred = np.full((1, epochs + 1), np.nan)
    Efull = np.zeros((1, epochs + 1))
    Epred[0, 0] = Efull[0, 0] = Einit
    Efull[0, 1:] = res["Efull"][0]
    RunTime = np.zeros((1, epochs + 1))
    RunTime[0, 1:] = 1e-3 * res["elapsed_ms"] * np.arange(1, epochs + 1) / epochs      # epochs are not timed separately
    return Epred, Efull, RunTime


def pmf(Y, C, X, num_p, num_m, num_feat, M, Mmiss, YorigInt, Einit, epochs=50, epsilon=50, lmd=0.01, momentum=0.8, num_batches=9):
    """ExperimentImpute/PMF.py:43-159 on the device.  Returns (Epred, Efull, RunTime) like the reference, each (1, epochs + 1): column
    0 is Einit, Epred is NaN beyond it (PMF predicts nothing online), RunTime spreads the kernels' time evenly over the epochs.  The
    permutations come from the global numpy RNG, one numpy.random.permutation per epoch, as in the reference: a script that saves
    and restores the RNG state around the call (PMF.py:218-224) gets the same repeats.  Requires Y == YorigInt * M."""
    YorigInt = _reference_args(Y, C, X, num_p, num_m, num_feat, M, YorigInt)
    res = pmf_batch(YorigInt, M, Mmiss, C, X, None, epochs=epochs, epsilon=epsilon, lmd=lmd, momentum=momentum, num_batches=num_batches)
    return _reference_result(res, Einit, epochs)
