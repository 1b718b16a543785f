#!/usr/bin/env python
"""Generate tests/golden/convergence_expdata.npz: the inputs and the recorded results of the reference's convergence experiment.

    python tests/golden/make_golden_convergence.py REFERENCE_ROOT

Build container only (the reference does not exist on the GPU box; needs scipy.io).  Data alone are written, and only the arrays the
tests read: from Convergence/data.mat the inputs Y (d x n), Ctrue (d x r), Q (r x r) and the diagonal of R; from Convergence/expdata.mat,
the workspace main.m saves after its 10000 iterations, the start of the Kalman pass X0k and P0k, the Kalman path Xk (r x n) and Pk
(r x r x n), the final C, the last iteration's Xps, Pps and W, and the last 10 entries of avW, CerrI and ErM."""

import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
TAIL = 10


def main(ref):
    from scipy.io import loadmat

    data = loadmat(os.path.join(ref, "Convergence", "data.mat"))
    exp = loadmat(os.path.join(ref, "Convergence", "expdata.mat"))
    d, n, r = int(data["d"][0, 0]), int(data["n"][0, 0]), int(data["r"][0, 0])
    R = np.asarray(data["R"], dtype=float)
    assert R.shape == (d, d) and np.array_equal(R, np.diag(np.diag(R))), "R is diagonal"
    for k in ("Y", "Ctrue", "Q", "R"):
        assert np.array_equal(data[k], exp[k]), f"{k}: main.m ran on data.mat"
    out = dict(Y=data["Y"], Ctrue=data["Ctrue"], Q=data["Q"], Rdiag=np.diag(R).copy(), X0k=exp["X0k"], P0k=exp["P0k"], Xk=exp["Xk"], Pk=exp["Pk"],
               C=exp["C"], Xps=exp["Xps"], Pps=exp["Pps"], W=exp["W"])
    out = {k: np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for k, v in out.items()}
    assert out["Y"].shape == (d, n) and out["Ctrue"].shape == (d, r) and out["Xk"].shape == (r, n) and out["Pk"].shape == (r, r, n)
    assert out["Xps"].shape == (r, n) and out["Pps"].shape == (r, r, n) and out["W"].shape == (1, n) and out["C"].shape == (d, r)
    for k in ("avW", "CerrI", "ErM"):
        a = np.asarray(exp[k], dtype=np.float64).ravel()
        assert a.shape == (10000,)
        out[k + "_tail"] = a[-TAIL:].copy()
    path = os.path.join(OUT, "convergence_expdata.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
