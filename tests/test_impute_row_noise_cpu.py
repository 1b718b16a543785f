"""Per-row observation noise (a diagonal R with unequal entries) in the masked filters, the parts that need no GPU:
(i) the CPU oracle with rho as a (d,) vector reproduces what the reference's own functions returned with R = np.diag(rho)
(tests/golden/impute_row_noise.npz, made by tests/golden/make_golden_row_noise.py); (ii) how rpsmf_amd.impute reads the R argument:
scalar, (d,) vector, (d, d) diagonal matrix; a constant diagonal goes down the scalar entry point; what is refused and how."""

import os

import numpy as np
import pytest

from conftest import ROOT, relerr
from oracle.impute_oracle import impute_filter, mle_smf_filter
from rpsmf_amd import impute

G = np.load(os.path.join(ROOT, "tests", "golden", "impute_row_noise.npz"))


def _inputs(tag):
    Yorig, Mmiss, M = G[tag + "_Yorig"], G[tag + "_Mmiss"].astype(float), G[tag + "_M"].astype(int)
    YorigInt = np.nan_to_num(Yorig, nan=0.0)
    return YorigInt, YorigInt * M, M, Mmiss, G[tag + "_C0"], G[tag + "_X0"], G[tag + "_rho"], float(G[tag + "_Einit"])


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("method", ["psmf", "rpsmf", "mle"])
def test_oracle_with_a_noise_vector_reproduces_the_reference(tag, method):
    YorigInt, Y, M, Mmiss, C0, X0, rho, Einit = _inputs(tag)
    r = C0.shape[1]
    assert rho.max() / rho.min() > 10
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    X = X0.copy()
    if method == "mle":
        ep, ef, ib = mle_smf_filter(Y, C0, X, M, Mmiss, Q, rho, P, 2, 2, YorigInt, Einit)
    else:
        ep, ef, ib = impute_filter(Y, C0, X, M, Mmiss, V, Q, rho, P, 2, 2, YorigInt, Einit, robust=method == "rpsmf", lambda0=1.8)
    assert relerr(ep, G[f"{tag}_{method}_Epred"]) < 1e-12 and relerr(ef, G[f"{tag}_{method}_Efull"]) < 1e-12
    assert relerr(X, G[f"{tag}_{method}_X"]) < 1e-12
    assert ib == float(G[f"{tag}_{method}_inside"])
    # ... and not by ignoring the vector: R = mean(rho) I is somewhere else entirely
    X = X0.copy()
    if method == "mle":
        mle_smf_filter(Y, C0, X, M, Mmiss, Q, float(rho.mean()), P, 2, 2, YorigInt, Einit)
    else:
        impute_filter(Y, C0, X, M, Mmiss, V, Q, float(rho.mean()), P, 2, 2, YorigInt, Einit, robust=method == "rpsmf", lambda0=1.8)
    assert relerr(X, G[f"{tag}_{method}_X"]) > 1e-4


def test_accepted_forms_of_R():
    d = 6
    rho = np.array([1.0, 2.5, 10.0, 0.0, 7.0, 100.0])
    assert impute._row_noise(10.0, d) == (10.0, None) and impute._row_noise(np.float64(3.0), d) == (3.0, None)
    for form in (rho, list(rho), np.diag(rho), rho.astype(np.float32)):
        s, rows = impute._row_noise(form, d)
        assert s is None and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"] and np.array_equal(rows, rho)
    rows = impute._row_noise(np.diag(rho), d)[1]
    rows[0] = -1.0          # (a copy, not a view of the caller's matrix)
    assert rho[0] == 1.0


def test_constant_diagonal_takes_the_scalar_path():
    d = 5
    for form in (np.full(d, 10.0), 10.0 * np.eye(d), [10.0] * d, np.full(1, 10.0)):
        dd = 1 if np.shape(form) == (1,) else d
        assert impute._row_noise(form, dd) == (10.0, None)
    assert impute._row_noise(np.zeros(d), d) == (0.0, None)


def test_refused_forms_of_R():
    d = 5
    R = 10.0 * np.eye(d)
    R[1, 3] = 0.5
    with pytest.raises(NotImplementedError, match="diagonal"):
        impute._row_noise(R, d)
    for bad in (np.ones(d + 1), np.eye(d - 1), np.ones((d, d + 1)), np.ones((d, d, 1))):
        with pytest.raises(ValueError):
            impute._row_noise(bad, d)
    for entry in (-1.0, np.nan, np.inf):
        v = np.arange(1.0, d + 1)
        v[2] = entry
        with pytest.raises(ValueError, match="finite and >= 0"):
            impute._row_noise(v, d)
        with pytest.raises(ValueError, match="finite and >= 0"):
            impute._row_noise(np.diag(v), d)


@pytest.mark.parametrize("d,r", [(513, 4), (40, 17), (600, 20)])
def test_unequal_entries_beyond_the_one_workgroup_kernels_are_refused_before_any_device_work(d, r):
    n = 4
    rng = np.random.default_rng(0)
    Y, M = rng.standard_normal((d, n)), np.ones((d, n))
    rho = 1.0 + rng.random(d)
    assert impute.kernel_name(d, r) == "masked per-step engine"
    for R in (rho, np.diag(rho)):
        with pytest.raises(NotImplementedError, match=r"d <= 512 and r <= 16"):
            impute.impute_batch(Y, M, 1 - M, rng.random((d, r)), rng.random((r, n)), np.eye(r), np.eye(r), R, np.eye(r), 2, 1)
    with pytest.raises(ValueError):      # a wrong length is reported as such on every shape
        impute.impute_batch(Y, M, 1 - M, rng.random((d, r)), rng.random((r, n)), np.eye(r), np.eye(r), rho[:-1], np.eye(r), 2, 1)


def test_the_limit_is_the_kernel_table_s():
    """every shape inside the stated limit is one of the one-workgroup kernels -- with the larger LDS need of the row-noise instances"""
    for d, r in ((512, 16), (512, 1), (1, 16), (80, 14), (81, 14), (80, 15), (19, 10)):
        assert impute.kernel_name(d, r) != "masked per-step engine"
    assert impute.ROW_NOISE_MAX_D == 512 and impute.ROW_NOISE_MAX_R == 16
