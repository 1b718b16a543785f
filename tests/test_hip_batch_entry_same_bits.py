"""The entry points without a handle (psmf_impute_run, psmf_impute_run_rows, psmf_ssm_run, psmf_ssm_run_ex, psmf_bocpd_run) write the
bits they wrote before their host code moved onto rpsmf_amd/csrc/psmf_batch.h.  tests/golden/batch_entry_parent.npz holds every array
those calls wrote -- status included, elapsed_ms excluded -- as recorded on an MI355X from commit 4f23d92 ("BOCPD: net over every dim,
extended reference, edges; outlier fix"), the parent of the commit that introduced the scaffold, with the inputs below (fixed numpy
seeds).  The comparison is np.array_equal with NaN positions equal: the kernels are the parent's instruction for instruction
(profiles/batch_scaffold_kernel_metadata_vs_parent.diff is empty), so nothing but the same bits is acceptable."""

import os
from functools import lru_cache

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "batch_entry_parent"
ERR_NUMERIC = -4


def _impute_problem(d, n, r, B, seed):
    rng = np.random.default_rng(seed)
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, n)), axis=1) + 3.0 * rng.random((d, 1))
    M = (rng.random((B, d, n)) > 0.4).astype(int)
    M[:, 3] = 0                  # a row that is never observed
    M[:, :, 5] = 0               # a column with no observation at all
    Mmiss = ((1 - M) * (rng.random((B, d, n)) > 0.1)).astype(float)
    return Yorig, M, Mmiss, rng.random((B, d, r)), rng.random((B, r, n))


def _impute(d, n, r, B, seed, kernel, *, passes=1, robust=False, bands=False, R=10.0):
    from rpsmf_amd import impute

    Yorig, M, Mmiss, C0, X0 = _impute_problem(d, n, r, B, seed)
    res = impute.impute_batch(Yorig, M, Mmiss, C0, X0, 2 * np.eye(r), 0.1 * np.eye(r), R, np.eye(r), 2, passes, robust=robust, lambda0=1.8,
                              want_bands=bands)
    assert res["kernel"].split("<")[0] == kernel, res["kernel"]
    keys = ("Epred", "Efull", "inside", "C", "X", "status") + (("Yrec", "YrecL", "YrecH") if bands else ())
    return {k: res[k] for k in keys}


def _ssm(ex):
    from rpsmf_amd.ssm import linear_psmf_batch

    d, r, p, n, B = 20, 10, 20, 30, 3
    rng = np.random.default_rng(20261020 + ex)
    Y = np.cumsum(0.2 * rng.standard_normal((B, d, n)), axis=2)
    C0, x0 = rng.standard_normal((B, d, r)), 0.1 * rng.standard_normal((B, p))
    A = 0.9 * np.eye(p) + 0.02 * rng.standard_normal((p, p))
    G = rng.standard_normal((p, p))
    Q = 0.05 * np.eye(p) + 0.01 * G @ G.T / p
    H = np.hstack([np.eye(r), 0.1 * rng.standard_normal((r, p - r))])
    kw = dict(want_pred=True)
    keys = ("X", "C", "V", "P", "x", "Ypred", "scalars", "status")
    if ex:
        mask = rng.random((B, d, n)) > 0.3
        mask[:, 0] = True            # every step keeps an observed row
        Y = np.where(mask, Y, np.nan)
        kw.update(mask=mask, robust=True, lambda0=1.8, first_step=False, robust_state=np.array([[2.5, 1.25], [21.8, 0.75], [1.8, 1.0]]))
        keys += ("omega", "phi", "robust_state")
    res = linear_psmf_batch(Y, C0, x0, np.eye(r), np.eye(p), A, Q, H, 0.1, **kw)
    return {k: res[k] for k in keys}


def _bocpd():
    from rpsmf_amd.changepoint import mvbocpd_batch

    dim, T, B = 3, 64, 5
    rng = np.random.default_rng(20261021)
    X = rng.standard_normal((B, dim, T))
    X[:, :, 30:] += 4.0              # a change of the mean that the heuristic declares
    X[1, 2, 17] = np.nan             # series 1 is refused on the host; the others are untouched by it
    old = os.environ.get("PSMF_BOCPD_CHUNK")
    os.environ["PSMF_BOCPD_CHUNK"] = "2"      # three chunks, the last one partial; the library reads it at every call
    try:
        res = mvbocpd_batch(X, lam=50.0, drop=4, settle=4, confirm=3, want_R=True, want_logpred=True, max_changepoints=4)
    finally:
        if old is None:
            del os.environ["PSMF_BOCPD_CHUNK"]
        else:
            os.environ["PSMF_BOCPD_CHUNK"] = old
    assert res["status"].tolist() == [0, ERR_NUMERIC, 0, 0, 0]
    out = {k: res[k] for k in ("map_run", "n_changepoints", "R_last", "R", "logpred", "status")}
    out["changepoints"] = np.array([np.pad(c, (0, 4 - len(c)), constant_values=-1) for c in res["changepoints"]], dtype=np.int32)
    return out


CASES = {
    "impute_kernel3": lambda: _impute(19, 40, 3, 2, 1, "psmf_impute_kernel3", passes=2, robust=True, bands=True),
    "impute_kernel2": lambda: _impute(100, 30, 5, 2, 2, "psmf_impute_kernel2"),
    "impute_rows": lambda: _impute(19, 40, 3, 2, 3, "psmf_impute_kernel3w", bands=True,
                                   R=10.0 * 100.0 ** (np.random.default_rng(4).random(19) - 0.5)),
    "impute_large": lambda: _impute(513, 20, 3, 2, 5, "masked per-step engine", robust=True, bands=True),
    "ssm_plain": lambda: _ssm(False),
    "ssm_ex": lambda: _ssm(True),
    "bocpd": _bocpd,
}


def record(path):
    """what the recording job calls on the parent commit: every case's outputs under "<case>.<array>" """
    np.savez_compressed(path, **{f"{case}.{k}": np.asarray(v) for case, fn in CASES.items() for k, v in fn().items()})


@lru_cache(maxsize=None)
def _fixture():
    return load_golden(FIXTURE)


@pytest.mark.parametrize("case", list(CASES))
def test_the_bits_of_the_parent_commit(case):
    want = {k.split(".", 1)[1]: v for k, v in _fixture().items() if k.startswith(case + ".")}
    got = CASES[case]()
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(got):
        g = np.asarray(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(g, want[k], equal_nan=g.dtype.kind == "f"), f"{case}.{k}: {int(np.sum(~((g == want[k]) | ((g != g) & (want[k] != want[k])))))} entries differ"
    if case == "bocpd":
        assert want["status"].tolist() == [0, ERR_NUMERIC, 0, 0, 0] and not want["R"][1].any() and not want["map_run"][1].any()
