"""The two matrix-factorisation entry points that process their batch in chunks of replicas (psmf_pmf_run, psmf_bpmf_run) write the bits
they wrote before their host loops moved onto the chunk plan and the per-item slots of rpsmf_amd/csrc/psmf_batch.h.
tests/golden/chunked_entry_parent.npz holds the arrays of the cases below -- status included, elapsed_ms excluded -- as recorded on an
MI355X from commit 061bb8d ("PMF and BPMF: seeded nets, long-double models, entry-check tests"), the parent of the commit that moved
them, by `record` below.  Every case has 5 replicas and, but for one, runs them through chunks of 2 (three chunks, the last partial), so
a stride or an offset of a per-replica buffer that disagrees between its allocation, its way in and its way out moves a bit here.  The
comparison is np.array_equal with NaN positions equal, dtype and shape included: the host code touches no arithmetic and the kernels
are the parent's instruction for instruction (profiles/chunk_scaffold_kernel_metadata_vs_parent.diff is empty), so nothing but the same
bits is acceptable.  (psmf_bocpd_run's chunked loop is pinned the same way by the `bocpd` case of
tests/test_hip_batch_entry_same_bits.py.)"""

import os
from functools import lru_cache

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "chunked_entry_parent"
ERR_NUMERIC = -4
B = 5
DIVERGING = 3                    # the replica of the pmf_regs inputs that leaves the finite range: in the second chunk of 2
KEYS = ("Efull", "C", "X", "mean", "mean_rating", "status", "Yrec")
PMF_EPSILON = 50                 # the reference's: by the numpy model of tests/pmf_model.py the healthy replicas of both shapes stay finite at it


def _problem(d, n, r, seed):
    """data like tests/pmf_cases.py: 40 + a rank-3 signal of standard deviation 6 + unit noise, a tenth natively missing (shared by the
    replicas), a fifth of the rest held out per replica"""
    rng = np.random.default_rng(seed)
    sig = rng.standard_normal((d, 3)) @ rng.standard_normal((3, n))
    sig *= 6.0 / float(sig.std())
    native = rng.random((d, n)) < 0.1
    YorgInt = np.where(native, 0.0, 40.0 + sig + rng.standard_normal((d, n)))
    M = np.zeros((B, d, n), dtype=np.uint8)
    Mmiss = np.zeros((B, d, n), dtype=np.uint8)
    for b in range(B):
        held = (rng.random((d, n)) < 0.2) & ~native
        M[b], Mmiss[b] = ~native & ~held, held
    return rng, YorgInt, M, Mmiss, rng.random((B, d, r)), rng.random((B, r, n))


def _with_switches(switches, call):
    """`call()` with the environment switches set (the library reads them at every call), and the environment put back"""
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        return call()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _pmf(d, n, r, epochs, nb, seed, switches, diverging=None):
    from pmf_cases import DIVERGING_SCALE
    from rpsmf_amd.pmf import pmf_batch

    rng, YorgInt, M, Mmiss, C0, X0 = _problem(d, n, r, seed)
    perms = [[rng.permutation(int(M[b].sum())) for _ in range(epochs)] for b in range(B)]
    if diverging is not None:
        C0[diverging] *= DIVERGING_SCALE      # as pmf_cases.diverging(): the steps leave the finite range within the two epochs (the model says so)
    res = _with_switches(switches, lambda: pmf_batch(YorgInt, M, Mmiss, C0, X0, perms, epochs=epochs, epsilon=PMF_EPSILON, num_batches=nb,
                                                     want_rec=True))
    return {k: res[k] for k in KEYS}


def _bpmf():
    from bpmf_cases import BETA, TINY, draw_seeded
    from rpsmf_amd.bpmf import bpmf_batch

    d, n, r, epochs, seed = 19, 50, 3, 2, 20261023
    _, YorgInt, M, Mmiss, C0, X0 = _problem(d, n, r, seed)
    draws = [draw_seeded([seed, b], d, n, r, int(M[b].sum()), epochs) for b in range(B)]
    assert d * n < TINY              # so the warm start runs at epsilon = 2, as tests/bpmf_cases.py has it: at 50 it diverges
    res = _with_switches({"PSMF_BPMF_COLS": "4", "PSMF_BPMF_CHUNK": "2"},      # 13 workgroups a replica, the last with two columns
                         lambda: bpmf_batch(YorgInt, M, Mmiss, C0, X0, draws, epochs=epochs, beta=BETA, want_rec=True,
                                            warm_start=dict(epsilon=2, num_batches=3)))
    return {k: res[k] for k in KEYS}


REGS = dict(d=19, n=50, r=3, epochs=2, nb=3, seed=20261021, diverging=DIVERGING)      # accumulators in registers
CASES = {
    # four workgroups a replica, the last with two columns; three chunks, the last partial
    "pmf_regs": lambda: _pmf(**REGS, switches={"PSMF_PMF_COLS": "16", "PSMF_PMF_CHUNK": "2"}),
    # the one-wave instance with its accumulators in LDS; the columns per workgroup are the library's
    "pmf_lds": lambda: _pmf(260, 20, 5, 1, 2, 20261022, {"PSMF_PMF_CHUNK": "2"}),
    "pmf_unchunked": lambda: _pmf(**REGS, switches={}),
    "bpmf": _bpmf,
}


@lru_cache(maxsize=None)
def _run(case):
    """the case's arrays: computed once, shared by the tests, not to be modified"""
    return CASES[case]()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _status_is_pinned(out):
    """one replica with a status, outside the first chunk: the offsets of the status loop and of its finite checks"""
    return out["pmf_regs.status"].tolist() == [ERR_NUMERIC if b == DIVERGING else 0 for b in range(B)] and \
        all(not out[f"{case}.status"].any() for case in ("pmf_lds", "bpmf"))


def record(path):
    """what the recording job calls on the parent commit: every case's outputs under "<case>.<array>" """
    out = {f"{case}.{k}": np.asarray(v) for case in CASES for k, v in _run(case).items()}
    assert _status_is_pinned(out), {k: v.tolist() for k, v in out.items() if k.endswith(".status")}
    assert all(_same(out[f"pmf_unchunked.{k}"], out[f"pmf_regs.{k}"]) for k in KEYS)
    np.savez_compressed(path, **out)


@lru_cache(maxsize=None)
def _fixture():
    return load_golden(FIXTURE)


@pytest.mark.parametrize("case", list(CASES))
def test_the_bits_of_the_parent_commit(case):
    want = {k.split(".", 1)[1]: v for k, v in _fixture().items() if k.startswith(case + ".")}
    got = _run(case)
    assert sorted(got) == sorted(want) == sorted(KEYS), (sorted(got), sorted(want))
    for k in KEYS:
        g = np.asarray(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert _same(g, want[k]), f"{case}.{k}: {int(np.sum(~((g == want[k]) | ((g != g) & (want[k] != want[k])))))} entries differ"
    if case == "pmf_unchunked":      # the chunking and the columns per workgroup move no bit
        for k in KEYS:
            assert _same(got[k], _run("pmf_regs")[k]), f"pmf_unchunked.{k} differs from pmf_regs.{k}"


def test_the_fixture_pins_a_status_outside_the_first_chunk():
    assert _status_is_pinned(_fixture())
