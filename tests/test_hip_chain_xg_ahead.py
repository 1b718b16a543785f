"""PSMF_XG_AHEAD and the K assembly's load group (DESIGN sections 4 and 9).  f3_assemble_K issues every global load of a block's
assembly as one group (the cross-Gram staging, the previous coefficients and Y^T Y, indexed without a division by the block
length), and a carried block of a chained launch of psmf_blk_filter3 / 3s whose hand-off is already answered issues that group in
front of the hand-off's store drain.  Only the order of loads, stores and barriers changes -- no floating-point operation, no
other place for any value -- so one series and initial state run in three handles must agree BIT FOR BIT (np.array_equal):
    default                 the group fetched ahead of the hand-off
    PSMF_XG_AHEAD=0         the group fetched behind the hand-off's barrier ("off" and "the poll said no" are the same code)
    PSMF_BLOCK_CHAIN=0      one launch per block: every block takes the assembly from DevState, no hand-off inside a launch
(switches are read per handle at psmf_create).  The default handle is also held against the float64 oracle at the bars the suite
states for this engine (tests/test_hip_filter.py TOL, tests/blocked_cases.py bar: relerr < 1e-5 with float32 storage, < 1e-9 with
float64 storage and a random walk).  The horizons are two or three blocks: the shapes at which the changed code can go wrong are
the edges of the LAST block (nb = 1: the Y^T Y indexing at its edge; nb = B - 1: the zeroed K image and the clamped loads), not
the length of the run.  GPU only: `pytest -m gpu`."""

import numpy as np
import pytest

import netlib
from conftest import relerr
from oracle import psmf_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")
COUNTER_KEYS = ("ns_steps", "sweep_steps", "ns_iterations", "ns_failed")
TOL = {"f64": 1e-9, "f32": 1e-5}
HANDLES = {"default": {}, "ahead_off": {"PSMF_XG_AHEAD": "0"}, "unchained": {"PSMF_BLOCK_CHAIN": "0"}}


def _block_steps(r):
    return min(64 - r, 48)


def _problem(d, r, T, robust, seed, storage):
    rng = np.random.default_rng(seed)
    Ct = rng.standard_normal((d, r))
    x = rng.standard_normal(r)
    Y = np.empty((T, d))
    for t in range(T):
        x = x + 0.1 * rng.standard_normal(r)
        Y[t] = Ct @ x + 0.3 * (rng.standard_t(3.0, d) if robust else rng.standard_normal(d))
    C0 = 0.1 * rng.standard_normal((d, r))
    if storage == "f32":
        Y, C0 = Y.astype(np.float32).astype(np.float64), C0.astype(np.float32).astype(np.float64)
    return Y, C0


def _rows(T, B):
    """the first, a middle and the last row of every block"""
    rows = set()
    for a in range(0, T, B):
        b = min(a + B, T)
        rows |= {a, (a + b) // 2, b - 1}
    return sorted(rows)


def _run(env, Y, C0, r, robust, storage, plan, want):
    """plan: a list of (a, b) runs.  Per run: the state, the sampled predictions, the mean history and the integer counters."""
    from rpsmf_amd import _capi as c

    d, T = Y.shape[1], Y.shape[0]
    env = dict(env)
    if want == "psmf_blk_filter3s":
        env["PSMF_FILTER6_DUAL"] = "0"        # r <= 16 runs psmf_blk_filter6d by default; this puts filter3s in its place
    V0, P0, Q = 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r)
    out = []
    with netlib.env(env):
        f = c.DeviceFilter(d, r, storage=storage, robust=robust)
    try:
        f.upload_series(Y)
        f.set_state(C0, V0, P0, Q, np.zeros(r), rho=1.0, lambda0=1.8)
        geo = f.geometry()
        assert geo["filter_kernel"] == want and geo["engine"] == "block", geo
        B = geo["block_steps"]
        assert B == _block_steps(r), geo
        done = 0
        for a, b in plan:
            f.counters(reset=True)
            f.run(a, b)
            done = max(done, b)
            cnt = f.counters()
            nblk = -(-(b - a) // B)
            assert cnt["filter_launches"] == nblk, (cnt, nblk)
            assert cnt["ns_steps"] + cnt["sweep_steps"] == b - a, cnt
            chained = "PSMF_BLOCK_CHAIN" not in env and nblk > 1      # the path under test: one launch for all the blocks of the run
            assert cnt["filter_kernel_launches"] == (1 if chained else nblk), cnt
            s = f.get_state()
            snap = {k: np.array(s[k]) for k in STATE_KEYS}
            for t in _rows(T, B):
                if t < done:
                    snap[f"y_pred[{t}]"] = f.y_pred(t, 1)
            snap["mu_hist"] = f.mu_history(1, done)
            for k in COUNTER_KEYS:
                snap[k] = np.int64(cnt[k])
            if b == T:
                snap["y_pred_all"] = f.y_pred(0, T)
            out.append(snap)
    finally:
        f.close()
    return out


def _oracle(Y, C0, r, robust, plan):
    """the float64 oracle over the same runs: (state, y_pred) after the last one"""
    st = O.State(C=C0.copy(), V=0.1 * np.eye(r), mu=np.zeros(r), P=np.eye(r), Q=0.1 * np.eye(r), rho=1.0, lam=1.8)
    mode = O.Mode(robust=robust)
    Yp = np.zeros_like(Y)
    for a, b in plan:        # (a further pass through the handle carries everything: the restart of rPSMF's Q, R, lambda is the caller's)
        for k in range(a + 1, b + 1):
            st, info = O.lowrank_step(st, Y[k - 1], k, mode, O.RandomWalkDyn())
            Yp[k - 1] = info.y_pred
    return st, Yp


def _check(d, r, T, robust, want, seed, storage="f32", plan=None):
    plan = plan or [(0, T)]
    Y, C0 = _problem(d, r, T, robust, seed, storage)
    got = {name: _run(env, Y, C0, r, robust, storage, plan, want) for name, env in HANDLES.items()}
    base = got["default"]
    for name in ("ahead_off", "unchained"):
        assert len(got[name]) == len(base)
        for i, (a, b) in enumerate(zip(base, got[name])):
            assert a.keys() == b.keys()
            for k in a:
                assert np.all(np.isfinite(a[k])), (k,)
                assert np.array_equal(a[k], b[k]), (name, f"run {i}", k, float(np.max(np.abs(np.asarray(a[k], dtype=float) - np.asarray(b[k], dtype=float)))))
    st, Yp = _oracle(Y, C0, r, robust, plan)
    tol = TOL[storage]
    last = base[-1]
    for name in ("C", "V", "mu", "P"):
        e = relerr(last[name], getattr(st, name))
        assert e < tol, (name, e)
    e = relerr(last["y_pred_all"], Yp)
    assert e < tol, ("y_pred", e)


def _horizons(B):
    # last block of one step | of B - 1 steps (r + nb < RB: the zeroed K image, the clamped loads) | a full one
    return {"2B+1": 2 * B + 1, "3B-1": 3 * B - 1, "2B": 2 * B}


@pytest.mark.parametrize("horizon", ["2B+1", "3B-1", "2B"])
@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
@pytest.mark.parametrize("d", [260, 257])        # the float32 MFMA bulk kernels | the general ones
def test_r32_last_block_edges(d, robust, horizon):
    r = 32
    T = _horizons(_block_steps(r))[horizon]
    _check(d, r, T, robust, "psmf_blk_filter3", 9800 + d + robust)


@pytest.mark.parametrize("r", [20, 17])
def test_three_column_tiles(r):
    """B = 44 and 47: three column tiles of the cross block, staging columns beyond 32, mask mode 1"""
    B = _block_steps(r)
    assert B > 32
    _check(260, r, 2 * B + 1, True, "psmf_blk_filter3", 9820 + r)


def test_filter3s_full_staging_width():
    """r = 12 with PSMF_FILTER6_DUAL=0: psmf_blk_filter3s, B = 48 -- the full staging width and the last Y^T Y trip"""
    r = 12
    B = _block_steps(r)
    assert B == 48
    _check(260, r, 2 * B + 1, False, "psmf_blk_filter3s", 9840)


def test_r32_float64_storage():
    r = 32
    _check(260, r, 2 * _block_steps(r) + 1, True, "psmf_blk_filter3", 9850, storage="f64")


def test_r32_two_passes():
    """the second pass starts from a carried state: its first block already runs Newton-Schulz steps"""
    r = 32
    T = 2 * _block_steps(r) + 1
    _check(260, r, T, True, "psmf_blk_filter3", 9860, plan=[(0, T), (0, T)])


def test_r32_run_split_inside_a_block():
    """run(0, B + 5), run(B + 5, T): the first launch ends inside a block and leaves the DevState dump, the second chains from it.
    (The Aprev loads of the group run in every case of this file: with PSMF_BLOCK_CHAIN=0 each block but a run's first assembles
    from DevState and Aprev.)"""
    r = 32
    B = _block_steps(r)
    T = 3 * B + 7
    _check(260, r, T, True, "psmf_blk_filter3", 9870, plan=[(0, B + 5), (B + 5, T)])
