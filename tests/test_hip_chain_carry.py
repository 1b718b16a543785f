"""PSMF_CHAIN_CARRY (DESIGN sections 4 and 9): inside a chained launch of psmf_blk_filter3 / filter3s the r x r state goes from block
to block on chip, and DevState gets it where the launch ends.  Only the transport of the values changes -- the same doubles and
floats through LDS instead of an L2 round trip, no operation and no order of operations -- so carry on (=1, the default) and carry
off (=0, the through-memory path) must agree BIT FOR BIT: every comparison here is np.array_equal.  The same series and initial
state run in a handle of each kind (switches are read per handle at psmf_create).  GPU only: `pytest -m gpu`."""

import numpy as np
import pytest

import netlib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")


def _problem(d, r, T, robust, seed):
    rng = np.random.default_rng(seed)
    Ct = rng.standard_normal((d, r))
    x = rng.standard_normal(r)
    Y = np.empty((T, d), dtype=np.float32)
    for t in range(T):
        x = x + 0.1 * rng.standard_normal(r)
        Y[t] = Ct @ x + 0.3 * (rng.standard_t(3.0, d) if robust else rng.standard_normal(d))
    C0 = (0.1 * rng.standard_normal((d, r))).astype(np.float32).astype(np.float64)
    return Y, C0


def _snapshot(f, done, rows):
    """state, y_pred at the sampled timesteps and the mean history, of the `done` timesteps run so far (later rows hold nothing yet)"""
    s = f.get_state()
    out = {k: np.array(s[k]) for k in STATE_KEYS}
    for t in rows:
        if t < done:
            out[f"y_pred[{t}]"] = f.y_pred(t, 1)
    out["mu_hist"] = f.mu_history(1, done)
    return out


def _run(carry, d, r, T, robust, plan, want, seed, make=None, chained=True):
    """plan(B), B the handle's block length: a list of ("run", a, b) | ("roundtrip",) | ("snap",) -> the snapshots taken, the last
    one after the whole plan"""
    env = {"PSMF_CHAIN_CARRY": carry}
    if want == "psmf_blk_filter3s":
        env["PSMF_FILTER6_DUAL"] = "0"        # r <= 16 runs psmf_blk_filter6d by default; this puts filter3s in its place
    from rpsmf_amd import _capi as c

    Y, C0 = _problem(d, r, T, robust, seed)
    V0, P0, Q = 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r)
    rows = sorted({0, 1, T // 3, T // 2, T - 2, T - 1})
    snaps, done = [], 0
    with netlib.env(env):
        f = make(c, d, r, robust, T) if make else c.DeviceFilter(d, r, storage="f32", robust=robust)
    # (the environment is back to what it was: the handle read it at psmf_create, nothing below looks at the environment)
    try:
        f.upload_series(Y)
        f.set_state(C0, V0, P0, Q, np.zeros(r), rho=1.0, lambda0=1.8)
        geo = f.geometry()
        assert geo["filter_kernel"] == want, geo
        B = geo["block_steps"]
        for op in plan(B):
            if op[0] == "run":
                f.counters(reset=True)
                f.run(op[1], op[2])
                done = max(done, op[2])
                cnt = f.counters()
                nblk = -(-(op[2] - op[1]) // B)
                assert cnt["filter_launches"] == nblk, (cnt, nblk)
                if chained and nblk > 1:        # the path under test: one launch for all the blocks of the run
                    assert cnt["filter_kernel_launches"] == 1, cnt
            elif op[0] == "roundtrip":
                s = f.get_state()
                f.set_state(s["C"], s["V"], s["P"], s["Q"], s["mu"], rho=s["rho"], lambda0=s["lam"])
            else:
                snaps.append(_snapshot(f, done, rows))
        snaps.append(_snapshot(f, done, rows))
    finally:
        f.close()
    return snaps, B


def _assert_same(on, off, what):
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (what, f"snapshot {i}", k, float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))))
            assert np.all(np.isfinite(a[k])), (what, k)


def _ab(d, r, T, robust, plan, want, seed, **kw):
    on, B = _run("1", d, r, T, robust, plan, want, seed, **kw)
    off, B0 = _run("0", d, r, T, robust, plan, want, seed, **kw)
    assert B == B0
    return on, off, B


# r = 32: mask mode 0, r = 20: mode 1 (both psmf_blk_filter3), r = 12: psmf_blk_filter3s (PSMF_FILTER6_DUAL=0, see _run)
SHAPES = [(32, 6000, "psmf_blk_filter3"), (20, 4000, "psmf_blk_filter3"), (12, 2000, "psmf_blk_filter3s")]


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
@pytest.mark.parametrize("r,d,want", SHAPES, ids=[f"r{s[0]}" for s in SHAPES])
def test_two_passes_from_the_initial_state(r, d, want, robust):
    """T = 1000 from the initial state (nothing carried into the first block: sweeps and failed starts in the first blocks), then a
    second pass over the series on the carried state.  The last block of a pass is a short one."""
    T = 1000
    on, off, B = _ab(d, r, T, robust, lambda B: [("run", 0, T), ("snap",), ("run", 0, T)], want, 9100 + r + robust)
    assert T % B != 0, B
    _assert_same(on, off, (r, robust))


@pytest.mark.parametrize("r,d,want", SHAPES, ids=[f"r{s[0]}" for s in SHAPES])
def test_pass_split_into_runs(r, d, want):
    """One pass as three run() calls, the first ending at a block edge, the second inside a block: the dump that a chain leaves at
    its end is what the next launch reloads.  (Compared with the same splits with carry off, not with the unsplit pass: the first
    block of every run takes the Gram of the stored C, a chained one assembles it -- other bits, with or without the carry.)"""
    T = 700
    plan = lambda B: [("run", 0, 4 * B), ("snap",), ("run", 4 * B, 9 * B + 7), ("snap",), ("run", 9 * B + 7, T)]
    on, off, B = _ab(d, r, T, True, plan, want, 9200 + r)
    assert 9 * B + 7 < T
    _assert_same(on, off, ("split", r))


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
def test_state_round_trip_between_runs(robust):
    """get_state / set_state between two runs: the upload clears the carried dump, the second run starts as a first one does"""
    r, d, T = 32, 5000, 600
    plan = lambda B: [("run", 0, 333), ("roundtrip",), ("snap",), ("run", 333, T)]
    on, off, _ = _ab(d, r, T, robust, plan, "psmf_blk_filter3", 9300 + robust)
    _assert_same(on, off, ("roundtrip", robust))


def _make_filter4(c, d, r, robust, T):
    f = c.DeviceFilter(d, r, storage="f32", robust=robust)
    f.set_schedules(np.ones(T + 1), np.linspace(1.0, 1.2, T + 1))       # per-step schedules: the sequential-inversion kernel
    return f


def _make_filter5(c, d, r, robust, T):
    # the simplified hooks (no coefficient update, eta = tr(R) / d, P_bar = P)
    return c.DeviceFilter(d, r, robust=robust, storage="f64", coef_update=False, eta_full=False, pbar_predict=False)


@pytest.mark.parametrize("make,want,r", [(_make_filter4, "psmf_blk_filter4", 24), (_make_filter5, "psmf_blk_filter5", 20)], ids=["filter4", "filter5"])
def test_other_kinds_unaffected(make, want, r):
    """filter4 / filter5 share the kernel skeleton (blk_filter3_body) and the chained launch but not the carry: the switch does not
    reach them, and what they compute must not depend on it"""
    d, T = 3000, 400
    plan = lambda B: [("run", 0, T), ("snap",), ("run", 0, T)]
    on, off, _ = _ab(d, r, T, False, plan, want, 9400 + r, make=make, chained=False)
    _assert_same(on, off, want)
