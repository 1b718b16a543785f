"""Block boundary of a chained launch of psmf_blk_filter3 / 3s / 4 / 5: inside a chained launch the diagnostics
are summed on chip and reach DevState where the launch ends, and (filter3 / 3s with the chain carry) the hand-off to the next block
is asked one timestep ahead; the announce of a finished block stays in the hand-off.  None of it is a floating-point operation, so
a chained launch (the default) and the same run with PSMF_BLOCK_CHAIN=0 -- one launch per block: the path that keeps the boundary
as it was -- must agree BIT FOR BIT on the state, the predictions and the mean history (np.array_equal), and on every integer
counter the host reads, per pass and after a reset.  The same series and initial state run in a handle of each kind (switches are
read per handle at psmf_create).

filter4 is the exception, on the commit before this change already: a block that follows another one in the same launch keeps the
last step's start-predictor operands in LDS ("warm", blk_filter3_body), a block launched on its own starts cold, so the two paths
take other inversion routes (other ns_steps / sweep_steps in the first pass) and agree to round-off only.  For filter4 and filter5
the chained launch is therefore compared with what the chained launch of the commit before this change left for the same case:
blake2b digests of every array of every snapshot and the integer counters, recorded on an MI355X (gfx950) with
`python tests/test_hip_chain_boundary.py tests/golden/chain_boundary_other_kinds.json` on that commit's build (this file runs
unchanged there; the series of these cases is built from elementwise operations only, so that it does not depend on the host's
BLAS).  The record binds these two cases to the compiler that built both libraries; its version is in the file under "hipcc".
With another compiler, record again on the parent commit.  filter5 is compared with one launch per block as well; its case is
weak for the predictions (every sampled y_pred row of it has one and the same digest in the record): what it pins is the
state, the mean history and the counters.
Not covered: the exit through a dead hand-off (f3_acc_flush beside f3_carry_flush) -- it needs a cross-Gram that never arrives.
GPU only: `pytest -m gpu`."""

import hashlib
import json
import sys

import os

import numpy as np
import pytest

import netlib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")
COUNTER_KEYS = ("ns_steps", "sweep_steps", "ns_iterations", "ns_failed", "filter_launches")


def _problem(d, r, T, robust, seed, elementwise=False):
    rng = np.random.default_rng(seed)
    Ct = rng.standard_normal((d, r))
    x = rng.standard_normal(r)
    Y = np.empty((T, d), dtype=np.float32)
    for t in range(T):
        x = x + 0.1 * rng.standard_normal(r)
        if elementwise:     # the same product, column by column in a fixed order: no library routine decides the rounding
            cx = np.zeros(d)
            for j in range(r):
                cx += Ct[:, j] * x[j]
        else:
            cx = Ct @ x
        Y[t] = cx + 0.3 * (rng.standard_t(3.0, d) if robust else rng.standard_normal(d))
    C0 = (0.1 * rng.standard_normal((d, r))).astype(np.float32).astype(np.float64)
    return Y, C0


def _snapshot(f, done, rows):
    s = f.get_state()
    out = {k: np.array(s[k]) for k in STATE_KEYS}
    for t in rows:
        if t < done:
            out[f"y_pred[{t}]"] = f.y_pred(t, 1)
    out["mu_hist"] = f.mu_history(1, done)
    return out


def _run(chain, d, r, T, robust, plan, want, seed, make=None, state_kw=None):
    """plan(B), B the handle's block length: a list of (a, b) runs -> per run a snapshot and the integer counters of that run, and
    the counters read once more after counters(reset=True)"""
    env = {"PSMF_BLOCK_CHAIN": chain}
    if want == "psmf_blk_filter3s":
        env["PSMF_FILTER6_DUAL"] = "0"        # r <= 16 runs psmf_blk_filter6d by default; this puts filter3s in its place
    from rpsmf_amd import _capi as c

    Y, C0 = _problem(d, r, T, robust, seed, elementwise=make is not None)
    V0, P0, Q = 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r)
    rows = sorted({0, 1, T // 3, T // 2, T - 2, T - 1})
    snaps, counts = [], []
    with netlib.env(env):
        f = make(c, d, r, robust, T) if make else c.DeviceFilter(d, r, storage="f32", robust=robust)
    try:
        f.upload_series(Y)
        if state_kw is None:
            f.set_state(C0, V0, P0, Q, np.zeros(r), rho=1.0, lambda0=1.8)
        else:
            f.set_state(C0, V0, P0, Q, state_kw["mu"], rho=1.0, lambda0=1.8, **{k: v for k, v in state_kw.items() if k != "mu"})
        geo = f.geometry()
        assert geo["filter_kernel"] == want, geo
        B = geo["block_steps"]
        done = 0
        for a, b in plan(B):
            f.counters(reset=True)
            f.run(a, b)
            done = max(done, b)
            cnt = f.counters()
            nblk = -(-(b - a) // B)
            assert cnt["filter_launches"] == nblk, (cnt, nblk)
            if make is None:    # filter3 / 3s.  Chained: one launch for all the blocks of the run; PSMF_BLOCK_CHAIN=0: one per block
                assert cnt["ns_steps"] + cnt["sweep_steps"] == b - a, cnt
                assert cnt["filter_kernel_launches"] == (1 if chain == "1" and nblk > 1 else nblk), cnt
            elif chain == "0":
                assert cnt["filter_kernel_launches"] == nblk, cnt
            counts.append({k: cnt[k] for k in COUNTER_KEYS})
            snaps.append(_snapshot(f, done, rows))
        f.counters(reset=True)
        cnt = f.counters()
        counts.append({k: cnt[k] for k in COUNTER_KEYS + ("filter_kernel_launches",)})
        assert all(v == 0 for v in counts[-1].values()), counts[-1]
    finally:
        f.close()
    return snaps, counts, B


def _assert_same(chained, single, what):
    (sa, ca, Ba), (sb, cb, Bb) = chained, single
    assert Ba == Bb and len(sa) == len(sb)
    assert ca == cb, (what, ca, cb)
    for i, (a, b) in enumerate(zip(sa, sb)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (what, f"snapshot {i}", k, float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))))
            assert np.all(np.isfinite(a[k])), (what, k)


def _ab(*args, **kw):
    return _run("1", *args, **kw), _run("0", *args, **kw)


# r = 32: mask mode 0, r = 20: mode 1 (both psmf_blk_filter3), r = 12: psmf_blk_filter3s (PSMF_FILTER6_DUAL=0, see _run)
SHAPES = [(32, 6000, "psmf_blk_filter3"), (20, 4000, "psmf_blk_filter3"), (12, 2000, "psmf_blk_filter3s")]


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
@pytest.mark.parametrize("r,d,want", SHAPES, ids=[f"r{s[0]}" for s in SHAPES])
def test_two_carried_passes(r, d, want, robust):
    """T = 1000 from the initial state (sweeps and failed starts in the first blocks: every counter moves), then a second pass on
    the carried state.  The last block of a pass is a short one: the K image keeps zeros that a full block overwrites."""
    T = 1000
    chained, single = _ab(d, r, T, robust, lambda B: [(0, T), (0, T)], want, 9500 + r + robust)
    assert T % chained[2] != 0
    _assert_same(chained, single, (r, robust))


@pytest.mark.parametrize("r,d,want", SHAPES, ids=[f"r{s[0]}" for s in SHAPES])
def test_run_split_inside_a_block(r, d, want):
    """One pass as two run() calls split at a step that is not a multiple of the block length: the first launch ends with a short
    block, the second starts from the dump it left; both flush their diagnostics on their own."""
    T = 700
    plan = lambda B: [(0, 9 * B + 7), (9 * B + 7, T)]
    chained, single = _ab(d, r, T, True, plan, want, 9600 + r)
    assert 0 < 9 * chained[2] + 7 < T
    _assert_same(chained, single, ("split", r))


def _make_filter4(c, d, r, robust, T):
    f = c.DeviceFilter(d, r, storage="f32", robust=robust)
    f.set_schedules(np.ones(T + 1), np.linspace(1.0, 1.2, T + 1))       # per-step schedules: the sequential-inversion kernel
    return f


def _make_filter5(c, d, r, robust, T):
    # the simplified hooks (no coefficient update, eta = tr(R) / d, P_bar = P)
    return c.DeviceFilter(d, r, robust=robust, storage="f64", coef_update=False, eta_full=False, pbar_predict=False)


OTHER_KINDS = {"filter4": (_make_filter4, "psmf_blk_filter4", 24), "filter5": (_make_filter5, "psmf_blk_filter5", 20)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_boundary_other_kinds.json")


def _other_kind(name):
    """the chained launch of one case -> {"counters": [...], "digests": [{array name: [dtype, shape, blake2b]}, ...]}"""
    make, want, r = OTHER_KINDS[name]
    d, T = 3000, 400
    snaps, counts, _ = _run("1", d, r, T, False, lambda B: [(0, T), (0, T)], want, 9700 + r, make=make)
    digests = []
    for sn in snaps:
        for k, v in sn.items():
            assert np.all(np.isfinite(v)), (name, k)
        digests.append({k: [str(np.asarray(v).dtype), list(np.shape(v)), hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).hexdigest()]
                        for k, v in sorted(sn.items())})
    return {"counters": counts, "digests": digests}


@pytest.mark.parametrize("name", sorted(OTHER_KINDS))
def test_other_kinds(name):
    """filter4 / filter5 share the kernel skeleton (blk_filter3_body), its LDS carve, the K assembly and the on-chip diagnostics of
    a chained launch; their hand-off stays blk_chain_next.  Two passes of T = 400, chained, against the record of the commit before
    this change (module docstring): same bits, same counters."""
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    got = json.loads(json.dumps(_other_kind(name)))
    assert got["counters"] == want["counters"]
    assert len(got["digests"]) == len(want["digests"])
    for i, (a, b) in enumerate(zip(got["digests"], want["digests"])):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (name, f"snapshot {i}", k)


def test_filter5_chained_against_one_launch_per_block():
    """filter5 has no start to predict: chained and per-block launches agree bit for bit, as for filter3"""
    make, want, r = OTHER_KINDS["filter5"]
    d, T = 3000, 400
    chained, single = _ab(d, r, T, False, lambda B: [(0, T), (0, T)], want, 9700 + r, make=make)
    _assert_same(chained, single, want)


if __name__ == "__main__":      # record the golden file (run on the build to compare with; see the module docstring)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import subprocess

    rec = {name: _other_kind(name) for name in sorted(OTHER_KINDS)}
    for name, v in rec.items():
        print(name, "distinct y_pred digests:", len({x[2] for sn in v["digests"] for k, x in sn.items() if k.startswith("y_pred")}))
    rec["hipcc"] = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[:2]
    with open(sys.argv[1], "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
