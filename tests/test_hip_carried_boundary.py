"""The boundary between two carried blocks of a chained launch of psmf_blk_filter3 (blk_filter3_body in
rpsmf_amd/csrc/psmf_blk34.hip, the prologues and block ends of psmf_blk3.hip): block j parks the r x r state in LDS (F3Carry),
block j + 1 picks it up, with ONE barrier between the hand-off and the prologues, the diagnostics summed one lane per word, the
coefficient stores addressed without a division per trip and issued in front of the barrier of the block end, and the parked state
moved in 16-byte pieces.  None of it touches the arithmetic, so every comparison here is bit for bit.  All of it is compiled into
psmf_blk_filter3 alone; filter3s, filter4 and filter5 share the body and the K assembly and must keep their bits as well.

Shapes are the smallest at which every changed path runs: d = 257 (and d = 3 once); r = 32 (mask mode 0), r = 20 (mode 1), r = 12
(filter3s); T = 3 B + 1 with B = min(64 - r, 48) -- two boundaries that are carried on both sides and a one-step last block --,
two passes, float32 and float64 storage, PSMF and rPSMF, one pass split into run(0, B + 5), run(B + 5, T); and one chained
filter4 (cos-phase, r = 24) and one filter5 case, which share the body and f3_assemble_K.  Each case is compared with

  * the record of the PARENT commit's library, tests/golden/carried_boundary_parent.npz: per pass a blake2b digest of the bytes of
    every array (state, all of y_pred, the mean history; equal digests are np.array_equal and more: the sign of a zero counts)
    and the integer counters of every run -- iterations, sweeps, failed starts, blocks and launches.  Written on an MI355X by
    tests/golden/make_golden_carried_boundary.py on the parent's build, in the same visit as the first run of this file;
  * the same library with PSMF_CHAIN_CARRY=0, with PSMF_XG_AHEAD=0 and with PSMF_BLOCK_CHAIN=0 (np.array_equal).  filter4 is left
    out of the last one: a filter4 block that follows another in the same launch keeps the start predictor's operands warm, so
    chained and one launch per block agree to round-off only -- on the parent as well (tests/test_hip_chain_boundary.py).

test_breakdown_inside_the_duration reads the diagnostics of a chained launch: duration and gap sums positive, the five parts
together no more than the in-kernel duration.  The library does not hand out the raw words of the parts (DevState::dbg):
psmf_counters prints them per block with two decimals when PSMF_DBG_BREAKDOWN is set, so the test reads that line and allows the
rounding of the print (0.005 us per part); one case per kernel that forms the sums (filter3, filter3s, filter5).  GPU only: `pytest -m gpu`; `-s` shows the counters."""

import hashlib
import os
import re

import numpy as np
import pytest

import netlib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")
COUNTER_KEYS = ("ns_steps", "sweep_steps", "ns_iterations", "ns_failed", "filter_launches", "filter_kernel_launches")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "carried_boundary_parent.npz")
KERNELS = {32: "psmf_blk_filter3", 20: "psmf_blk_filter3", 12: "psmf_blk_filter3s"}
SWITCHES = ({"PSMF_CHAIN_CARRY": "0"}, {"PSMF_XG_AHEAD": "0"}, {"PSMF_BLOCK_CHAIN": "0"})


def _case(name, kind, d, r, robust, storage, split=False):
    B = min(64 - r, 48)
    T = 3 * B + 1
    runs = [(0, B + 5), (B + 5, T)] if split else [(0, T)]
    want = {"filter3": KERNELS.get(r), "filter4": "psmf_blk_filter4", "filter5": "psmf_blk_filter5"}[kind]
    return dict(name=name, kind=kind, d=d, r=r, robust=robust, storage=storage, B=B, T=T, runs=runs, want=want)


def cases():
    out = []
    for r in (32, 20, 12):
        for robust in (False, True):
            for storage in ("f32", "f64"):
                out.append(_case(f"r{r}-{'rPSMF' if robust else 'PSMF'}-{storage}", "filter3", 257, r, robust, storage))
    out.append(_case("r32-rPSMF-f32-d3", "filter3", 3, 32, True, "f32"))
    out.append(_case("r32-rPSMF-f32-split", "filter3", 257, 32, True, "f32", split=True))
    out.append(_case("filter4-cos-r24", "filter4", 257, 24, False, "f32"))
    out.append(_case("filter5-r20", "filter5", 257, 20, False, "f64"))
    return out


CASES = cases()


_PROBLEMS = {}


def problem(cs):
    """series and initial state of a case, made once (read-only): column by column in a fixed order, no library routine decides
    the rounding of the series"""
    key = (cs["d"], cs["r"], cs["T"], cs["robust"])
    if key not in _PROBLEMS:
        d, r, T = cs["d"], cs["r"], cs["T"]
        rng = np.random.default_rng(9800 + 7 * r + d + cs["robust"])
        Ct = rng.standard_normal((d, r))
        x = rng.standard_normal(r)
        Y = np.empty((T, d), dtype=np.float32)
        for t in range(T):
            x = x + 0.1 * rng.standard_normal(r)
            cx = np.zeros(d)
            for j in range(r):
                cx += Ct[:, j] * x[j]
            Y[t] = cx + 0.3 * (rng.standard_t(3.0, d) if cs["robust"] else rng.standard_normal(d))
        C0 = (0.1 * rng.standard_normal((d, r))).astype(np.float32).astype(np.float64)
        theta0 = 0.01 + 0.02 * rng.random(r)
        _PROBLEMS[key] = dict(Y=Y, C0=C0, theta0=theta0)
    return _PROBLEMS[key]


def drive(c, cs, env=None):
    """The two passes of a case on one handle -> per pass: state, y_pred, mean history, the integer counters of every run"""
    d, r, T = cs["d"], cs["r"], cs["T"]
    pb = problem(cs)
    env = dict(env or {})
    if cs["want"] == "psmf_blk_filter3s":
        env["PSMF_FILTER6_DUAL"] = "0"        # r <= 16 runs psmf_blk_filter6d by default; this puts filter3s in its place
    kw = dict(robust=cs["robust"], storage=cs["storage"])
    if cs["kind"] == "filter4":
        kw["dyn_kind"] = c.DYN_COS_PHASE
    elif cs["kind"] == "filter5":
        kw.update(coef_update=False, eta_full=False, pbar_predict=False)       # the simplified hooks
    with netlib.env(env):
        f = c.DeviceFilter(d, r, **kw)
    try:
        f.upload_series(np.ascontiguousarray(pb["Y"]))
        V0, P0, Q = 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r)
        theta = dict(theta=pb["theta0"]) if cs["kind"] == "filter4" else {}
        f.set_state(pb["C0"], V0, P0, Q, np.zeros(r), rho=1.0, lambda0=1.8, **theta)
        geo = f.geometry()
        assert geo["filter_kernel"] == cs["want"] and geo["block_steps"] == cs["B"], geo
        out = []
        for ep in range(2):
            if ep and cs["robust"]:              # rPSMF's step_reset (rpsmf.py:106-114)
                f.set_state(Q=Q, rho=1.0, lambda0=1.8)
            counters = []
            for a, b in cs["runs"]:
                f.counters(reset=True)
                f.run(a, b)
                cnt = f.counters()
                counters.append({k: int(cnt[k]) for k in COUNTER_KEYS})
            out.append(dict(state=f.get_state(), y_pred=f.y_pred(0, T), mu_hist=f.mu_history(1, T), counters=counters))
        return out
    finally:
        f.close()


def digest(a):
    a = np.ascontiguousarray(np.asarray(a))
    return np.frombuffer(hashlib.blake2b(a.tobytes(), digest_size=16).digest(), dtype=np.uint8).copy()


def record_of(passes):
    """what the golden file keeps of a case: {key: array}"""
    rec = {}
    for ep, p in enumerate(passes):
        rec[f"pass{ep}/counters"] = np.array([[n[k] for k in COUNTER_KEYS] for n in p["counters"]], dtype=np.int64)
        for k in STATE_KEYS:
            rec[f"pass{ep}/{k}"] = digest(np.asarray(p["state"][k], dtype=np.float64))
        rec[f"pass{ep}/y_pred"] = digest(p["y_pred"])
        rec[f"pass{ep}/mu_hist"] = digest(p["mu_hist"])
    return rec


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("cs", CASES, ids=[cs["name"] for cs in CASES])
def test_carried_boundary(cs, golden):
    from rpsmf_amd import _capi as c

    passes = drive(c, cs)
    B = cs["B"]
    for ep, p in enumerate(passes):
        print(f"\nBOUNDARY case={cs['name']} pass={ep} {p['counters']}")
        for (a, b), n in zip(cs["runs"], p["counters"]):
            nblk = -(-(b - a) // B)
            assert n["filter_launches"] == nblk and n["filter_kernel_launches"] == (1 if nblk > 1 else nblk), n
            assert n["ns_steps"] + n["sweep_steps"] == b - a, n
        for k in STATE_KEYS:
            assert np.all(np.isfinite(np.asarray(p["state"][k], dtype=float))), (cs["name"], k)
        assert np.all(np.isfinite(p["y_pred"])) and np.all(np.isfinite(p["mu_hist"])), cs["name"]
    # the parent's record: same bits, same counters
    for k, v in record_of(passes).items():
        want = golden[f"{cs['name']}/{k}"]
        assert np.array_equal(v, want), (cs["name"], k, v, want)
    # the other routes across a boundary, in this library: same bits
    for env in SWITCHES:
        if cs["kind"] == "filter4" and "PSMF_BLOCK_CHAIN" in env:
            continue                            # (agrees to round-off only, on the parent as well: module docstring)
        other = drive(c, cs, env)
        for ep, (p, q) in enumerate(zip(passes, other)):
            for k in STATE_KEYS:
                assert np.array_equal(np.asarray(p["state"][k]), np.asarray(q["state"][k])), (cs["name"], env, ep, k)
            assert np.array_equal(p["y_pred"], q["y_pred"]), (cs["name"], env, ep, "y_pred")
            assert np.array_equal(p["mu_hist"], q["mu_hist"]), (cs["name"], env, ep, "mu_hist")
            for n, m in zip(p["counters"], q["counters"]):
                for k in COUNTER_KEYS[:5]:      # (the number of launches is what PSMF_BLOCK_CHAIN changes)
                    assert n[k] == m[k], (cs["name"], env, ep, k, n, m)


_LINE = re.compile(r"filter3 per launch: hand-off ([0-9.]+) us, K ([0-9.]+), init ([0-9.]+), steps ([0-9.]+), end ([0-9.]+)")


@pytest.mark.parametrize("name", ["r32-PSMF-f32", "r12-rPSMF-f64", "filter5-r20"])
def test_breakdown_inside_the_duration(name, capfd):
    """The sums a chained launch keeps on chip and flushes where it ends: in-kernel duration and gaps between its blocks positive,
    and hand-off + K + init + steps + end -- the five parts of a block, printed per block with two decimals when
    PSMF_DBG_BREAKDOWN is set -- no more than the duration (they telescope to it: equal up to the rounding of the print, 0.005 us
    each)."""
    from rpsmf_amd import _capi as c

    cs = next(x for x in CASES if x["name"] == name)
    d, r, T = cs["d"], cs["r"], cs["T"]
    pb = problem(cs)
    env = {"PSMF_DBG_BREAKDOWN": "1"}
    if cs["want"] == "psmf_blk_filter3s":
        env["PSMF_FILTER6_DUAL"] = "0"
    kw = dict(coef_update=False, eta_full=False, pbar_predict=False) if cs["kind"] == "filter5" else {}
    with netlib.env(env):
        f = c.DeviceFilter(d, r, robust=cs["robust"], storage=cs["storage"], **kw)
        try:
            f.upload_series(np.ascontiguousarray(pb["Y"]))
            f.set_state(pb["C0"], 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0, lambda0=1.8)
            assert f.geometry()["filter_kernel"] == cs["want"]
            f.counters(reset=True)
            capfd.readouterr()
            f.run(0, T)
            cnt = f.counters()
        finally:
            f.close()
    err = capfd.readouterr().err
    m = _LINE.search(err)
    assert m, err
    parts = [float(x) for x in m.groups()]
    print(f"\nBREAKDOWN case={name} blocks={cnt['filter_launches']} duration/block={cnt['filter_us_mean']:.3f} us "
          f"gap/boundary={cnt['filter_gap_us_mean']:.3f} us parts={parts}")
    assert cnt["filter_launches"] == 4 and cnt["filter_kernel_launches"] == 1, cnt
    assert cnt["filter_us_mean"] > 0 and cnt["filter_gap_us_mean"] > 0, cnt
    assert all(p >= 0 for p in parts) and parts[3] > 0, parts
    assert sum(parts) <= cnt["filter_us_mean"] + 5 * 0.005 + 1e-9, (parts, cnt)
