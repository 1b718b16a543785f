"""The time-blocked engine on configurations drawn at random (seeded, tests/blocked_cases.py): every coefficient-space kernel
select_filter_kernel can answer with (psmf_blk_filter<8|16|32>, filter2, filter3, filter3s, filter4, filter4s, filter5, filter6,
filter6d, filter7), both families of d-sized kernels, rows from 1 (fewer rows than the rank, than one tile, than the Gram
workgroups) to 6000, horizons and cut points at 1, B - 1, B, B + 1 (B = min(64 - r, 48) steps per block), empty runs, a second
pass from the carried state, every dynamics kind, the hook configurations, PSMF / rPSMF with fixed lambda and scaling factors,
a general Q, R_k / Q_k schedules, the in-loop optimisers, float32 / float64 storage, the environment switches, and two or three
uneven row shards (one of 1 .. 3 rows) on one GPU -- each against the float64 oracle carried across the same run parts.  The
blocked engine is the one behind the headline number and its hand-picked tests leave these shapes out; this is the net under it.
GPU only: `pytest -m gpu`; `-s` shows the error figures of every case (each prints before it asserts).

Bars (the ones the suite states for these quantities, blocked_cases.bar): float64 storage 1e-9 with the random walk, 1e-8 with
device-evaluated dynamics (1e-7 for rPSMF on psmf_blk_filter6), gradsum 1e-7; float32 storage 1e-5.  tests/test_blocked_cases_cpu.py
has shown that the oracle's own response to a last-bit change of the inputs sits 16 x inside them for every case.

An empty run `run(a, a)` must leave get_state() bit-identical: every key of it, the step counter `k` included, where the empty
run follows a run part that ended at a (psmf_run then does nothing at all).  Where the empty run opens a pass (a = 0, after
set_state or after the previous pass ended at T) psmf_run positions the handle at step a like any other run, which writes `k`;
there `k` alone is left out of the comparison.
The NET line of a case names the family of d-sized kernels per handle (per shard): blocked_cases.expected_bulk of its row count.
Reference: pypsmf/psmf/psmf.py:85-188,287-304, rpsmf.py:116-184."""

import numpy as np
import pytest

import blocked_cases as BC
import netlib
from conftest import relerr, relerr_elementwise

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "theta", "gradsum", "rho", "lam", "s", "eta", "N", "phi", "omega")


def _drive(c, cs, pb, row0, dl, comm=None):
    """One handle (the whole filter, or the rows row0 .. row0 + dl of it) through the passes and parts of the case.  Returns the
    per-part records (state, y_pred of the part) and the end-of-run quantities."""
    T, nl = cs["T"], pb["nl"]
    rows = slice(row0, row0 + dl)
    f = netlib.open_filter(c, cs, pb, "block", row0=row0, d_local=dl)
    try:
        if comm is not None:
            f.comm_init_host(*comm)
        f.upload_series(np.ascontiguousarray(pb["Y"][:, rows]))
        f.set_state(pb["C0"][rows], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=pb["lam"],
                    theta=pb["theta"] if nl.n_params else None)
        if cs["sched"]:
            f.set_schedules(pb["rho_k"], pb["q_k"])
        geo = f.geometry()
        assert geo["engine"] == "block" and geo["block_steps"] == cs["B"], geo
        assert geo["filter_kernel"] == BC.expected_kernel(cs), (geo, cs)
        recs = []
        for ep in range(BC.passes_of(cs)):
            netlib.start_pass(f, cs, pb, ep)
            for j, (a, b) in enumerate(cs["parts"]):
                if a == b:                       # an empty run leaves the state as it is, bit for bit
                    before = f.get_state()
                    f.run(a, a)
                    s = f.get_state()
                    # (the step counter too, unless the empty run opens the pass: the module docstring)
                    keys = STATE_KEYS + (("k",) if j > 0 else ())
                    same = [k for k in keys if not np.array_equal(np.asarray(before[k]), np.asarray(s[k]), equal_nan=True)]
                    assert not same, (cs["i"], "empty run changed", same)
                    recs.append(dict(state=s, y_pred=np.empty((0, dl))))
                else:
                    f.run(a, b)
                    recs.append(dict(state=f.get_state(), y_pred=f.y_pred(a, b - a)))
        end = dict(sq_error=f.sq_error(0, T), y_pred=f.y_pred(0, T), predict=f.predict(T, 3))
        return recs, end
    finally:
        f.close()


def _drive_shards(c, cs, pb):
    n = len(cs["shards"])
    starts = np.concatenate([[0], np.cumsum(cs["shards"])]).astype(int)
    _, out = netlib.run_ranks(n, lambda rank, comm: _drive(c, cs, pb, int(starts[rank]), int(cs["shards"][rank]), comm=comm), 200)
    # the replicated state: bit-identical across the shards, after every part
    for j in range(len(out[0][0])):
        for rank in range(1, n):
            for k in STATE_KEYS[1:]:
                assert np.array_equal(np.asarray(out[rank][0][j]["state"][k]), np.asarray(out[0][0][j]["state"][k]), equal_nan=True), (cs["i"], "shards differ", k, j)
    recs = []
    for j in range(len(out[0][0])):
        s = dict(out[0][0][j]["state"])
        s["C"] = np.vstack([out[rank][0][j]["state"]["C"] for rank in range(n)])
        recs.append(dict(state=s, y_pred=np.hstack([out[rank][0][j]["y_pred"] for rank in range(n)])))
    end = dict(sq_error=sum(out[rank][1]["sq_error"] for rank in range(n)), y_pred=np.hstack([out[rank][1]["y_pred"] for rank in range(n)]),
               predict=np.hstack([out[rank][1]["predict"] for rank in range(n)]))
    return recs, end


@pytest.mark.parametrize("i", range(BC.N_CASES))
def test_block_engine_random_configuration(i):
    from rpsmf_amd import _capi as c

    cs = BC.device_case(i)
    pb = BC.problem(cs)
    ref, rollout = BC.reference(cs, pb)
    with netlib.env(cs["env"]):
        recs, end = _drive_shards(c, cs, pb) if cs["shards"] else _drive(c, cs, pb, 0, cs["d"])
    tol, gtol = BC.bar(cs), BC.gradsum_bar(cs)
    errs = []          # (quantity, part, error, bound)
    for j, (rec, want) in enumerate(zip(recs, ref)):
        s = rec["state"]
        errs += netlib.state_errors(cs, s, want, j, tol, gtol, y_pred=rec["y_pred"])
        errs.append(("C elementwise", j, relerr_elementwise(s["C"], want["C"], floor=1e-3)[0], 100 * tol))
        if want["b"] > want["a"] and not cs["robust"]:
            errs += [("eta", j, relerr(s["eta"], want["eta"]), tol), ("N", j, relerr(s["N"], want["N"]), tol)]
    Y, T = pb["Y"], cs["T"]
    last = [w for w in ref if w["ep"] == BC.passes_of(cs) - 1 and w["b"] > w["a"]]
    errs.append(("y_pred of the last pass", -1, relerr(end["y_pred"], np.vstack([w["y_pred"] for w in last])), tol))
    # the device's own sum of squares against the host's over the rows it stored: float64 sums of the same <= 1.2e6 terms
    errs.append(("sq_error", -1, relerr(end["sq_error"], float(np.sum((end["y_pred"] - Y[:T]) ** 2))), 1e-10))
    errs.append(("predict", -1, relerr(end["predict"], rollout), tol))
    bulk = "+".join(BC.expected_bulk(cs, dl)[0] + str(BC.expected_bulk(cs, dl)[1] or "") for dl in (cs["shards"] or [cs["d"]]))
    worst = netlib.verdict(errs)
    print(f"\nNET case={i} kernel={BC.expected_kernel(cs)} bulk={bulk} storage={cs['storage']} dyn={cs['dyn']} hooks={cs['hooks']} "
          f"r={cs['r']} d={cs['d']} T={cs['T']} parts={cs['parts']} shards={cs['shards']} robust={int(cs['robust'])} rec={cs['recursive']} env={cs['env']} "
          f"bar={tol:.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} ratio={worst[2] / worst[3]:.3g}")
    netlib.assert_within(errs, cs)
