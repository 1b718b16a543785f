"""The series ring (psmf_series_ring): a handle that keeps n_slots windows of `chunk` rows of the series on the device and is fed
chunk by chunk, against a resident handle of the whole series and against the CPU oracle.  GPU only: `pytest -m gpu`; `-s` shows
the error figures (each prints before it asserts).

1. The same bits as a resident handle run as run(0, c); run(c, 2c); ... -- C, V, P, Q, mu, theta, gradsum, the eight scalars,
   every chunk's y_hat and mean history, masked handles' (s, eta) -- one case per engine path (tests/ring_cases.py); both handles
   report the intended kernel.
2. The same runs against oracle.psmf_oracle.lowrank_step (mask= for the masked cases): float64 storage 1e-9, float32 1e-5.
3. Residency: what is not on the device is refused on the host, by name, and nothing is launched.
4. A stream of the other element type is converted on the device (psmf_cast_rows) to the bits numpy's cast gives, both ways.
5. Two row shards, each with a ring of its own, under the host communicator.
6. step_stream of the filter classes, and step() after it (the ring handle gives way to a resident one).
7. psmf_masked_metrics of resident chunks while later runs are queued: the sums of a resident handle run to the same step.
8. A launched per-step handle with chunks above 256 steps: the captured graph is rebuilt with every chunk's window.
Reference: pypsmf/psmf/psmf.py:85-102 (step consumes one observation after the other and never looks back)."""

import numpy as np
import pytest

import blocked_cases as BC
import netlib
import ring_cases as RC
from conftest import relerr
from rpsmf_amd.sharding import shard_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

STATE_KEYS = ("C", "V", "P", "Q", "mu", "theta", "gradsum")
SCALARS = ("rho", "lam", "s", "eta", "N", "phi", "omega", "k")


def _handle(c, cs, pb, ring, row0=0, dl=None, comm=None, storage=None):
    d, r = cs["d"], cs["r"]
    dl = d if dl is None else dl
    rows = slice(row0, row0 + dl)
    nl = pb["nl"]
    f = c.DeviceFilter(d, r, row0=row0, d_local=dl, robust=cs["robust"], dyn_kind=nl.device_kind, dyn_flags=nl.device_flags, dyn_terms=nl.device_terms,
                       storage=storage or cs["storage"], recursive=cs["recursive"], update_every=1, adam_lr=RC.ADAM_LR, engine=cs["engine"],
                       nonuniform_R=cs["nonuniform"], masked=cs["masked"])
    if comm is not None:
        f.comm_init_host(*comm)
    if ring:
        f.series_ring(cs["chunk"], cs["n_slots"])
    if cs["nonuniform"]:
        f.set_row_noise(pb["rho_rows"][rows], rho_mean=float(pb["rho_rows"].sum()) / d)
    f.set_state(pb["C0"][rows], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=1.0 if cs["nonuniform"] else pb["rho"], lambda0=pb["lam"],
                theta=pb["theta"] if nl.n_params else None)
    if nl.n_params:
        f.zero_gradsum()
    if cs["recursive"]:
        f.set_adam(np.zeros(nl.n_params), np.zeros(nl.n_params))
    return f


def _record(f, cs, kb, ke, yp=None):
    rec = dict(y_pred=f.y_pred(kb, ke - kb) if yp is None else yp, mu_hist=f.mu_history(kb, ke - kb + 1))
    if cs["masked"]:
        rec["sc"] = f.step_scalars(kb, ke - kb)
    return rec


def _check_kernel(f, cs):
    assert f.geometry()["filter_kernel"] == cs["kernel"], (cs["name"], f.geometry())
    if cs["engine"] == "step":
        assert f.step_plan()["usable"] == (cs["kernel"] == "psmf_pstep_k"), (cs["name"], f.step_plan())


def _chunks(cs, pb, rows=slice(None), dtype=None):
    for kb, ke in RC.spans(cs):
        Y = np.ascontiguousarray(pb["Y"][kb:ke, rows])
        Y = Y if dtype is None else Y.astype(dtype)
        yield (Y, np.ascontiguousarray(pb["M"][kb:ke, rows])) if cs["masked"] else Y


def _expected_slots(cs, j):
    """the chunk every slot holds when run_stream yields chunk j: it has uploaded up to n_slots chunks from j on"""
    n, hi = cs["n_slots"], min(j + cs["n_slots"], RC.N_CHUNKS)
    return [max([c for c in range(hi) if c % n == s], default=-1) for s in range(n)]


def _run_resident(c, cs, pb):
    f = _handle(c, cs, pb, ring=False)
    try:
        f.upload_series(pb["Y"])
        if cs["masked"]:
            f.upload_mask(pb["M"])
        recs = []
        for kb, ke in RC.spans(cs):
            f.run(kb, ke)
            recs.append(_record(f, cs, kb, ke))
        _check_kernel(f, cs)
        return dict(state=f.get_state(), recs=recs)
    finally:
        f.close()


def _run_ring(c, cs, pb, row0=0, dl=None, comm=None, dtype=None, storage=None, yp_dtype=None):
    f = _handle(c, cs, pb, ring=True, row0=row0, dl=dl, comm=comm, storage=storage)
    dl = cs["d"] if dl is None else dl
    try:
        recs, slots = [], []
        for j, (kb, ke, yp) in enumerate(f.run_stream(_chunks(cs, pb, slice(row0, row0 + dl), dtype), y_pred_dtype=np.float64)):
            assert (kb, ke) == RC.spans(cs)[j] and yp.dtype == np.float64 and yp.shape == (ke - kb, dl)
            slots.append(f.series_ring_info()["slots"])
            rec = _record(f, cs, kb, ke, yp)
            if yp_dtype is not None:
                rec["y_pred_other"] = f.y_pred(kb, ke - kb, dtype=yp_dtype)
            recs.append(rec)
        assert len(recs) == RC.N_CHUNKS
        if comm is None:
            _check_kernel(f, cs)
        return dict(state=f.get_state(), recs=recs, slots=slots)
    finally:
        f.close()


_RUNS = {}


def _runs(i):
    """(resident, ring, oracle) of case i, computed once for the tests that share them; a failure is kept and raised again
    instead of running the device a second time"""
    if i not in _RUNS:
        cs = RC.CASES[i]
        try:
            pb = RC.problem(cs)
            _RUNS[i] = (_run_resident(netlib.capi(), cs, pb), _run_ring(netlib.capi(), cs, pb), RC.reference(cs, pb))
        except BaseException as e:      # noqa: BLE001
            _RUNS[i] = e
    if isinstance(_RUNS[i], BaseException):
        raise _RUNS[i]
    return _RUNS[i]


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.IDS)
def test_ring_run_has_the_bits_of_the_resident_handle(i):
    cs = RC.CASES[i]
    res, ring, _ = _runs(i)
    diff = [k for k in STATE_KEYS + SCALARS if not np.array_equal(np.asarray(res["state"][k]), np.asarray(ring["state"][k]))]
    for j, (a, b) in enumerate(zip(res["recs"], ring["recs"])):
        diff += [(k, j) for k in a if not np.array_equal(a[k], b[k])]
    print(f"\nRING {cs['name']}: chunk={cs['chunk']} slots={cs['n_slots']} d={cs['d']} r={cs['r']} T={cs['T']} differing: {diff}")
    assert not diff, (cs["name"], diff)
    assert ring["slots"] == [_expected_slots(cs, j) for j in range(RC.N_CHUNKS)], ring["slots"]


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.IDS)
def test_ring_run_against_the_oracle(i):
    cs = RC.CASES[i]
    _, ring, ref = _runs(i)
    s, tol = ring["state"], RC.bar(cs)
    errs = {k: relerr(s[k], ref[k]) for k in ("C", "V", "P", "mu")}
    for k in ("y_pred", "mu_hist") + (("sc",) if cs["masked"] else ()):
        got = np.vstack([rec[k] if k != "mu_hist" or j == 0 else rec[k][1:] for j, rec in enumerate(ring["recs"])])
        errs[k] = relerr(got, ref[k])
    if cs["robust"]:
        errs.update(rho=relerr(s["rho"], ref["rho"]), lam=relerr(s["lam"], ref["lam"]), Q=relerr(s["Q"], ref["Q"]))
    if ref["theta"].size:
        errs["theta"] = relerr(s["theta"], ref["theta"])
    print(f"\nRING-ORACLE {cs['name']}: bar {tol:.0e} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, (cs["name"], errs)


def test_residency_is_enforced_on_the_host():
    """Nothing here reaches the device with an index outside a slot: every case is refused by the library's host code."""
    c = netlib.capi()
    cs = RC.CASES[0]
    pb = RC.problem(cs)
    ch, n, d = cs["chunk"], cs["n_slots"], cs["d"]
    Y = pb["Y"]
    f = _handle(c, cs, pb, ring=True)
    try:
        assert f.series_ring_info() == dict(chunk=ch, n_slots=n, slots=[-1, -1])
        with pytest.raises(ValueError, match="chunk boundary"):
            f.upload_series(Y[ch - 1:ch + 1], ch - 1)
        with pytest.raises(c.PsmfError, match="step 1 is not resident"):
            f.run(0, 1)
        f.upload_series(Y[:ch], 0)
        assert f.series_ring_info()["slots"] == [0, -1]
        with pytest.raises(c.PsmfError, match="-5.*psmf_series_ring"):
            f.series_ring(ch, n)                       # after an upload
        before = f.get_state()
        with pytest.raises(c.PsmfError, match=f"-5.*step {ch + 1} is not resident"):
            f.run(0, ch + 5)                           # into a chunk never uploaded: nothing of the call is launched
        after = f.get_state()
        assert all(np.array_equal(np.asarray(before[k]), np.asarray(after[k])) for k in before), "a refused run changed the state"
        f.run(0, ch)
        f.upload_series(Y[ch:2 * ch], ch)
        assert f.series_ring_info()["slots"] == [0, 1]
        f.run(ch, 2 * ch)
        y0 = f.y_pred(0, ch)                           # chunk 0 is still resident
        f.upload_series(Y[2 * ch:3 * ch - 3], 2 * ch)  # evicts it; a short chunk
        assert f.series_ring_info()["slots"] == [2, 1]
        with pytest.raises(c.PsmfError, match="-5.*step 1 is no longer resident"):
            f.y_pred(0, ch)
        with pytest.raises(c.PsmfError, match="-5.*no longer resident"):
            f.mu_history(1, 3)
        with pytest.raises(c.PsmfError, match="-5.*no longer resident"):
            f.sq_error(0, ch)
        with pytest.raises(c.PsmfError, match=f"-5.*step {3 * ch - 2} is not resident"):
            f.run(2 * ch, 3 * ch)                      # the rows of the chunk that were not uploaded
        f.run(2 * ch, 3 * ch - 3)
        assert np.array_equal(f.y_pred(ch, ch), f.y_pred(ch, ch)) and y0.shape == (ch, d)
        # the sum of squares over resident chunks against the host's over the same rows (float64 sums of 2 x 37 x 257 terms)
        yp = f.y_pred(ch, 2 * ch - 3)
        assert relerr(f.sq_error(ch, 2 * ch - 3), float(np.sum((yp - Y[ch:3 * ch - 3]) ** 2))) < 1e-10
        for call in (lambda: f.set_schedules(np.ones(10), None), lambda: f.set_schedules(None, np.ones(10)), lambda: f.time_kernel(0, 1)):
            with pytest.raises(c.PsmfError, match="-5.*series ring"):
                call()
        f.sync()
    finally:
        f.close()
    g = c.DeviceFilter(8, 3, engine="step", storage="f64")
    try:
        g.series_ring(5, 2)
        with pytest.raises(c.PsmfError, match="-5.*psmf_set_q_matrix_schedule.*series ring"):
            g.set_q_matrix_schedule(np.tile(np.eye(3), (4, 1, 1)))
    finally:
        g.close()
    g = c.DeviceFilter(8, 3, nonuniform_R=True, engine="step", storage="f64")
    try:
        g.series_ring(5, 2)
        with pytest.raises(c.PsmfError, match="-5.*psmf_set_noise_rotation.*series ring"):
            g.set_noise_rotation(np.eye(8), np.ones(8))
    finally:
        g.close()
    g = c.DeviceFilter(8, 3, dyn_kind=c.DYN_HOST, engine="step", storage="f64")
    try:
        with pytest.raises(c.PsmfError, match="-5.*host-stepped.*series ring"):
            g.series_ring(5, 2)
        for bad in ((0, 2), (5, 1)):
            with pytest.raises(ValueError):
                g.series_ring(*bad)
    finally:
        g.close()


@pytest.mark.parametrize("d,chunk", [(257, 37), (1, 37), (4, 100)], ids=["d257", "d1", "d4"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_a_stream_of_the_other_dtype_is_converted_as_numpy_does(storage, d, chunk):
    """float64 chunks into a float32 handle, float32 chunks into a float64 handle: the same bits as a stream converted by numpy
    beforehand; and the y_hat downloads in the other type (float32 storage read as float64 -- run_stream asked for float64 -- and float64
    storage read as float32) are numpy's cast of the stored rows.  37 x 257 rows start at odd elements (scalar head, vector body,
    scalar tail of psmf_cast_rows); d = 1 leaves chunks without a vector body; d = 4 is all body."""
    c = netlib.capi()
    cs = dict(RC.CASES[0], d=d, chunk=chunk, T=(RC.N_CHUNKS - 1) * chunk + chunk // 2 + 2, storage=storage)
    pb = RC.problem(dict(cs, storage="f64"))          # float64 values that float32 has to round
    if storage == "f64":
        pb["Y"] = pb["Y"].astype(np.float32)          # the caller's stream is float32
    stored, given = (np.float32, np.float64) if storage == "f32" else (np.float64, np.float32)
    by_numpy = _run_ring(c, cs, pb, dtype=stored, yp_dtype=np.float32)
    on_device = _run_ring(c, cs, pb, dtype=given, yp_dtype=np.float32)
    diff = [k for k in STATE_KEYS + SCALARS if not np.array_equal(np.asarray(by_numpy["state"][k]), np.asarray(on_device["state"][k]))]
    for j, (a, b) in enumerate(zip(by_numpy["recs"], on_device["recs"])):
        diff += [(k, j) for k in a if not np.array_equal(a[k], b[k])]
        assert b["y_pred"].dtype == np.float64 and b["y_pred_other"].dtype == np.float32
        ok = (np.array_equal(b["y_pred"], b["y_pred_other"].astype(np.float64)) if storage == "f32" else
              np.array_equal(b["y_pred_other"], b["y_pred"].astype(np.float32)))
        diff += [] if ok else [("download", j)]
    assert not diff, diff


def test_two_row_shards_each_with_its_ring():
    c = netlib.capi()
    cs = dict(RC.CASES[0], name="two shards", r=12, storage="f64", kernel="psmf_blk_filter6d")
    pb = RC.problem(cs)
    whole = _run_ring(c, cs, pb)
    nsh = 2

    def worker(rank, comm):
        row0, dl = shard_rows(cs["d"], nsh, rank)
        return _run_ring(c, cs, pb, row0=row0, dl=dl, comm=comm)

    _, out = netlib.run_ranks(nsh, worker, 150)
    for k in ("V", "P", "mu", "Q", "rho", "lam"):
        assert np.array_equal(np.asarray(out[0]["state"][k]), np.asarray(out[1]["state"][k])), k
    for a, b in zip(out[0]["recs"], out[1]["recs"]):
        assert np.array_equal(a["mu_hist"], b["mu_hist"])
    tol = 1e-11       # tests/test_hip_multishard.py, float64 storage
    C = np.vstack([o["state"]["C"] for o in out])
    errs = dict(C=relerr(C, whole["state"]["C"]), **{k: relerr(out[0]["state"][k], whole["state"][k]) for k in ("V", "P", "mu")})
    for j, w in enumerate(whole["recs"]):
        errs[f"y_pred {j}"] = relerr(np.hstack([o["recs"][j]["y_pred"] for o in out]), w["y_pred"])
    print("\nRING shards:", errs)
    assert max(errs.values()) < tol, errs


@pytest.mark.parametrize("which", ["PSMFIter", "rPSMFRecursive"])
def test_step_stream_of_the_classes(which):
    import rpsmf_amd as psmf

    d, r, T, chunk = 40, 4, 300, 64
    robust, recursive = which == "rPSMFRecursive", which == "rPSMFRecursive"
    cs = dict(RC.CASES[0], d=d, r=r, T=T, seed=77, storage="f64", robust=robust, dyn="cos_phase" if recursive else "random_walk",
              recursive=int(recursive), masked=False)
    pb = BC.problem(cs)
    ref = RC.reference(cs, pb)
    Y, mu0 = pb["Y"], pb["mu0"].reshape(-1, 1)
    chunks = [Y[a:a + chunk] for a in range(0, T, chunk)]
    if recursive:
        f = psmf.rPSMFRecursive(pb["theta"].reshape(-1, 1), pb["C0"], pb["V0"], mu0, pb["P0"], pb["Q"], pb["rho"], pb["lam"], psmf.CosPhase(r), storage="f64")
        f._update_every = 1
        f.optim_init(gam=RC.ADAM_LR)
        assert f.step_stream(iter(chunks), chunk, n_slots=3, keep_y_pred=True) == T
        tol = 1e-8        # tests/test_hip_dynamics.py: device-evaluated dynamics with the in-loop optimiser against the oracle
        assert relerr(f._theta[T].reshape(-1), ref["theta"]) < tol
    else:
        f = psmf.PSMFIter(np.zeros((0, 1)), pb["C0"], pb["V0"], mu0, pb["P0"], {k: pb["Q"] for k in range(T + 1)}, {k: pb["rho"] for k in range(T + 1)},
                          psmf.RandomWalk(), storage="f64")
        f.optim_init()
        assert f.step_stream(iter(chunks), chunk, keep_y_pred=True) == T
        tol = 1e-9        # tests/test_hip_dynamics.py / test_hip_filter.py: the random walk through the class surface, float64
    assert f._dev.ring == (chunk, 3 if recursive else 2) and f._dev.series_ring_info()["slots"].count(-1) == 0
    yp = np.array([f._y_pred[k].reshape(-1) for k in range(1, T + 1)])
    errs = dict(C=relerr(f._C[T], ref["C"]), V=relerr(f._V[T], ref["V"]), P=relerr(f._P[T], ref["P"]), mu=relerr(f._mu[T].reshape(-1), ref["mu"]),
                y_pred=relerr(yp, ref["y_pred"]))
    print(f"\nRING class {which}: {errs}")
    assert max(errs.values()) < tol, errs
    assert sorted(f._mu) == [T]                       # the mean history is not kept
    if not recursive:
        # step() after step_stream(): the ring handle gives way to a resident one, and the second epoch is the one that follows a
        # first epoch through step() (the same bar: the blocked engine cut at other steps rounds differently)
        y = np.vstack([np.zeros((1, d)), Y])
        g = psmf.PSMFIter(np.zeros((0, 1)), pb["C0"], pb["V0"], mu0, pb["P0"], {k: pb["Q"] for k in range(T + 1)}, {k: pb["rho"] for k in range(T + 1)},
                          psmf.RandomWalk(), storage="f64")
        g.optim_init()
        g.step(y, 1, T)
        g.optim_update(1)             # (theta is empty: this only names theta_1, as run() does between epochs)
        g.step(y, 2, T)
        f.optim_update(1)
        f.step(y, 2, T)
        assert f._dev.ring is None
        again = dict(C=relerr(f._C[T], g._C[T]), V=relerr(f._V[T], g._V[T]), P=relerr(f._P[T], g._P[T]), mu=relerr(f._mu[T], g._mu[T]))
        print(f"RING class {which}, step() after step_stream(): {again}")
        assert max(again.values()) < tol, again
    g = psmf.PSMFIter(np.zeros((0, 1)), pb["C0"], pb["V0"], mu0, pb["P0"], {0: pb["Q"]}, {0: pb["rho"]}, psmf.RandomWalk(), backend="numpy")
    with pytest.raises(NotImplementedError, match="numpy"):
        g.step_stream(iter(chunks), chunk)


def test_masked_metrics_of_resident_chunks_while_later_runs_are_queued():
    """psmf_masked_metrics reads the live C for its second sum, so on a ring handle it waits for the compute stream: taken right
    after runs were queued without a sync, the four sums are those of a resident handle run to the same step and asked for the
    same chunks -- bit for bit (the same kernel over the same rows, partial sums added in a fixed order)."""
    c = netlib.capi()
    cs = next(x for x in RC.CASES if x["name"] == "masked persistent")
    pb = RC.problem(cs)
    ch, Y, M, sig = cs["chunk"], pb["Y"], pb["M"], 2.0
    held = ((np.random.default_rng(5).random(M.shape) < 0.3) & (M == 0)).astype(np.uint8)      # held-out entries: never observed
    res, ring = _handle(c, cs, pb, ring=False), _handle(c, cs, pb, ring=True)
    try:
        res.upload_series(Y)
        res.upload_mask(M)

        def up(j):
            ring.upload_series(Y[j * ch:(j + 1) * ch], j * ch)
            ring.upload_mask(M[j * ch:(j + 1) * ch], j * ch)

        for j in range(3):
            up(j)
        ring.run(0, ch, sync=False)
        ring.run(ch, 2 * ch, sync=False)
        got = ring.masked_metrics(held[:ch], sig, 0)              # chunk 0, behind both runs
        res.run(0, ch)
        res.run(ch, 2 * ch)
        want = res.masked_metrics(held[:ch], sig, 0)
        print(f"\nRING masked metrics, chunk 0 after two chunks: {got} against {want}")
        assert np.array_equal(got, want) and got[3] == held[:ch].sum() > 0
        up(3)                                                       # evicts chunk 0
        ring.run(2 * ch, 3 * ch, sync=False)
        got = ring.masked_metrics(held[ch:3 * ch], sig, ch)       # two chunks in one call
        res.run(2 * ch, 3 * ch)
        want = res.masked_metrics(held[ch:2 * ch], sig, ch) + res.masked_metrics(held[2 * ch:3 * ch], sig, 2 * ch)
        print(f"RING masked metrics, chunks 1 and 2 after three: {got} against {want}")
        assert np.array_equal(got, want)
        # and the first sum against the host's over the same rows (float64 sums of about 0.1 x 74 x 257 terms)
        yp = ring.y_pred(ch, 2 * ch)
        assert relerr(got[0], float(np.sum(held[ch:3 * ch] * (yp - Y[ch:3 * ch]) ** 2))) < 1e-10
        with pytest.raises(c.PsmfError, match="-5.*step 1 is no longer resident"):
            ring.masked_metrics(held[:ch], sig, 0)
        ring.sync()
    finally:
        res.close()
        ring.close()


def test_launched_handle_with_chunks_above_the_graph_threshold():
    """The launched per-step engine captures its launches into a graph for runs of 256 steps and more, and the captured nodes
    carry the parameter block: with chunks of 260 steps every chunk rebuilds the graph with its own series_t0.  The bits of the
    resident handle cut at the same steps, and the oracle at the float64 bar."""
    c = netlib.capi()
    cs = RC.GRAPH_CASE
    pb = RC.problem(cs)
    res, ring, ref = _run_resident(c, cs, pb), _run_ring(c, cs, pb), RC.reference(cs, pb)
    diff = [k for k in STATE_KEYS + SCALARS if not np.array_equal(np.asarray(res["state"][k]), np.asarray(ring["state"][k]))]
    for j, (a, b) in enumerate(zip(res["recs"], ring["recs"])):
        diff += [(k, j) for k in a if not np.array_equal(a[k], b[k])]
    assert not diff, diff
    errs = {k: relerr(ring["state"][k], ref[k]) for k in ("C", "V", "P", "mu")}
    errs["y_pred"] = relerr(np.vstack([rec["y_pred"] for rec in ring["recs"]]), ref["y_pred"])
    print(f"\nRING graph case: bar {RC.bar(cs):.0e} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < RC.bar(cs), errs
