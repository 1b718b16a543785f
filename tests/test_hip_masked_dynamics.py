"""Masked handles with built-in dynamics: DeviceFilter(masked = 4 (MASKED_DYNAMICS), dyn_kind = cos-phase / ScaledWalk / Sinusoid / FourierBasis), theta
learned between epochs or inside the device time loop -- the serial stage's masked gradient g_f = n_obs w / N - h / N - ee w / N^2
(psmf_kernels.hip: serial_body; the persistent kernel's hub, psmf_pstep.hip, for cos-phase at r <= 32).  The cases of
tests/masked_dyn_cases.py (conditioned by tests/test_masked_dyn_cases_cpu.py) against the float64 model there; a run cut in two; two
uneven row shards; the series ring; the captured graph; the persistent against the launched form; the classes with `mask=`; the
refusals.  GPU only: `pytest -m gpu`; `-s` shows the error figures (each prints before it asserts).

Bars, the suite's own: C, V, P, the mean history and y_hat within gram_cases.bar (float64 storage 5e-9, float32 1e-5); gradsum 1e-7,
theta after an epoch 1e-7, theta stepped inside the loop 1e-6, predict 1e-8 (tests/test_hip_dynamics.py) -- with float32 storage
those four times 1e3; sharded against unsharded SHARD_BAR = 1e-11 with the replicated quantities bit-identical."""

import os

import numpy as np
import pytest

import gram_cases as GC
import masked_dyn_cases as D
import netlib
from oracle import psmf_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def bars(cs):
    x = 1e3 if cs["storage"] == "f32" else 1.0
    return dict(state=GC.bar(cs), gradsum=1e-7 * x, theta=1e-7 * x, theta_loop=1e-6 * x, pred=1e-8 * x)


def make_handle(c, cs, pb, row0=0, dl=None, **kw):
    nl = pb["nl"]
    ue = cs["update_every"]
    opts = dict(robust=cs["robust"], storage=cs["storage"], masked=c.MASKED_DYNAMICS, engine="step", dyn_kind=nl.device_kind, dyn_flags=nl.device_flags,
                dyn_terms=nl.device_terms, row0=row0, d_local=cs["d"] if dl is None else dl)
    if ue:
        opts.update(recursive=1 if cs["optim"] == "adam" else 2, update_every=ue, adam_lr=D.LR_LOOP if cs["optim"] == "adam" else D.LR_SGD)
    opts.update(kw)
    return c.DeviceFilter(cs["d"], cs["r"], **opts)


def start(f, cs, pb, sl=slice(None)):
    n = pb["nl"].n_params
    f.set_state(pb["C0"][sl], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=D.LAMBDA0 if cs["robust"] else 0.0, theta=pb["theta0"])
    f.zero_gradsum()
    if cs["update_every"] and cs["optim"] == "adam":
        f.set_adam(np.zeros(n), np.zeros(n))


def run_handle(c, cs, pb, parts=None, row0=0, dl=None, comm=None, **kw):
    """One handle (or row shard) over the case -> dict(s = the final state, X, yp, pred, records = [(gradsum, theta after the host's
    update) per epoch], cut = {k: (gradsum, theta) where a part ended}, kernel)."""
    d, T = cs["d"], cs["T"]
    dl = d if dl is None else dl
    sl = slice(row0, row0 + dl)
    parts = [(0, T)] if parts is None else parts
    n = pb["nl"].n_params
    f = make_handle(c, cs, pb, row0, dl, **kw)
    try:
        assert f.n_theta == n
        if comm is not None:
            f.comm_init_host(*comm)
        f.upload_series(np.ascontiguousarray(pb["Y"][:, sl]))
        f.upload_mask(np.ascontiguousarray(pb["M"][:, sl]))
        start(f, cs, pb, sl)
        records, cut = [], {}
        theta, am, av = pb["theta0"].copy(), np.zeros(n), np.zeros(n)
        for ep in range(1, (1 if cs["update_every"] else D.EPOCHS) + 1):
            if ep > 1:
                f.set_state(theta=theta)
                if cs["robust"]:
                    f.set_state(Q=pb["Q"], rho=pb["rho"], lambda0=D.LAMBDA0)
                f.zero_gradsum()
            for a, b in parts:
                f.run(a, b)
                if b < T:
                    s = f.get_state(want_C=False)
                    cut[b] = (s["gradsum"], s["theta"])
            s = f.get_state()
            if not cs["update_every"]:          # the optimiser between the epochs is the host's, from the device's gradient sum
                if cs["optim"] == "adam":
                    theta, am, av = O.adam_update(s["theta"], s["gradsum"], am, av, ep, lr=D.LR_EPOCH)
                else:
                    theta = O.sgd_update(s["theta"], s["gradsum"], lr=D.LR_SGD)
                records.append((s["gradsum"], theta))
        if not cs["update_every"]:
            f.set_state(theta=theta)
        return dict(s=s, X=f.mu_history(1, T), yp=f.y_pred(0, T), pred=f.predict(T, 3), records=records, cut=cut,
                    kernel=f.geometry()["filter_kernel"], theta=theta if not cs["update_every"] else s["theta"])
    finally:
        f.close()


def errs_of(cs, ref, got, sl=slice(None)):
    b = bars(cs)
    s = got["s"]
    out = [("C", D.relerr(s["C"], ref["C"][sl]), b["state"]), ("V", D.relerr(s["V"], ref["V"]), b["state"]), ("P", D.relerr(s["P"], ref["P"]), b["state"]),
           ("mu_hist", D.relerr(got["X"], ref["X"]), b["state"]), ("y_hat", D.relerr(got["yp"], ref["yp"][:, sl]), b["state"]),
           ("predict", D.relerr(got["pred"], ref["pred"][:, sl]), b["pred"])]
    if cs["update_every"]:
        out += [("theta_loop", D.relerr(s["theta"], ref["theta"]), b["theta_loop"]),
                ("gradsum", D.relerr(s["gradsum"], ref["gradsum"]) if np.any(ref["gradsum"]) else float(np.max(np.abs(s["gradsum"]))), b["gradsum"])]
    else:
        for ep, ((g, th), (rg, rth)) in enumerate(zip(got["records"], ref["records"]), 1):
            out += [(f"gradsum{ep}", D.relerr(g, rg), b["gradsum"]), (f"theta{ep}", D.relerr(th, rth), b["theta"])]
    return out


def report(what, errs):
    worst = max(errs, key=lambda e: (e[1] / e[2]) if np.isfinite(e[1]) else np.inf)
    print(f"\nMASKED DYNAMICS {what}: " + " ".join(f"{k}={e:.3e}" for k, e, _ in errs) + f"  worst {worst[0]} at {worst[1] / worst[2]:.3g} of its bar")
    bad = [e for e in errs if not e[1] < e[2]]
    assert not bad, (what, bad)


@pytest.mark.parametrize("cs", D.CASES, ids=D.IDS)
def test_masked_dynamics_vs_model(cs):
    """Every case through DeviceFilter against the model."""
    from rpsmf_amd import _capi as c

    pb, ref = D.reference(cs)
    got = run_handle(c, cs, pb)
    # cos-phase at r <= 32: the persistent kernel's masked instance; the kinds with a matrix in them: the launched form
    assert got["kernel"] == ("psmf_pstep_k" if cs["dyn"] == "cos_phase" and os.environ.get("PSMF_STEP_PERSISTENT") != "0" else "psmf_sweep_solve")
    report(D.IDS[D.CASES.index(cs)], errs_of(cs, ref, got))


@pytest.mark.parametrize("dyn,ue", [("cos_phase", 2), ("sinusoid", 3), ("fourier2", 0)])
def test_run_cut_in_two(dyn, ue):
    """run(0, T/2) then run(T/2, T): the first = 1 preparation in mid-series (mu_bar, P_bar = F P F^T + Q and the look-ahead Gram formed
    again from the carried state), the gradient sum and theta at the cut against the model's."""
    from rpsmf_amd import _capi as c

    cs = D.find(dyn, robust=True, update_every=ue)
    pb, ref = D.reference(cs)
    h = cs["T"] // 2                              # (in-loop: 15 of 30 with update_every = 2, 20 of 40 with 3 -- inside an optimiser window)
    got = run_handle(c, cs, pb, parts=[(0, h), (h, cs["T"])])
    snap = D.run_model(cs, pb, keep=(h,))["snap"][h]
    b = bars(cs)
    assert np.any(snap["gradsum"])
    errs = errs_of(cs, ref, got) + [("gradsum at the cut", D.relerr(got["cut"][h][0], snap["gradsum"]), b["gradsum"]),
                                    ("theta at the cut", D.relerr(got["cut"][h][1], snap["theta"]), b["theta_loop"])]
    report(f"cut at {h} {dyn}", errs)


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
def test_two_uneven_shards(robust):
    """(300, 10) Sinusoid with Adam inside the loop on two uneven row shards under the host communicator: gathered C and y_hat equal
    the unsharded handle's within SHARD_BAR; theta, the gradient sum, V, P and the mean history are replicated and bit-identical."""
    from rpsmf_amd import _capi as c

    cs = D.find("sinusoid", robust=robust, update_every=3)
    pb, ref = D.reference(cs)
    h = cs["T"] - 2                               # (38 of 40, update_every = 3: the gradient sum of an open window at the cut)
    parts = [(0, h), (h, cs["T"])]
    whole = run_handle(c, cs, pb, parts=parts)
    shards = (187, 113)
    row0 = (0, shards[0])
    _, out = netlib.run_ranks(2, lambda rank, comm: run_handle(c, cs, pb, parts=parts, row0=row0[rank], dl=shards[rank], comm=comm), 100)
    for k in ("V", "P", "mu", "theta", "gradsum"):
        assert np.array_equal(out[0]["s"][k], out[1]["s"][k]), k
    assert np.array_equal(out[0]["X"], out[1]["X"]) and np.array_equal(out[0]["cut"][h][0], out[1]["cut"][h][0])
    assert np.any(out[0]["cut"][h][0])
    Cg = np.concatenate([o["s"]["C"] for o in out])
    ypg = np.concatenate([o["yp"] for o in out], axis=1)
    predg = np.concatenate([o["pred"] for o in out], axis=1)
    vs = [("vs whole " + k, D.relerr(a, b), GC.SHARD_BAR) for k, a, b in (
        ("C", Cg, whole["s"]["C"]), ("y_hat", ypg, whole["yp"]), ("X", out[0]["X"], whole["X"]), ("V", out[0]["s"]["V"], whole["s"]["V"]),
        ("P", out[0]["s"]["P"], whole["s"]["P"]), ("theta", out[0]["s"]["theta"], whole["s"]["theta"]),
        ("gradsum at the cut", out[0]["cut"][h][0], whole["cut"][h][0]))]
    gathered = dict(out[0], s=dict(out[0]["s"], C=Cg), yp=ypg, pred=predg)
    report(f"two shards {'rPSMF' if robust else 'PSMF'}", vs + errs_of(cs, ref, gathered))


def test_series_ring_same_bits():
    """(300, 10) Sinusoid rPSMF, Adam in the loop, through series_ring(16, 3) fed by run_stream: the bits of the resident handle cut at
    the same steps, theta and the gradient sum included."""
    from rpsmf_amd import _capi as c

    cs = D.find("sinusoid", robust=True, update_every=3)
    pb, _ = D.reference(cs)
    T, ch = cs["T"], 16
    Y, M = np.ascontiguousarray(pb["Y"]), np.ascontiguousarray(pb["M"])
    spans = [(a, min(a + ch, T)) for a in range(0, T, ch)]
    out = []
    for ring in (False, True):
        f = make_handle(c, cs, pb)
        try:
            if ring:
                f.series_ring(ch, 3)
            else:
                f.upload_series(Y)
                f.upload_mask(M)
            start(f, cs, pb)
            if ring:
                yps = [yp for _, _, yp in f.run_stream(((Y[a:b], M[a:b]) for a, b in spans), y_pred_dtype=np.float64)]
            else:
                yps = []
                for a, b in spans:
                    f.run(a, b)
                    yps.append(f.y_pred(a, b - a))
            s = f.get_state()
            assert s["k"] == T and f.geometry()["filter_kernel"] == "psmf_sweep_solve"
            out.append(dict(C=s["C"], V=s["V"], P=s["P"], mu=s["mu"], theta=s["theta"], gradsum=s["gradsum"], rho=s["rho"], yp=np.concatenate(yps)))
        finally:
            f.close()
    assert np.any(out[0]["gradsum"]) and np.max(np.abs(out[0]["theta"] - pb["theta0"])) > 0
    for k in out[0]:
        assert np.all(np.isfinite(out[0][k])) and np.array_equal(out[0][k], out[1][k]), k


def test_captured_graph_same_bits():
    """A run longer than the graph chunk of 256 steps: the captured graph gives the bits of the eager launches (the count that the
    gradient reads is the one of the step, in the graph's order of launches as in the eager one)."""
    from rpsmf_amd import _capi as c
    from rpsmf_amd import nonlinearities as NL

    d, r, n = 64, 6, 300
    rng = np.random.default_rng(31)
    Y = np.cumsum(0.3 * rng.standard_normal((n, d)), axis=0) + 3.0 * rng.random(d)
    M = (rng.random((n, d)) > 0.4).astype(np.uint8)
    M[40] = 0
    nl = NL.Sinusoid(r)
    theta = D.theta_for(nl, rng, r)
    C0 = 0.3 * rng.random((d, r))
    out = []
    for use_graph in (False, True):
        f = c.DeviceFilter(d, r, robust=True, storage="f64", masked=c.MASKED_DYNAMICS, engine="step", dyn_kind=nl.device_kind, dyn_flags=nl.device_flags,
                           recursive=1, update_every=7, adam_lr=1e-3, use_graph=use_graph)
        try:
            f.upload_series(Y)
            f.upload_mask(M)
            f.set_state(C0, 2 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.full(r, 0.3), rho=1.0, lambda0=D.LAMBDA0, theta=theta)
            f.zero_gradsum()
            f.set_adam(np.zeros(nl.n_params), np.zeros(nl.n_params))
            f.run(0, n)
            assert f.geometry()["graph_chunk"] == (256 if use_graph else 0)
            s = f.get_state()
            out.append(dict(C=s["C"], V=s["V"], P=s["P"], theta=s["theta"], gradsum=s["gradsum"], X=f.mu_history(1, n), yp=f.y_pred(0, n)))
        finally:
            f.close()
    assert np.any(out[0]["gradsum"]) and np.max(np.abs(out[0]["theta"] - theta)) > 0
    for k in out[0]:
        assert np.all(np.isfinite(out[0][k])) and np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
@pytest.mark.parametrize("ue", [0, 2], ids=["epochs", "in_loop"])
def test_persistent_against_launched_form(robust, ue):
    """The cos-phase case on the persistent kernel's masked instance (the hub carries the step's observed count from the Gram
    hand-off of the step before) and, PSMF_STEP_PERSISTENT=0, on the launched form: the same filter within the bars of
    tests/test_hip_step_engine_net.py (masked 5e-9, gradsum 1e-7)."""
    from rpsmf_amd import _capi as c

    cs = D.find("cos_phase", robust=robust, update_every=ue)
    pb, ref = D.reference(cs)
    got = {}
    for name, env in (("persistent", {"PSMF_STEP_PERSISTENT": "1"}), ("launched", {"PSMF_STEP_PERSISTENT": "0"})):
        with netlib.env(env):
            got[name] = run_handle(c, cs, pb)
    assert got["persistent"]["kernel"] == "psmf_pstep_k" and got["launched"]["kernel"] == "psmf_sweep_solve"
    a, b = got["persistent"], got["launched"]
    errs = [(k, D.relerr(a["s"][k], b["s"][k]), 5e-9) for k in ("C", "V", "P")] + [(k, D.relerr(a[k], b[k]), 5e-9) for k in ("X", "yp")]
    errs += [("theta", D.relerr(a["theta"], b["theta"]), 1e-6 if ue else 1e-7)]
    errs += [(f"gradsum{j}", D.relerr(x[0], y[0]), 1e-7) for j, (x, y) in enumerate(zip(a["records"], b["records"]), 1)]
    for name in got:
        errs += [(f"{name} {k}", e, bar) for k, e, bar in errs_of(cs, ref, got[name])]
    report(f"persistent against launched {'rPSMF' if robust else 'PSMF'} ue={ue}", errs)


@pytest.mark.parametrize("robust", [False, True], ids=["PSMF", "rPSMF"])
def test_random_walk_is_the_masked_handle_of_before(robust):
    """masked = MASKED_DYNAMICS with the random walk is masked = 1, bit for bit, on the persistent and on the launched form."""
    from rpsmf_amd import _capi as c

    cs = D.find("cos_phase", robust=robust)
    pb = D.problem(cs)
    T = cs["T"]
    for env in ({"PSMF_STEP_PERSISTENT": "1"}, {"PSMF_STEP_PERSISTENT": "0"}):
        out = []
        with netlib.env(env):
            for masked in (1, c.MASKED_DYNAMICS):
                f = c.DeviceFilter(cs["d"], cs["r"], robust=robust, storage="f64", masked=masked, engine="step")
                try:
                    f.upload_series(pb["Y"])
                    f.upload_mask(pb["M"])
                    f.set_state(pb["C0"], pb["V0"], pb["P0"], pb["Q"], pb["mu0"], rho=pb["rho"], lambda0=D.LAMBDA0 if robust else 0.0)
                    f.run(0, T)
                    s = f.get_state()
                    out.append((f.geometry()["filter_kernel"], s["C"], s["V"], s["P"], f.mu_history(1, T), f.y_pred(0, T), f.step_scalars(0, T)))
                finally:
                    f.close()
        assert out[0][0] == out[1][0] == ("psmf_pstep_k" if env["PSMF_STEP_PERSISTENT"] == "1" else "psmf_sweep_solve")
        for a, b in zip(out[0][1:], out[1][1:]):
            assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def _ydict(A):
    return {k + 1: A[k][:, None].copy() for k in range(A.shape[0])}


def test_PSMFIter_run_with_a_mask():
    """PSMFIter(...).run(y, T, 2, 3, mask=m): two epochs with Adam between them and the roll-out, against the model."""
    import rpsmf_amd as psmf

    cs = D.find("sinusoid")
    pb, ref = D.reference(cs)
    d, r, T = cs["d"], cs["r"], cs["T"]
    f = psmf.PSMFIter(pb["theta0"].reshape(-1, 1), pb["C0"], pb["V0"], pb["mu0"].reshape(-1, 1), pb["P0"], {k: pb["Q"] for k in range(T + 1)},
                      {k: pb["rho"] for k in range(T + 1)}, pb["nl"], storage="f64")
    f.run(_ydict(pb["Y"]), T, D.EPOCHS, 3, mask=_ydict(pb["M"]))
    assert f._dev.masked == 4 and f._dev.geometry()["engine"] == "step"
    b = bars(cs)
    yp = np.array([f._y_pred[k].reshape(-1) for k in range(1, T + 4)])
    # predict(i) precedes optim_update(i) (psmf.py:207-212): the roll-out of the last epoch uses the theta that epoch ran with
    pred = O.predict_rollout(ref["C"], ref["mu"], ref["records"][-2][1], D.ClosedFormDyn(pb["nl"]), T, 3)
    errs = [("C", D.relerr(f._C[T], ref["C"]), b["state"]), ("V", D.relerr(f._V[T], ref["V"]), b["state"]), ("P", D.relerr(f._P[T], ref["P"]), b["state"]),
            ("mu", D.relerr(f._mu[T].reshape(-1), ref["mu"]), b["state"]), ("y_hat", D.relerr(yp[:T], ref["yp"]), b["state"]),
            ("predict", D.relerr(yp[T:], pred), b["pred"]), ("gradsum", D.relerr(f._gradsum.reshape(-1), ref["records"][-1][0]), b["gradsum"])]
    errs += [(f"theta{i}", D.relerr(f._theta[i].reshape(-1), ref["records"][i - 1][1]), b["theta"]) for i in range(1, D.EPOCHS + 1)]
    report("PSMFIter.run(mask=)", errs)
    # the array form of y and mask (row 0 unused), and the unchanged content: nothing is uploaded again, the same numbers
    key = (f._session.series_key, f._session.mask_key)
    f2 = psmf.PSMFIter(pb["theta0"].reshape(-1, 1), pb["C0"], pb["V0"], pb["mu0"].reshape(-1, 1), pb["P0"], pb["Q"], pb["rho"], pb["nl"], storage="f64")
    f2.optim_init()
    Y1, M1 = np.vstack([np.zeros((1, d)), pb["Y"]]), np.vstack([np.ones((1, d)), pb["M"]])
    f2.step(Y1, 1, T, mask=M1)
    assert (f2._session.series_key, f2._session.mask_key) == key
    assert D.relerr(f2._gradsum.reshape(-1), ref["records"][0][0]) < b["gradsum"]


def test_rPSMFRecursive_with_a_mask():
    """rPSMFRecursive.step(y, T, mask=m), Adam every 3 steps inside the device loop, and the roll-out, against the model."""
    import rpsmf_amd as psmf

    cs = D.find("sinusoid", robust=True, update_every=3)
    pb, ref = D.reference(cs)
    T = cs["T"]
    f = psmf.rPSMFRecursive(pb["theta0"].reshape(-1, 1), pb["C0"], pb["V0"], pb["mu0"].reshape(-1, 1), pb["P0"], pb["Q"], pb["rho"], D.LAMBDA0, pb["nl"],
                            storage="f64")
    f._update_every = cs["update_every"]
    f.optim_init(gam=D.LR_LOOP)
    f.step(_ydict(pb["Y"]), T, mask=_ydict(pb["M"]))
    f.predict(T, 3)
    assert f._dev.masked == 4
    b = bars(cs)
    yp = np.array([f._y_pred[k].reshape(-1) for k in range(1, T + 4)])
    report("rPSMFRecursive.step(mask=)", [
        ("C", D.relerr(f._C[T], ref["C"]), b["state"]), ("P", D.relerr(f._P[T], ref["P"]), b["state"]), ("y_hat", D.relerr(yp[:T], ref["yp"]), b["state"]),
        ("theta", D.relerr(f._theta[T].reshape(-1), ref["theta"]), b["theta_loop"]), ("predict", D.relerr(yp[T:], ref["pred"]), b["pred"])])


def test_mask_none_changes_nothing():
    """mask=None is the call without the keyword, bit for bit."""
    import rpsmf_amd as psmf

    cs = D.find("cos_phase")
    pb = D.problem(cs)
    T = cs["T"]
    out = []
    for kw in ({}, {"mask": None}):
        f = psmf.PSMFIter(pb["theta0"].reshape(-1, 1), pb["C0"], pb["V0"], pb["mu0"].reshape(-1, 1), pb["P0"], pb["Q"], pb["rho"], pb["nl"], storage="f64")
        f.run(_ydict(pb["Y"]), T, 2, 3, **kw)
        assert f._dev.masked == 0
        g = psmf.rPSMFRecursive(pb["theta0"].reshape(-1, 1), pb["C0"], pb["V0"], pb["mu0"].reshape(-1, 1), pb["P0"], pb["Q"], pb["rho"], D.LAMBDA0, pb["nl"],
                                storage="f64")
        g.run(_ydict(pb["Y"]), T, 3, update_every=2, **kw)
        out.append((np.asarray(f._C[T]), f._theta[2], np.array([f._y_pred[k] for k in range(1, T + 4)]), np.asarray(g._C[T]), g._theta[T]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_refusals_by_message():
    """What a masked handle does not run is refused by name: MLE-SMF / TMF and the ExperimentImpute filter (masked = 1) with dynamics, host-stepped dynamics, a row noise with
    learned theta, R_k / Q_k schedules; and by the classes: a host-stepped callable, schedules, a non-uniform R with learned theta,
    the numpy back end."""
    from rpsmf_amd import _capi as c
    import rpsmf_amd as psmf

    d, r, T = 40, 5, 6
    rng = np.random.default_rng(4)
    for masked in (2, 3):
        with pytest.raises(ValueError, match=r"MLE-SMF\) / 3 \(TMF\) are random-walk"):
            c.DeviceFilter(d, r, storage="f64", masked=masked, engine="step", dyn_kind=c.DYN_COS_PHASE)
    with pytest.raises(ValueError, match="masked handles evaluate f_theta on the device: not with PSMF_DYN_HOST"):
        c.DeviceFilter(d, r, storage="f64", masked=c.MASKED_DYNAMICS, engine="step", dyn_kind=c.DYN_HOST)
    with pytest.raises(ValueError, match="masked handles with nonuniform_R = 1 do not learn theta"):
        c.DeviceFilter(d, r, storage="f64", masked=c.MASKED_DYNAMICS, engine="step", dyn_kind=c.DYN_COS_PHASE, nonuniform_R=True)
    for masked in (1, c.MASKED_DYNAMICS):          # the random walk with a row noise stays
        c.DeviceFilter(d, r, storage="f64", masked=masked, engine="step", nonuniform_R=True).close()
    with pytest.raises(ValueError, match="masked = 1 handles are random-walk filters.*masked = 4 runs f_theta"):
        c.DeviceFilter(d, r, storage="f64", masked=1, engine="step", dyn_kind=c.DYN_COS_PHASE)
    with pytest.raises(ValueError, match="masked must be 0 .. 4"):
        c.DeviceFilter(d, r, storage="f64", masked=5, engine="step")
    f = c.DeviceFilter(d, r, storage="f64", masked=c.MASKED_DYNAMICS, engine="step", dyn_kind=c.DYN_COS_PHASE)
    try:
        assert f.n_theta == r
        with pytest.raises(ValueError, match="psmf_set_schedules: masked handles take a constant"):
            f.set_schedules(np.ones(T + 1), None)
        with pytest.raises(ValueError, match="psmf_set_q_matrix_schedule: masked handles take a constant Q"):
            f.set_q_matrix_schedule(np.tile(np.eye(r), (T + 1, 1, 1)))
    finally:
        f.close()
    Y, M = _ydict(rng.standard_normal((T, d))), _ydict((rng.random((T, d)) > 0.4).astype(np.uint8))
    C0, V0, P0, Q, mu0 = 0.1 * rng.standard_normal((d, r)), 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros((r, 1))
    th = 0.05 * np.ones((r, 1))

    def tanh_f(theta, x, t):
        return np.tanh(np.asarray(x).reshape(-1, 1) + np.asarray(theta).reshape(-1, 1))

    mk = lambda nl=None, R=1.0, Qs=None, **kw: psmf.PSMFIter(th, C0, V0, mu0, P0, Q if Qs is None else Qs, R, psmf.CosPhase(r) if nl is None else nl, **kw)
    for f, what in ((mk(tanh_f, recognise=False), "host-stepped callables"),
                    (mk(R={k: 1.0 + 0.1 * k for k in range(T + 1)}), "schedules that vary with k"),
                    (mk(Qs={k: (1.0 + k) * Q for k in range(T + 1)}), "schedules that vary with k"),
                    (mk(R=np.linspace(0.5, 2.0, d)), "non-uniform diagonal R with learned theta"),
                    (mk(backend="numpy"), 'backend="numpy"')):
        f.optim_init()
        with pytest.raises(NotImplementedError, match=what):
            f.step(Y, 1, T, mask=M)
    g = psmf.PSMFRecursive(th, C0, V0, mu0, P0, Q, 1.0, psmf.CosPhase(r), backend="numpy")
    g._update_every = 2
    g.optim_init()
    with pytest.raises(NotImplementedError, match='backend="numpy"'):
        g.step(Y, T, mask=M)
    with pytest.raises(NotImplementedError):
        psmf.PSMFIterMissing()
