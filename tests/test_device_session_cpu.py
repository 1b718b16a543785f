"""Which device calls the filter classes make, handle by handle -- checked without a GPU: `_capi.DeviceFilter` is replaced by a stand-in
that records every call (constructor keywords, method, and per argument None / shape / scalar; uploads with a content hash) and answers
with correctly shaped arrays.  The traces of the scenarios below were recorded at the commit BEFORE the classes' device plumbing moved
into rpsmf_amd/_session.py (`python tests/test_device_session_cpu.py --record` there) and are kept in
tests/golden/session_call_trace_parent.json: the classes must make the same calls, call for call.  The one deliberate difference
(a handle replaced for a Q-matrix schedule once a device epoch has run) has its own test at the end."""

import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rpsmf_amd as psmf  # noqa: E402
from rpsmf_amd import _capi  # noqa: E402
from rpsmf_amd.learning_rate import BaseLearningRate  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "session_call_trace_parent.json")
D, R, T = 8, 3, 6


def _describe(a):
    if a is None or isinstance(a, (bool, str)):
        return a
    if isinstance(a, (int, float, np.integer, np.floating)):
        return float(a) if isinstance(a, (float, np.floating)) else int(a)
    if isinstance(a, np.ndarray):
        return {"shape": list(a.shape)}
    if isinstance(a, (tuple, list)):
        return [_describe(x) for x in a]
    return type(a).__name__


def _digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.blake2b(a.tobytes(), digest_size=8).hexdigest() + ":" + a.dtype.str


class Recorder:
    """Stand-in for _capi.DeviceFilter: logs [handle, method, args, kwargs] into the class-level `log`, returns shaped arrays."""

    log, handles = [], 0
    _VOID = ("zero_gradsum", "set_adam", "run", "set_schedules", "set_q_matrix_schedule", "set_row_noise", "set_noise_rotation", "close")

    def __init__(self, d, r, **kw):
        self.id, Recorder.handles = Recorder.handles, Recorder.handles + 1
        self.d = self.d_local = int(d)
        self.r = int(r)
        self.dyn_kind = int(kw.get("dyn_kind", _capi.DYN_RANDOM_WALK))
        self.n_theta = _capi.dyn_n_theta(self.dyn_kind, self.r, int(kw.get("dyn_flags", 0)), int(kw.get("dyn_terms", 0)))
        self.store_y_pred, self.masked, self.ring, self.T = True, int(kw.get("masked", 0)), None, 0
        self._rng = np.random.default_rng(1000 + self.id)
        self._rec("__init__", (d, r), kw)

    def _rec(self, name, args=(), kw=None, **extra):
        entry = [self.id, name, [_describe(a) for a in args], {k: _describe(v) for k, v in sorted((kw or {}).items())}]
        Recorder.log.append(entry + ([extra] if extra else []))

    def __getattr__(self, name):
        if name not in Recorder._VOID:
            raise AttributeError(name)
        return lambda *a, **kw: self._rec(name, a, kw)

    def _spd(self):
        A = self._rng.standard_normal((self.r, self.r))
        return 0.5 * np.eye(self.r) + 0.05 * A @ A.T

    def set_state(self, C_=None, V=None, P=None, Q=None, mu=None, rho=None, lambda0=None, theta=None):
        self._rec("set_state", (C_, V, P, Q, mu), dict(rho=rho, lambda0=lambda0, theta=theta))

    def get_state(self, want_C=True):
        self._rec("get_state", (), dict(want_C=want_C))
        g = self._rng
        return dict(C=g.standard_normal((self.d, self.r)) if want_C else None, V=0.2 * self._spd(), P=self._spd(), Q=0.1 * self._spd(),
                    mu=g.standard_normal(self.r), theta=0.1 + 0.1 * g.random(self.n_theta), gradsum=g.standard_normal(self.n_theta),
                    rho=1.5, lam=2.5 + self.d, s=0.1, eta=1.0, N=1.1, phi=1.0, omega=1.0, k=0)

    def upload_series(self, Y, t0=0, T_total=None):
        self._rec("upload_series", (Y,), dict(t0=t0, T_total=T_total), content=_digest(Y))
        self.T = max(self.T, t0 + Y.shape[0] if T_total is None else T_total)

    def upload_mask(self, M, t0=0):
        self._rec("upload_mask", (M,), dict(t0=t0), content=_digest(M))

    def series_ring(self, chunk, n_slots=2):
        self._rec("series_ring", (chunk, n_slots))
        self.ring = (int(chunk), int(n_slots))

    def run_stream(self, chunks, k0=0, y_pred_dtype=None):
        self._rec("run_stream", (), dict(k0=k0))
        kb = k0
        for Y in chunks:
            Y = np.asarray(Y)
            self._rec("run_stream.chunk", (Y,), content=_digest(Y))
            yield kb, kb + Y.shape[0], self._rng.standard_normal(Y.shape)
            kb += Y.shape[0]

    def step_host(self, k, mu_bar, P_bar, want_PQ=True):
        self._rec("step_host", (k, mu_bar, P_bar))
        return 0.5 * np.asarray(mu_bar).reshape(-1), self._rng.standard_normal(self.r), self._spd(), 0.1 * self._spd()

    def y_pred(self, t0, nt, dtype=np.float64):
        self._rec("y_pred", (t0, nt))
        return self._rng.standard_normal((nt, self.d)).astype(dtype)

    def mu_history(self, k0, nk):
        self._rec("mu_history", (k0, nk))
        return self._rng.standard_normal((nk, self.r))

    def predict(self, T_, n_pred):
        self._rec("predict", (T_, n_pred))
        return self._rng.standard_normal((n_pred, self.d))

    def project(self, mu):
        self._rec("project", (np.asarray(mu),))
        return self._rng.standard_normal((np.asarray(mu).reshape(-1, self.r).shape[0], self.d))

    def sq_error(self, t0, nt):
        self._rec("sq_error", (t0, nt))
        return 3.0

    def predict_sq_error(self, T_, Y_true):
        self._rec("predict_sq_error", (T_, np.asarray(Y_true)))
        return 1.0


# ---------------------------------------------------------------------------------------------------------------------
# scenarios: each takes a pytest MonkeyPatch and returns what it observed beside the call trace (or None)
# ---------------------------------------------------------------------------------------------------------------------
def _series(seed=0, n=T + 2):
    Y = np.random.default_rng(seed).standard_normal((n, D))
    return Y, {k + 1: Y[k][:, None].copy() for k in range(n)}


def _mask(seed=5):
    M = (np.random.default_rng(seed).random((T, D)) < 0.7).astype(float)
    return M, {k + 1: M[k][:, None].copy() for k in range(T)}


def _make(cls=None, Qs=None, Rs=None, nl=None, robust_args=None, **kw):
    cls = cls or psmf.PSMFIter
    rng = np.random.default_rng(3)
    nl = nl if nl is not None else psmf.CosPhase(R)
    n = getattr(nl, "n_params", 0)
    theta0 = 0.05 + 0.1 * rng.random((n, 1))
    C0 = rng.standard_normal((D, R))
    args = (theta0, C0, 0.1 * np.eye(R), np.zeros((R, 1)), np.eye(R))
    if robust_args is not None:
        return cls(*args, 0.1 * np.eye(R), robust_args.pop("R0", 1.0), 2.5, nl, **robust_args, **kw)
    Qs = Qs if Qs is not None else {k: 0.1 * np.eye(R) for k in range(T + 1)}
    Rs = Rs if Rs is not None else {k: 1.0 for k in range(T + 1)}
    return cls(*args, Qs, Rs, nl, **kw)


def _two_epochs(f, y, **kw):
    f.optim_init()
    f.step(y, 1, T, **kw)
    f.predict(1, T, 2)
    f.optim_update(1)
    f.step(y, 2, T, **kw)


def two_epochs_same_series(mp):
    _two_epochs(_make(), _series()[1])


def series_changed_in_place(mp):
    Y = np.vstack([np.zeros((1, D)), _series()[0]])
    f = _make()
    f.optim_init()
    f.step(Y, 1, T)
    f.optim_update(1)
    Y[2, 3] += 1.0
    f.step(Y, 2, T)


def mask_on_off_on(mp):
    f, y, m = _make(), _series()[1], _mask()[1]
    f.optim_init()
    for i, mk in enumerate((m, None, m), 1):
        f.step(y, i, T, mask=mk)
        f.optim_update(i)


def mask_as_dict_then_array(mp):
    f, y, (M, m) = _make(), _series()[1], _mask()
    f.optim_init()
    f.step(y, 1, T, mask=m)
    f.optim_update(1)
    f.step(y, 2, T, mask=np.vstack([np.ones((1, D)), M]))


def nonuniform_diagonal_R(mp):
    rho = np.linspace(0.5, 2.0, D)
    _two_epochs(_make(Rs={k: rho for k in range(T + 1)}), _series()[1])


def dense_R(mp):
    A = np.random.default_rng(8).standard_normal((D, D))
    Rm = np.eye(D) + 0.1 * A @ A.T
    _two_epochs(_make(Rs={k: Rm for k in range(T + 1)}), _series()[1])


def scalar_schedules(mp):
    f = _make(Qs={k: (0.1 + 0.01 * k) * np.eye(R) for k in range(T + 1)}, Rs={k: 1.0 + 0.1 * k for k in range(T + 1)})
    _two_epochs(f, _series()[1])


def _q_matrices(T_=T, const_to=0):
    rng, Qs = np.random.default_rng(9), {}
    for k in range(T_ + 1):
        A = rng.standard_normal((R, R))
        Qs[k] = 0.05 * np.eye(R) + (0.01 * A @ A.T if k > const_to else 0.0)
    return Qs


def q_matrix_schedule_on_device(mp):
    _two_epochs(_make(Qs=_q_matrices(), nl=psmf.RandomWalk()), _series()[1])


def q_matrix_schedule_host_stepped(mp):
    mp.setattr(psmf.PSMFIter, "_Q_MATRIX_SCHEDULE_MAX_BYTES", 0)
    _two_epochs(_make(Qs=_q_matrices(), nl=psmf.RandomWalk()), _series()[1])


def step_stream_step(mp):
    f, (Y, y) = _make(), _series()
    f.optim_init()
    f.step(y, 1, T)
    f.optim_update(1)
    n = f.step_stream([Y[0:3], Y[3:6], Y[6:8]], chunk=3, n_slots=2, i=2, keep_y_pred=True)
    f.optim_update(2)
    f.step(y, 3, T)
    return dict(streamed=n, kept=sorted(f._y_pred) if isinstance(f._y_pred, dict) else None)


class _Halving(BaseLearningRate):
    def get(self, t):
        return 1e-2 / (1 + t)


def _recursive(cls, custom, **robust):
    f = _make(cls, robust_args=dict(robust) if robust else None)
    if custom:
        f._update_every = 2
        f.optim_init(gam=_Halving())
        f.step(_series()[1], T)
        f.predict(T, 2)
    else:
        f.run(_series()[1], T, 2, update_every=2)
    f.step(_series()[1], T)
    return dict(theta_keys=sorted(f._theta))


def recursive_adam(mp):
    return _recursive(psmf.PSMFRecursive, False)


def recursive_custom_learning_rate(mp):
    return _recursive(psmf.PSMFRecursive, True)


def robust_recursive_adam(mp):
    return _recursive(psmf.rPSMFRecursive, False, fixed_lambda=False)


def robust_recursive_custom_learning_rate(mp):
    return _recursive(psmf.rPSMFRecursive, True, fixed_lambda=False)


def _robust_iter(fixed, R0=1.0):
    f = _make(psmf.rPSMFIter, robust_args=dict(fixed_lambda=fixed, R0=R0))
    _two_epochs(f, _series()[1])
    return {"lambda": {str(k): float(v) for k, v in dict(f._lambda).items()}, "lambda_default": float(f._lambda[99]) if fixed else None,
            "Q": {str(k): _describe(np.asarray(v)) for k, v in f._Q.items()}, "R": {str(k): _describe(np.asarray(v, dtype=float)) for k, v in f._R.items()},
            "R_sum": float(np.sum(f._R[T]))}


def robust_iter_fixed_lambda(mp):
    return _robust_iter(True)


def robust_iter_growing_lambda(mp):
    return _robust_iter(False)


def robust_iter_row_noise(mp):
    return _robust_iter(False, R0=np.linspace(0.5, 2.0, D))


def unrecognised_callable(mp):
    f = _make(nl=lambda theta, x, t: np.tanh(x), recognise=False)
    _two_epochs(f, _series()[1])


def _tracked(other_y):
    class Tracked(psmf.TrackingMixin, psmf.PSMFIter):
        pass

    f, (Y, y) = _make(Tracked), _series()
    f.optim_init()
    f.errors_init(y, T, 1, 2)
    f.step({k: y[k] for k in range(1, T + 1)}, 1, T)
    f.predict(1, T, 2)
    f.optim_update(1)
    f.errors_update(1, _series(seed=11)[1] if other_y else y, T, 2)
    return dict(on_device=f._tracking_on_device, E_train=f._E_train[1] if not other_y else None)


def tracking_resident_series(mp):
    return _tracked(False)


def tracking_other_series(mp):
    return _tracked(True)


SCENARIOS = [two_epochs_same_series, series_changed_in_place, mask_on_off_on, mask_as_dict_then_array, nonuniform_diagonal_R, dense_R,
             scalar_schedules, q_matrix_schedule_on_device, q_matrix_schedule_host_stepped, step_stream_step, recursive_adam,
             recursive_custom_learning_rate, robust_recursive_adam, robust_recursive_custom_learning_rate, robust_iter_fixed_lambda,
             robust_iter_growing_lambda, robust_iter_row_noise, unrecognised_callable, tracking_resident_series, tracking_other_series]


def trace_of(scenario, mp):
    mp.setattr(_capi, "DeviceFilter", Recorder)
    Recorder.log, Recorder.handles = [], 0
    seen = scenario(mp)
    return json.loads(json.dumps(dict(calls=Recorder.log, observed=seen)))


def _calls(trace, handle=None, name=None):
    return [c for c in trace["calls"] if (handle is None or c[0] == handle) and (name is None or c[1] == name)]


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as fp:
        return json.load(fp)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda s: s.__name__)
def test_same_device_calls_as_before_the_session_object(scenario, parent, monkeypatch):
    got, want = trace_of(scenario, monkeypatch), parent[scenario.__name__]
    for n, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"call {n}: {a} != {b}"
    assert len(got["calls"]) == len(want["calls"]) and got["observed"] == want["observed"]


def test_what_the_recorded_scenarios_show(parent):
    """The parent traces say what the scenarios were written to show (so an empty or wrong recording cannot pass for agreement)."""
    up = {n: [c[0] for c in _calls(parent[n], name="upload_series")] for n in parent}
    first_C = {n: [c[2][0] for c in _calls(parent[n], name="set_state")] for n in parent}
    assert up["two_epochs_same_series"] == [0] and first_C["two_epochs_same_series"] == [{"shape": [D, R]}, None]
    assert up["series_changed_in_place"] == [0, 0]
    t = parent["mask_on_off_on"]["calls"]
    closes = [n for n, c in enumerate(t) if c[1] == "close"]
    assert [t[n][0] for n in closes] == [0, 1] and all(t[n - 1][1:] == ["get_state", [], {"want_C": True}] for n in closes)
    assert [c[3]["masked"] for c in _calls(parent["mask_on_off_on"], name="__init__") if "masked" in c[3]] == [_capi.MASKED_DYNAMICS] * 2
    assert len(_calls(parent["mask_as_dict_then_array"], name="upload_mask")) == 1
    assert len(_calls(parent["nonuniform_diagonal_R"], name="set_row_noise")) == 1
    assert len(_calls(parent["dense_R"], name="set_noise_rotation")) == 1 and _calls(parent["dense_R"], name="__init__")[0][3]["engine"] == "step"
    assert len(_calls(parent["scalar_schedules"], name="set_schedules")) == 1
    assert len(_calls(parent["q_matrix_schedule_on_device"], name="set_q_matrix_schedule")) == 1
    assert _calls(parent["q_matrix_schedule_on_device"], name="__init__")[0][3]["engine"] == "step"
    host = parent["q_matrix_schedule_host_stepped"]
    assert _calls(host, name="__init__")[0][3]["dyn_kind"] == _capi.DYN_HOST and len(_calls(host, name="step_host")) == 2 * T
    ring = parent["step_stream_step"]
    assert [c[0] for c in _calls(ring, name="series_ring")] == [1] and len(_calls(ring, name="__init__")) == 3 and ring["observed"]["streamed"] == T + 2
    for n in ("recursive_adam", "robust_recursive_adam"):
        names = [c[1] for c in _calls(parent[n], handle=0)]
        assert names.index("set_adam") < names.index("run")
    for n in ("recursive_custom_learning_rate", "robust_recursive_custom_learning_rate", "unrecognised_callable"):
        assert _calls(parent[n], name="__init__")[0][3]["dyn_kind"] == _capi.DYN_HOST and not _calls(parent[n], name="run")
    assert all(c[3]["lambda0"] == 2.5 for c in _calls(parent["robust_iter_fixed_lambda"], name="set_state"))
    assert parent["robust_iter_fixed_lambda"]["observed"]["lambda_default"] == 2.5
    assert parent["robust_iter_growing_lambda"]["observed"]["lambda"] == {str(T): 2.5 + D}
    assert parent["tracking_resident_series"]["observed"]["on_device"] == 1 and _calls(parent["tracking_resident_series"], name="sq_error")
    assert parent["tracking_other_series"]["observed"]["on_device"] == 0 and not _calls(parent["tracking_other_series"], name="sq_error")


def test_handle_replaced_for_a_q_matrix_schedule_keeps_C(monkeypatch):
    """Q[k] constant up to T1 = 4 and 0.05 I + 0.01 A A^T beyond; step(y, 1, 4), optim_update(1), step(y, 2, 7).  The second epoch needs
    another kind of handle (a Q-matrix schedule).  Before the session object the classes closed handle 0 WITHOUT fetching the device-resident
    C first -- its trace read [..., get_state(want_C=False), close] -- and handed handle 1 set_state(C=None, ...): the native library then
    has no state to run from (psmf_set_state leaves it unset without a C) and refuses the run.  With the one teardown path C is fetched
    before the close and handle 1 gets it as a (d, r) array."""
    T1, T2 = 4, 7

    def scenario(mp):
        f = _make(Qs=_q_matrices(T2, const_to=T1), nl=psmf.RandomWalk())
        f.optim_init()
        f.step(_series()[1], 1, T1)
        f.optim_update(1)
        f.step(_series()[1], 2, T2)
        return dict(C_shape=list(f._C[T2].shape))

    t = trace_of(scenario, monkeypatch)
    calls = t["calls"]
    close = [n for n, c in enumerate(calls) if c[1] == "close"]
    assert len(close) == 1 and calls[close[0]][0] == 0
    assert calls[close[0] - 1] == [0, "get_state", [], {"want_C": True}]
    new = _calls(t, handle=1)
    assert new[0][1] == "__init__" and new[0][3]["engine"] == "step"
    assert _calls(t, handle=1, name="set_state")[0][2][0] == {"shape": [D, R]}
    assert len(_calls(t, handle=1, name="set_q_matrix_schedule")) == 1 and _calls(t, handle=1, name="run")[0][2] == [0, T2]
    assert [c[0] for c in _calls(t, name="get_state") if c[3]["want_C"]] == [0, 1] and t["observed"]["C_shape"] == [D, R]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_device_session_cpu.py --record   (writes tests/golden/session_call_trace_parent.json)")
    out = {}
    for sc in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            out[sc.__name__] = trace_of(sc, mp)
    with open(GOLDEN, "w") as fp:
        json.dump(out, fp, separators=(",", ":"), sort_keys=True)
        fp.write("\n")
    print(f"{len(out)} scenarios, {sum(len(v['calls']) for v in out.values())} calls -> {GOLDEN}")
