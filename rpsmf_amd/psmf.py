"""PSMF filter classes with the call surface of pypsmf (`PSMFIter`, `PSMFRecursive`).

Same constructor, `run / step / inner / predict / optim_* / adam_* / sgd_*` methods, the same
overridable hook names and the same state attributes (`_C, _V, _mu, _P, _theta, _y_pred, _Q, _R,
_gradsum`, `C0, theta0, V0, _d, _r`) as pypsmf/psmf/psmf.py, so experiment subclasses written
against the reference (and its TrackingMixin) run unchanged.  Two execution back ends:

backend="hip"    (default) the whole `for k in 1..T: inner(...)` loop runs on the MI355X through
                 libpsmf_hip.so (include/psmf_hip.h).  Only *recognised* hook configurations can
                 be fused: the class attribute `hip_mode` names one ("full" = the hooks as
                 shipped; "simplified" = the ExperimentSynthetic overrides: P_bar = P_{k-1},
                 eta = tr(R)/d, no coefficient update).  A subclass that overrides compute hooks
                 must declare its `hip_mode`; otherwise the constructor raises.  There is no
                 silent CPU fallback: if the library or the GPU is missing, it raises.
backend="numpy"  the hooks below are executed one by one on the host, exactly as the
                 reference does, but in O(d r^2): no d x d matrix is ever formed (diagonal R,
                 Woodbury in r x r form, S^-1 as an implicit operator).  This is the plumbing
                 path for arbitrary hook overrides and arbitrary `nonlinearity` callables.

Deviations from the reference, all deliberate: `Rs[k]` / `Qs[k]` may be scalars or (d,) vectors
in addition to dense matrices (dense d x d is unusable at d >= 10^4); derivatives of the
nonlinearity are analytic / complex-step instead of autograd.
"""

from functools import cached_property

import numpy as np

from . import _capi, _noise
from ._noise import diag_of as _diag_of
from ._session import DeviceSession, _content_hash, _Lazy, _StateDict  # noqa: F401  (names other modules import from here)
from .learning_rate import BaseLearningRate, ConstantLearningRate
from .linop import InverseInnovation
from .nonlinearities import BaseNonLinearity, wrap_nonlinearity

__all__ = ["PSMFIter", "PSMFIterMissing", "PSMFRecursive"]

COMPUTE_HOOKS = (
    "_predictive_mean", "_predictive_covariance", "_predict_measurement", "_compute_eta_k",
    "_compute_dictionary_innovation", "_update_dictionary_mean", "_update_dictionary_covariance",
    "_compute_inverse_coefficient_innovation", "_update_coefficient_mean",
    "_update_coefficient_covariance", "_store_gradient",
)

HIP_MODES = {
    # name: (coef_update, eta_full, pbar_predict)
    "full": (True, True, True),
    "simplified": (False, False, False),
}
# compute hooks a class may override under each declared mode (the overrides ARE the mode: synthetic_psmf.py:82-98,
# synthetic_rpsmf.py:86-114); anything else would be skipped silently by the fused device loop
HIP_MODE_HOOKS = {
    "full": frozenset(),
    "simplified": frozenset({"_predictive_covariance", "_compute_eta_k", "_compute_inverse_coefficient_innovation",
                             "_update_coefficient_mean", "_update_coefficient_covariance"}),
}
# drive-level methods the fused loop replaces as a whole
FUSED_METHODS = ("inner", "_store_gradient", "_set_gradient", "_reset_gradient", "_carry_theta")


class _MuHist(_StateDict):
    """`_mu[k]` -> (r, 1) for k = 0..T after a device epoch: served from the device's mean history
    (the reference only keeps them when the experiment's `_prune` override spares `_mu`)."""

    def __init__(self, owner, T, last):
        super().__init__({T: last})
        self._owner, self._T, self._host = owner, T, None

    def __missing__(self, k):
        if 0 <= k <= self._T:
            if self._host is None:
                self._host = self._owner._dev.mu_history(0, self._T + 1)
            return self._host[k].reshape(-1, 1)
        raise KeyError(k)

    def __contains__(self, k):
        return 0 <= k <= self._T


class _YPred(dict):
    """`_y_pred[k]` -> (d, 1).  Steps 1..T are served from the device buffer (fetched once, whole)."""

    def __init__(self, owner=None, T=0):
        super().__init__()
        self._owner, self._T, self._host = owner, T, None

    def _block(self):
        if self._host is None:
            self._host = self._owner._dev.y_pred(0, self._T)
        return self._host

    def __missing__(self, k):
        if self._owner is not None and 1 <= k <= self._T:
            return self._block()[k - 1].reshape(-1, 1)
        raise KeyError(k)

    def __contains__(self, k):
        return dict.__contains__(self, k) or (self._owner is not None and 1 <= k <= self._T)


def _recognise_default():
    import os

    return os.environ.get("PSMF_RECOGNISE", "1").strip().lower() not in ("0", "false", "off", "no")


class PSMFIter:
    """Iterative (epochs over a fixed series) PSMF.  See the module docstring."""

    hip_mode = "full"
    robust = False

    def __init__(self, theta0, C0, V0, mu0, P0, Qs, Rs, nonlinearity, optim="adam", backend="hip",
                 device=0, storage="auto", gram_refresh=0, engine="auto", recognise=None):
        assert optim in ["adam", "sgd"]
        if backend not in ("hip", "numpy"):
            raise ValueError("backend must be 'hip' or 'numpy'")
        self.optim = optim
        self.backend = backend
        self.theta0 = theta0
        self.C0 = C0
        self.V0 = V0
        self.mu0 = mu0
        self.P0 = P0
        self._d, self._r = C0.shape
        self.nonlinearity = nonlinearity
        # `recognise` (default: on, unless the environment says PSMF_RECOGNISE=0): may the constructor work out by PROBING what
        # an undeclared hook override / a plain-function nonlinearity computes (modes.py)?  False = the strict behaviour:
        # undeclared overrides raise TypeError, plain functions are host-stepped (correct for any callable).
        self.recognise = _recognise_default() if recognise is None else bool(recognise)
        # (backend "hip": a plain function that IS one of the closed-form families runs inside the device loop, modes.py)
        self._nl = wrap_nonlinearity(nonlinearity, np.asarray(theta0).size,
                                     rank=self._r if (backend == "hip" and self.recognise) else None)
        self._C = _StateDict()
        self._P = _StateDict()
        self._V = _StateDict()
        self._mu = _StateDict()
        self._Q = Qs
        self._R = Rs
        self._theta = {0: theta0}
        self._y_pred = {}
        self._gradsum = np.zeros(np.asarray(theta0).shape)
        self._dev_opts = dict(device=device, storage=storage, gram_refresh=gram_refresh, engine=engine)
        self._session = DeviceSession(self)      # (created here, so that a probe object of modes.py has its own; no handle yet)
        if backend == "hip":
            self._check_hip_configuration()

    # ------------------------------------------------------------------ drive methods
    def run(self, y, T, n_iter, n_pred, mask=None):
        self.optim_init()
        for i in range(1, n_iter + 1):
            self.step(y, i, T, **({} if mask is None else dict(mask=mask)))      # (a step() written against the reference takes no mask)
            self.predict(i, T, n_pred)
            self.optim_update(i)

    def step_reset(self):
        """Epoch start: carry the last C, mu, P, V (or the initial values); zero the gradient."""
        def latest(D, init):
            if not D:
                return init
            k = max(D.keys())
            return D.raw(k) if isinstance(D, _StateDict) else D[k]

        self._C = _StateDict({0: latest(self._C, self.C0)})
        self._mu = _StateDict({0: latest(self._mu, self.mu0)})
        self._P = _StateDict({0: latest(self._P, self.P0)})
        self._V = _StateDict({0: latest(self._V, self.V0)})
        self._gradsum = np.zeros(np.asarray(self.theta0).shape)

    def step(self, y, i, T, mask=None):
        """One epoch over y[1..T].  `mask` (device back end): the observed entries of every step, {k: (d, 1) or (d,)} like y or an
        array indexed the same way (row 0 unused), nonzero = observed -- the masked filter of ExperimentImpute (e = m o (y - y_hat),
        eta and lambda with d, y_hat stored unmasked) with this class's f_theta, and theta learned from the gradient of the masked
        incremental likelihood (psmf.py:264-270).  None: every entry observed, nothing changes."""
        if mask is not None and self.backend != "hip":
            raise NotImplementedError('mask=: backend="numpy" executes the reference\'s hooks, which know no missing entries; use backend="hip"')
        if self.backend == "hip":
            self._device_epoch(i, T, y, mask)
            return
        self.step_reset()
        for k in range(1, T + 1):
            self.inner(i, k, np.asarray(y[k]).reshape(-1, 1))     # y[k], k = 1..T: dict or array-like (row 0 unused)

    def inner(self, i, k, yk):
        self._filter_step(i, k, yk)
        self._prune(k)

    def _filter_step(self, i, k, yk):
        """The hook sequence of one step, in the reference's order (psmf.py:90-101; the recursive inner(), psmf.py:288-298, calls it with i = k)."""
        mu_bar = self._predictive_mean(i, k)
        P_bar = self._predictive_covariance(i, k)
        self._y_pred[k] = self._predict_measurement(k, mu_bar)
        eta_k = self._compute_eta_k(k, P_bar)
        Nk = self._compute_dictionary_innovation(k, eta_k, mu_bar, P_bar)
        self._update_dictionary_mean(k, yk, Nk, mu_bar)
        self._update_dictionary_covariance(k, Nk, mu_bar, yk)
        Skinv = self._compute_inverse_coefficient_innovation(k, mu_bar, P_bar)
        self._update_coefficient_mean(k, yk, Skinv, mu_bar, P_bar)
        self._update_coefficient_covariance(k, Skinv, P_bar, yk)
        self._store_gradient(i, k, yk, eta_k)

    # ------------------------------------------------------------------ hooks (numpy backend)
    def _q_at(self, k):
        return self._Q[k]

    def _r_index(self, k):
        return k

    def _rho_at(self, k):
        """diag(R_k) as (d,) vector; raises for a non-diagonal R (use the dense route)."""
        dg = _diag_of(self._R[self._r_index(k)], self._d)
        if dg is None:
            return None
        return np.full(self._d, dg) if np.ndim(dg) == 0 else dg

    def _predictive_mean(self, i, k):
        return self._nl(self._theta[i - 1], self._mu[k - 1], k)

    def _predictive_covariance(self, i, k):
        F = self._nl.jac_x(self._theta[i - 1], self._mu[k - 1], k)
        return F @ self._P[k - 1] @ F.T + self._q_at(k)

    def _predict_measurement(self, k, mu_bar):
        return self._C[k - 1] @ mu_bar

    def _compute_eta_k(self, k, P_bar):
        C = self._C[k - 1]
        rho = self._rho_at(k)
        tr_R = np.trace(self._R[self._r_index(k)]) if rho is None else rho.sum()
        return (tr_R + np.sum((C.T @ C) * P_bar)) / self._d

    def _compute_dictionary_innovation(self, k, eta_k, mu_bar, P_bar):
        return mu_bar.T @ self._V[k - 1] @ mu_bar + eta_k

    def _update_dictionary_mean(self, k, yk, Nk, mu_bar):
        w = self._V[k - 1] @ mu_bar
        self._C[k] = self._C[k - 1] + (yk - self._y_pred[k]) @ w.T / Nk

    def _update_dictionary_covariance(self, k, Nk, mu_bar, yk):
        w = self._V[k - 1] @ mu_bar
        self._V[k] = self._V[k - 1] - (w @ w.T) / Nk

    def _compute_inverse_coefficient_innovation(self, k, mu_bar, P_bar):
        C = self._C[k - 1]
        s = float(np.squeeze(mu_bar.T @ self._V[k - 1] @ mu_bar))
        rho = self._rho_at(k)
        if rho is not None and (rho + s).sum() > 0:
            w = 1.0 / (rho + s)
            U = w[:, None] * C
            K = np.linalg.inv(np.linalg.inv(P_bar) + C.T @ U)
            return InverseInnovation(w, U, K)
        Rbar = np.asarray(self._R[self._r_index(k)], dtype=float) + s * np.eye(self._d)
        return np.linalg.inv(C @ P_bar @ C.T + Rbar)

    def _update_coefficient_mean(self, k, yk, Skinv, mu_bar, P_bar):
        self._mu[k] = mu_bar + P_bar @ (self._C[k - 1].T @ (Skinv @ (yk - self._y_pred[k])))

    def _update_coefficient_covariance(self, k, Skinv, P_bar, yk):
        C = self._C[k - 1]
        self._P[k] = P_bar - P_bar @ (C.T @ (Skinv @ C)) @ P_bar

    def _grad_f(self, k, yk, eta_k, mu_prev, theta):
        """d(incremental likelihood)/d f at the pre-update state (closed form of psmf.py:57-64)."""
        f = self._nl(theta, mu_prev, k)
        C, V = self._C[k - 1], self._V[k - 1]
        u = V @ f
        N = float(np.squeeze(f.T @ u)) + float(np.squeeze(eta_k))
        e = yk - C @ f
        ee = float(np.squeeze(e.T @ e))
        return self._d * u / N - (C.T @ e) / N - ee * u / N**2

    def _store_gradient(self, i, k, yk, eta_k):
        theta = self._theta[i - 1]
        if np.asarray(theta).size == 0:
            return
        Jt = self._nl.jac_theta(theta, self._mu[k - 1], k)
        g = Jt.T @ self._grad_f(k, yk, eta_k, self._mu[k - 1], theta)
        self._gradsum = self._gradsum + g.reshape(self._gradsum.shape)

    def _prune(self, k):
        del self._C[k - 1], self._V[k - 1], self._mu[k - 1], self._P[k - 1]

    def predict(self, i, T, n_pred):
        if self.backend == "hip" and self._dev is not None and isinstance(self._y_pred, _YPred):
            return self._predict_hip(i, T, n_pred)
        self._mu_pred = {T: self._mu[T]}
        for k in range(T + 1, T + n_pred + 1):
            self._mu_pred[k] = self._nl(self._theta[i - 1], self._mu_pred[k - 1], k)
            self._y_pred[k] = self._C[T] @ self._mu_pred[k]

    # ------------------------------------------------------------------ optimiser (host, p-sized)
    def adam_init(self, gam=1e-3, b1=0.9, b2=0.999):
        self.adam_gam = gam if isinstance(gam, BaseLearningRate) else ConstantLearningRate(gam)
        self.adam_b1, self.adam_b2 = b1, b2
        shape = np.asarray(self.theta0).shape
        self.adam_m, self.adam_v = np.zeros(shape), np.zeros(shape)
        self.adam_m_hat, self.adam_v_hat = np.zeros(shape), np.zeros(shape)

    def sgd_init(self, gam=1e-3):
        self.sgd_gam = gam if isinstance(gam, BaseLearningRate) else ConstantLearningRate(gam)

    def optim_init(self, gam=1e-3):
        if self.optim == "adam":
            self.adam_init(gam=gam)
        else:
            self.sgd_init(gam=gam)

    def optim_update(self, i, project=True):
        if self.optim == "adam":
            return self.adam_update(i, project=project)
        return self.sgd_update(i, project=project)

    def adam_update(self, i, project=True):
        g = self._gradsum
        self.adam_m = self.adam_b1 * self.adam_m + (1 - self.adam_b1) * g
        self.adam_v = self.adam_b2 * self.adam_v + (1 - self.adam_b2) * g * g
        self.adam_m_hat = self.adam_m / (1 - self.adam_b1**i)
        self.adam_v_hat = self.adam_v / (1 - self.adam_b2**i)
        step = self.adam_gam.get(i) * self.adam_m_hat / (np.sqrt(self.adam_v_hat) + 1e-8)
        self._theta[i] = self._theta[i - 1] - step
        if project:
            self._theta[i] = np.maximum(self._theta[i], 0)

    def sgd_update(self, i, project=True):
        self._theta[i] = self._theta[i - 1] - self.sgd_gam.get(i) * self._gradsum
        if project:
            self._theta[i] = np.maximum(self._theta[i], 0)

    # ------------------------------------------------------------------ device back end
    def _overridden_hooks(self):
        base = rPSMF_BASE if self.robust else PSMFIter
        return [h for h in COMPUTE_HOOKS if getattr(type(self), h) is not getattr(base, h)]

    def _overrides(self, name):
        """True if the class replaces `name` of the library class it derives from (PSMFIter / PSMFRecursive / rPSMF*)."""
        mine = getattr(type(self), name, None)
        for base in type(self).__mro__:
            if base in _BASE_CLASSES and base is not object and name in vars(base):
                return mine is not vars(base)[name]
        return False

    def _check_hip_configuration(self):
        over = self._overridden_hooks()
        declared = any("hip_mode" in vars(c) for c in type(self).__mro__ if c not in _BASE_CLASSES)
        recognised = False
        if over and not declared:
            # an experiment subclass written against the reference (synthetic_psmf.py:78-100): find out WHAT its hooks compute
            # by running them on small probe problems next to the library's statement of every device mode (modes.py)
            from .modes import HookRecognitionWarning, recognise_hip_mode

            if not self.recognise:
                raise TypeError(
                    f"{type(self).__name__} overrides {over} without declaring hip_mode, and recognition by probing is switched "
                    "off (recognise=False / PSMF_RECOGNISE=0).  Declare the class attribute hip_mode, or use backend='numpy'.")
            mode = recognise_hip_mode(self)
            if mode is not None:
                import warnings

                warnings.warn(
                    f"{type(self).__name__}: the overridden hooks {over} were matched to the device mode {mode!r} by running them on "
                    "probe problems (several sizes, step indices up to 10^5); the fused device loop executes that mode, NOT the "
                    "Python hooks.  A hook whose behaviour depends on something the probes do not vary is not detected: declare "
                    "`hip_mode` on the class to state the intent, or pass recognise=False / backend='numpy'.",
                    HookRecognitionWarning, stacklevel=4)
            if mode is None:
                raise TypeError(
                    f"{type(self).__name__} overrides {over}: the device back end can only fuse recognised hook "
                    f"configurations, and on a probe problem these hooks match none of {sorted(HIP_MODES)}.  Declare the class "
                    "attribute hip_mode if they are meant to, or construct with backend='numpy' (which executes the hooks).")
            self.hip_mode = mode
            recognised = True
        self.hip_mode_recognised = recognised
        if self.hip_mode not in HIP_MODES:
            raise ValueError(f"unknown hip_mode {self.hip_mode!r}")
        extra = [] if recognised else sorted(set(over) - HIP_MODE_HOOKS[self.hip_mode])
        if extra:
            raise TypeError(
                f"{type(self).__name__} declares hip_mode={self.hip_mode!r} but also overrides {extra}, which that mode "
                "does not cover: the fused device loop would skip them.  Use backend='numpy'.")
        lost = [m for m in FUSED_METHODS if m not in COMPUTE_HOOKS and self._overrides(m)]
        if lost:
            raise TypeError(
                f"{type(self).__name__} overrides {lost}: with backend='hip' the whole time loop runs on the device and "
                "these methods are never called.  Use backend='numpy'.")
        if self._r > _capi.RMAX:
            raise ValueError(f"r = {self._r} > {_capi.RMAX}")

    _dev = property(lambda self: self._session.dev, doc="The DeviceFilter this object runs on; None before the first device epoch.")

    # what R and Q are to the device: _noise.py; the structure of R is worked out once per object
    def _first_R(self):
        R = self._R
        return R[1 if 1 in R else min(R.keys())] if isinstance(R, dict) else R

    @cached_property
    def _R_structure(self):
        """(dense, rows): (lam, U) of a NON-DIAGONAL R = U diag(lam) U^T or None, and what _row_noise() returns (_noise.structure_of)."""
        return _noise.structure_of(self._first_R(), self._d)

    def _row_noise(self):
        """diag(R) as a (d,) vector when R is a NON-uniform diagonal (or its eigenvalues when it is dense), else None."""
        return self._R_structure[1]

    def _rho_of(self, Rk):
        return _noise.rho_of(Rk, self._d, self._first_R(), *self._R_structure)

    def _device_rho_q(self, T=None):
        """(rho, Q, rho_sched, q_sched) for the device: PSMFIter reads R[k], Q[k] of step k (psmf.py:115,123,141), the simplified
        hooks R[k - 1] (synthetic_psmf.py:86-87); q_sched = "host": a Q[k] that is not a multiple of Q[1] (_noise.rho_q_schedules)."""
        return _noise.rho_q_schedules(self._R, self._Q, T, self._r, 1 if self.hip_mode == "simplified" else 0, self._rho_of)

    # a Q[k] schedule of matrices (not multiples of Q[1]) goes to the device as [T + 1, r, r] up to this size, else host-stepped
    _Q_MATRIX_SCHEDULE_MAX_BYTES = 1 << 31

    def _q_matrices(self, T):
        return _noise.q_matrices(self._Q, T, self._r)

    def _host_stepped(self):
        """True when f is evaluated on the host, one device step at a time (psmf_step_host): arbitrary callables and what
        psmf_dyn.hip does not hold (a Fourier basis of more than 4 + 4 terms), or a Q[k] schedule of matrices too large to
        upload.  The recognised kinds run inside the device time loop on either engine (scaled walk / sinusoid / Fourier at
        r > 32 or with a non-uniform R: the per-step engine's serial stage).  The recursive classes: also when the in-loop optimiser
        is not one the device implements."""
        return (self._nl.device_kind is None or self._session.kind.host_forced
                or (self._in_loop_optimiser and np.asarray(self.theta0).size > 0 and _device_optimiser(self) is None))

    def _device_kwargs(self):
        coef, eta_full, pbar = HIP_MODES[self.hip_mode]
        kind = self._session.kind
        kw = dict(robust=self.robust, coef_update=coef, eta_full=eta_full, pbar_predict=pbar, **self._dev_opts)
        if self._host_stepped():
            kw.update(dyn_kind=_capi.DYN_HOST, engine="step")
        else:
            kw.update(dyn_kind=self._nl.device_kind, dyn_flags=self._nl.device_flags, dyn_terms=self._nl.device_terms)
        if self._row_noise() is not None or kind.q_matrices:
            kw.update(engine="step")
        if self._row_noise() is not None:
            kw.update(nonuniform_R=True)
        if kind.masked:
            kw.update(masked=_capi.MASKED_DYNAMICS, engine="step")
        if self._in_loop_optimiser and kw["dyn_kind"] != _capi.DYN_HOST:
            # the in-loop optimiser's configuration (psmf.py:224-248,299-304): recursive = 1 Adam, 2 SGD.  (Host-stepped: theta and
            # its optimiser, any schedule, stay on the host.)
            kw.update(update_every=self._update_every, adam_b1=getattr(self, "adam_b1", 0.9),
                      adam_b2=getattr(self, "adam_b2", 0.999), **_device_optimiser(self))
        return kw

    def _open_device(self, ring):
        """A new handle of the session's kind (DeviceSession.ensure): resident series buffers, or a series ring of `ring` = (chunk, n_slots)."""
        dev = _capi.DeviceFilter(self._d, self._r, **self._device_kwargs())
        dense, rows = self._R_structure
        if dense is not None:
            dev.set_noise_rotation(dense[1], dense[0])
        elif rows is not None:
            dev.set_row_noise(rows)
        if ring is not None:
            dev.series_ring(*ring)
        return dev

    def _select_device(self, mask, T, ring=None):
        """The handle this epoch runs on.  A masked epoch runs on a masked handle (cfg.masked = PSMF_MASKED_DYNAMICS, per-step engine), an
        unmasked one on the handle it always had; a stream on a handle with a series ring; a Q[k] of matrices on yet another kind.  Going
        from one to the other replaces the handle (DeviceSession.ensure).  What a masked handle cannot run is refused here, by name."""
        kind = self._session.kind._replace(masked=mask is not None, ring=ring)
        if mask is not None:
            if self._host_stepped():
                raise NotImplementedError("mask=: host-stepped callables (a nonlinearity or learning-rate schedule evaluated on the host) "
                                          "would need the masked gradient g_f on the host; use one of the built-in nonlinearities")
            if HIP_MODES[self.hip_mode] != (True, True, True):
                raise NotImplementedError(f"mask=: the masked filter is the full filter; hip_mode {self.hip_mode!r} is not")
            _rho, _Q, rho_s, q_s = self._device_rho_q(T)
            if rho_s is not None or q_s is not None or kind.q_matrices:
                raise NotImplementedError("mask=: R / Q schedules that vary with k are not run on masked handles (a constant R = rho I or "
                                          "diagonal R, a constant Q)")
            if self._R_structure[0] is not None:
                raise NotImplementedError("mask=: a dense (non-diagonal) R is run in its eigenbasis, where a mask over the rows means nothing")
            if self._row_noise() is not None and np.asarray(self.theta0).size > 0:
                raise NotImplementedError("mask=: a non-uniform diagonal R with learned theta (the device then carries sum m_i rho_i in "
                                          "place of the observed count the masked gradient needs); use R = rho I")
        if (ring is None and not self._in_loop_optimiser and not self._host_stepped() and not self.robust and not kind.q_matrices
                and isinstance(self._device_rho_q(T)[3], str)):
            # Q[k] is not a scalar multiple of Q[1]: uploaded matrix by matrix, P_bar = F P F^T + Q_k formed in the per-step
            # engine's serial stage (psmf_set_q_matrix_schedule) -- or, beyond _Q_MATRIX_SCHEDULE_MAX_BYTES, by the host, one
            # device step at a time.  Either way another kind of handle, from here on.
            fits = (T + 1) * self._r * self._r * 8 <= self._Q_MATRIX_SCHEDULE_MAX_BYTES
            kind = kind._replace(q_matrices=fits, host_forced=not fits)
        return self._session.ensure(kind)

    def _device_lambda0(self):
        return 0.0

    def _pull_state(self, T):
        s, C = self._session.pull_state()
        self._C, self._V, self._P = _StateDict({T: C}), _StateDict({T: s["V"]}), _StateDict({T: s["P"]})
        self._mu = _MuHist(self, T, s["mu"].reshape(-1, 1))
        if s["gradsum"].size == np.asarray(self.theta0).size and s["gradsum"].size:
            self._gradsum = s["gradsum"].reshape(np.asarray(self.theta0).shape)
        self._y_pred = _YPred(self, T)
        return s

    _in_loop_optimiser, _update_every = False, 1      # the recursive classes: theta takes an optimiser step inside the time loop, every so many steps

    def _device_epoch(self, i, T, y=None, mask=None, stream=None, keep_y_pred=False):
        """One epoch on the device, for step() of every class and step_stream(): epoch reset, the handle this epoch needs, series and
        state onto it, the fused time loop (or the host-stepped one), state back, the recognised nonlinearity re-checked.  Returns T.
        `y`, `mask`: the resident series, run(0, T).  `stream` = (chunks, chunk, n_slots) instead: through a series ring; `T` going in
        is then only how far the R / Q dictionaries reach, the T coming out what the stream held, and of `_mu` / `_y_pred` only the last
        mean and what keep_y_pred collects are kept.  The recursive classes start from theta_0 whatever `i` and take theta_T back."""
        rec = self._in_loop_optimiser
        self.step_reset()
        dev = self._select_device(mask, T, ring=None if stream is None else (int(stream[1]), int(stream[2])))
        if stream is None:
            self._session.upload_series(y, T, self._d)
            if mask is not None:
                self._session.upload_mask(mask, T, self._d)
        else:
            self._session.series_key = None
        if rec:
            self._theta, i = {0: self._theta[0]}, 1
        theta, mu0 = self._theta[i - 1], np.asarray(self._mu[0], dtype=float).reshape(-1, 1)
        rho, Q, rho_s, q_s = self._device_rho_q(T)
        Qm = self._q_matrices(T) if (self._session.kind.q_matrices and not self._host_stepped()) else None
        self._session.push_state(self._C.raw(0), self._V[0], self._P[0], Q, mu0.reshape(-1), rho, self._device_lambda0(),
                                 np.asarray(theta, dtype=float).reshape(-1), rho_s, q_s, Qm)
        if self._host_stepped():
            self._after_device_epoch(self._run_host_stepped(i, T, recursive=rec), T)
            return T
        dev.zero_gradsum()
        if rec and self.optim == "adam":
            dev.set_adam(self.adam_m.reshape(-1), self.adam_v.reshape(-1))
        if stream is None:
            dev.run(0, T)
        else:
            kept, T = {}, 0
            for kb, ke, yp in dev.run_stream(stream[0]):
                T = ke
                if keep_y_pred and yp is not None:
                    kept.update((k + 1, yp[k - kb].reshape(-1, 1)) for k in range(kb, ke))
        s = self._pull_state(T)
        if stream is not None:
            self._mu, self._y_pred = _StateDict({T: s["mu"].reshape(-1, 1)}), kept
        if rec:
            self._theta[T] = s["theta"].reshape(np.asarray(self.theta0).shape)
        self._after_device_epoch(s, T)
        # theta moves inside the recursive loop: only step 1 has a known theta; a stream keeps no mean history: step 1, from the mean it began with
        self._verify_recognised_nonlinearity(theta, T, ks=[1] if (rec or stream is not None) else None, mu0=None if stream is None else mu0)
        return T

    def step_stream(self, chunks, chunk, n_slots=2, i=1, keep_y_pred=False):
        """One pass over a stream that need not fit on the device, nor have a known length: `chunks` is an iterable of
        (nt, d) time-major arrays of `chunk` observations each (the last may be shorter), y_1 first.  What step() does -- epoch
        reset, state onto the device, the fused time loop, state back -- with the series going through a ring of n_slots chunks
        (DeviceFilter.run_stream): chunk j + 1 is uploaded while chunk j is filtered.  The recursive classes keep their in-loop
        optimiser (and take no epoch index).  `_y_pred` and the mean history are not kept beyond the last step unless
        keep_y_pred=True collects the predictions on the host.  Returns T, the number of observations filtered."""
        if self.backend != "hip":
            raise NotImplementedError('step_stream: backend="numpy" steps through a dict of observations; use step()')
        if self._host_stepped():
            raise NotImplementedError("step_stream: host-stepped callables (a nonlinearity or learning-rate schedule evaluated on "
                                      "the host, one device step at a time) are not streamed; use step()")
        if self._R_structure[0] is not None:
            raise NotImplementedError("step_stream: a non-diagonal R keeps the series rotated on the device; use step()")
        t_max = max([k for D in (self._R, self._Q) if isinstance(D, dict) for k in D] + [0])
        _rho, _Q, rho_s, q_s = self._device_rho_q(t_max)
        if rho_s is not None or q_s is not None or self._session.kind.q_matrices:
            raise NotImplementedError("step_stream: R / Q schedules that vary with k are indexed by step and not windowed; use step()")
        return self._device_epoch(i, t_max, stream=(chunks, chunk, n_slots), keep_y_pred=keep_y_pred)

    def _q_for_step(self, k, Q_running):
        """Q entering P_bar of step k: PSMFIter reads Q[k] (psmf.py:115); rPSMFIter its running Q_{k-1} (rpsmf.py:123)."""
        if self.robust:
            return Q_running
        Q = self._Q[k] if isinstance(self._Q, dict) else self._Q
        return _noise.q_matrix(Q, self._r)

    def _run_host_stepped(self, i, T, recursive=False):
        """The time loop with f on the host: per step the host evaluates mu_bar = f(theta, mu, k), F = df/dx and
        P_bar = F P F^T + Q_k (r-sized, psmf.py:104-115), the device does everything d-sized of inner() (psmf_step_host),
        and the theta gradient is accumulated as J_theta^T g_f from the g_f the device returns (psmf.py:167-177)."""
        dev, nl, r = self._dev, self._nl, self._r
        pbar_predict = HIP_MODES[self.hip_mode][2]
        theta = self._theta[i - 1]           # (the recursive classes: i = 1)
        n_th = np.asarray(theta).size
        mu = np.asarray(self._mu[0], dtype=float).reshape(-1, 1)
        P = np.asarray(self._P[0], dtype=float)
        Qrun = _noise.q_matrix(self.Q0, self._r) if self.robust else None
        grad = np.zeros(np.asarray(self.theta0).shape)
        for k in range(1, T + 1):
            mu_bar = np.asarray(nl(theta, mu, k), dtype=float).reshape(-1)
            if pbar_predict:
                F = nl.jac_x(theta, mu, k)
                P_bar = F @ P @ F.T + self._q_for_step(k, Qrun)
            else:
                P_bar = P
            mu_new, gf, P, Qrun_dev = dev.step_host(k - 1, mu_bar, 0.5 * (P_bar + P_bar.T))
            if self.robust:
                Qrun = Qrun_dev
            if n_th:
                Jt = nl.jac_theta(theta, mu, k)
                grad = grad + (Jt.T @ gf).reshape(grad.shape)
            mu = mu_new.reshape(-1, 1)
            if recursive:
                self._gradsum = grad
                if k % self._update_every == 0:
                    self.optim_update(k)
                    grad = np.zeros_like(grad)
                else:
                    self._carry_theta(k)
                theta = self._theta[k]
        s = self._pull_state(T)
        self._gradsum = grad
        s["gradsum"] = np.zeros(0)
        s["theta"] = np.asarray(theta, dtype=float).reshape(-1)
        return s

    def _after_device_epoch(self, s, T):
        pass

    def _verify_recognised_nonlinearity(self, theta, T, ks=None, mu0=None):
        """A plain callable that the constructor matched to a closed-form family (modes.recognise_nonlinearity) ran inside
        the device loop as that family.  Re-check the match where it matters: at (theta, mu_{k-1}, k) for step indices spread
        over the epoch just filtered (the mean history is on the device; `mu0`: a stream, which kept none: step 1 only).  A mismatch
        means the epoch was filtered with the wrong f: raise, naming the way out."""
        fn = getattr(self._nl, "recognised_from", None)
        if fn is None or T < 1:
            return
        from .modes import nonlinearity_mismatch

        if ks is None:
            ks = sorted({1, 2, T, *np.linspace(1, T, num=min(T, 24), dtype=int).tolist()})
        for k in ks:
            if nonlinearity_mismatch(fn, self._nl, theta, self._mu[k - 1] if mu0 is None else mu0, k):
                raise RuntimeError(
                    f"the nonlinearity {getattr(fn, '__name__', fn)!r} was recognised as {type(self._nl).__name__} on probe inputs "
                    f"but differs from it at step {k} of this " + ("stream.  Construct with recognise=False." if mu0 is not None else
                    "run: the device evaluated the wrong function.  Construct with "
                    "recognise=False (or PSMF_RECOGNISE=0) so that the callable is host-stepped."))

    def _predict_hip(self, i, T, n_pred):
        if self._host_stepped():
            theta = self._theta[i - 1] if (i - 1) in self._theta else self._theta[max(self._theta)]
            mu, roll = self._mu[T], []
            for k in range(T + 1, T + n_pred + 1):      # psmf.py:183-187 on the host (r-sized), C mu_pred on the device
                mu = np.asarray(self._nl(theta, mu, k), dtype=float).reshape(-1, 1)
                roll.append(mu.reshape(-1))
            out = self._dev.project(np.array(roll)) if roll else np.zeros((0, self._d))
        else:
            out = self._dev.predict(T, n_pred)
        for q in range(n_pred):
            dict.__setitem__(self._y_pred, T + q + 1, out[q].reshape(-1, 1))

    def sq_errors(self, T):
        """sum_k ||y_hat_k - y_k||^2 over the filtered steps, reduced on the device
        (what TrackingMixin.errors_update computes from `_y_pred` on the host)."""
        return self._dev.sq_error(0, T)


def _device_optimiser(obj):
    """Keyword arguments of the in-loop optimiser the device implements -- Adam (psmf.py:224-242) or plain SGD (psmf.py:244-248),
    each with a constant or an exponentially decaying learning rate (learning_rate.py:13-27) -- or None: custom learning-rate
    schedules keep theta and its optimiser on the host (host-stepped device loop)."""
    if obj.optim not in ("adam", "sgd"):
        return None
    gam, kind = getattr(obj, obj.optim + "_gam", ConstantLearningRate(1e-3)), 1 if obj.optim == "adam" else 2
    if isinstance(gam, ConstantLearningRate):
        return dict(recursive=kind, adam_lr=gam.lr)
    if hasattr(gam, "lr_start") and hasattr(gam, "lr_end") and hasattr(gam, "steps"):
        return dict(recursive=kind, adam_lr=gam.lr_start, adam_lr_end=gam.lr_end, adam_lr_steps=gam.steps)
    return None


class PSMFIterMissing(PSMFIter):
    """Unfinished in the reference (pypsmf/psmf/psmf.py:251-254) and not constructible here either.  Missing observations with this
    library's dynamics: PSMFIter(...).step(y, i, T, mask=m) / .run(..., mask=m) (and the recursive classes' step / run), or
    rpsmf_amd.impute for the ExperimentImpute drivers."""

    def __init__(*args, **kwargs):
        # unfinished in the reference as well (pypsmf/psmf/psmf.py:251-254); the working masked
        # filter is rpsmf_amd.impute (ExperimentImpute semantics)
        raise NotImplementedError


class PSMFRecursive(PSMFIter):
    """Online variant: theta takes an optimiser step inside the time loop every `update_every`
    observations (pypsmf/psmf/psmf.py:275-331)."""

    # device: Adam and plain SGD run inside the time loop of either engine; custom learning-rate schedules: host-stepped
    _in_loop_optimiser = True

    def run(self, y, T, n_pred, update_every=1, mask=None):
        self._update_every = update_every
        self.optim_init()
        self.step(y, T, **({} if mask is None else dict(mask=mask)))
        self.predict(T, n_pred)

    def step(self, y, T, mask=None):
        if mask is not None and self.backend != "hip":
            raise NotImplementedError('mask=: backend="numpy" executes the reference\'s hooks, which know no missing entries; use backend="hip"')
        if self.backend == "hip":
            self._device_epoch(1, T, y, mask)
            return
        self.step_reset()
        for k in range(1, T + 1):
            self.inner(k, np.asarray(y[k]).reshape(-1, 1))

    def inner(self, k, yk):
        self._filter_step(k, k, yk)
        if k % self._update_every == 0:
            self.optim_update(k)
            self._reset_gradient()
        else:
            self._carry_theta(k)

    def _reset_gradient(self):
        self._gradsum = np.zeros(np.asarray(self.theta0).shape)

    def _carry_theta(self, i):
        self._theta[i] = self._theta[i - 1]

    def _set_gradient(self, k, yk, eta_k):
        self._reset_gradient()
        self._store_gradient(k, k, yk, eta_k)

    def predict(self, T, n_pred):
        return PSMFIter.predict(self, T + 1, T, n_pred)        # rolls forward with theta_T (psmf.py:324-331)


rPSMF_BASE = PSMFIter          # rebound by rpsmf.py once rPSMFIter exists
_BASE_CLASSES = [PSMFIter, PSMFRecursive, PSMFIterMissing, object]
