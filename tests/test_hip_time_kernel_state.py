"""psmf_time_kernel: "State is saved and restored around the measurement" (include/psmf_hip.h) -- bench.py calls it between
its measurements and then goes on using the handle.  The measurement launches a step's kernels at the FIRST steps of the series
whatever the handle has run so far, so besides C, the r x r state and theta it overwrites the y_hat rows and the posterior means
recorded for those steps; all of it must be back afterwards, bit for bit, and the rest of the run must land where an
uninterrupted handle lands.  GPU only: `pytest -m gpu`.

What the library does with psmf_counters across the calls is printed (`-s`), not asserted: the header promises nothing about
them.  Observed on an MI355X: they do not move -- the inversion counters, block and launch counts and in-kernel durations live in
the device state that the measurement saves and restores, so the stand-alone launches it makes leave no trace in them
(psmf_filter_kernel_time's HIP-event sums are host-side and only chained launches of psmf_run add to them).
Reference: the reference times whole runs with time.time() (ExperimentImpute/PSMF.py:59,91) and has no counterpart."""

import numpy as np
import pytest

from oracle import psmf_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

# (id, DeviceFilter keywords, d, r, T, kernel the handle must report, `which` values the engine accepts)
CONFIGS = [
    ("block_filter3_r32_f32", dict(engine="block", storage="f32"), 2048, 32, 100, "psmf_blk_filter3", (0, 1, 2)),
    ("block_filter6d_r12", dict(engine="block", storage="f64"), 777, 12, 110, "psmf_blk_filter6d", (0, 1, 2)),
    ("step_r20", dict(engine="step", storage="f64"), 1000, 20, 40, "psmf_pstep_k", (0, 1)),
]
KEYS = ("C", "V", "P", "Q", "mu", "theta", "gradsum", "rho", "lam", "s", "eta", "N", "phi", "omega", "k")


@pytest.mark.parametrize("name,kw,d,r,T,kernel,whiches", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_time_kernel_leaves_the_handle_as_it_found_it(name, kw, d, r, T, kernel, whiches):
    from rpsmf_amd import _capi as c

    Y = O.synthetic_series(d, r, T, 4100 + r, dtype=np.float64)
    C0 = 0.1 * np.random.default_rng(r).standard_normal((d, r))
    if kw["storage"] == "f32":
        Y, C0 = Y.astype(np.float32).astype(np.float64), C0.astype(np.float32).astype(np.float64)
    h = T // 2

    def start():
        f = c.DeviceFilter(d, r, **kw)
        f.upload_series(Y)
        f.set_state(C0, 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0, lambda0=1.8)
        assert f.geometry()["filter_kernel"] == kernel, f.geometry()
        f.run(0, h)
        return f

    f = g = None
    try:
        f, g = start(), start()
        snap, yp, mu = f.get_state(), f.y_pred(0, h), f.mu_history(0, h + 1)
        before = f.counters()
        for which in whiches:
            us = f.time_kernel(which, 3)
            assert np.isfinite(us) and us > 0.0, (which, us)
            now, yp_now, mu_now = f.get_state(), f.y_pred(0, h), f.mu_history(0, h + 1)
            changed = [k for k in KEYS if not np.array_equal(np.asarray(now[k]), np.asarray(snap[k]), equal_nan=True)]
            assert not changed, (name, which, "state changed", changed)
            assert np.array_equal(yp_now, yp), (name, which, "y_pred rows changed", np.flatnonzero(np.any(yp_now != yp, axis=1)))
            assert np.array_equal(mu_now, mu), (name, which, "posterior-mean rows changed", np.flatnonzero(np.any(mu_now != mu, axis=1)))
        after = f.counters()
        print(f"\n{name}: counters before the time_kernel calls {before}\n{name}: counters after {after}")
        f.run(h, T)
        g.run(h, T)
        end_f, end_g = f.get_state(), g.get_state()
        changed = [k for k in KEYS if not np.array_equal(np.asarray(end_f[k]), np.asarray(end_g[k]), equal_nan=True)]
        assert not changed, (name, "the run after the measurement differs from an uninterrupted handle's", changed)
        assert np.array_equal(f.y_pred(0, T), g.y_pred(0, T))
    finally:
        for x in (f, g):
            if x is not None:
                x.close()
