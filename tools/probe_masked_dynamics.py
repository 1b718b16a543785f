"""GPU-box probe: us per masked timestep of the large-d handle with built-in dynamics at d = 1e5, r = 32, float32 storage, 60 % of the
entries observed (psmf_run_timed, 1 000 steps after a warm-up run, best of three), the gradient sum of theta accumulated over the run:

    python tools/probe_masked_dynamics.py walk cos fourier     -- any of: `walk` the random walk, `cos` cos-phase (n_theta = 32), `fourier` FourierBasis N = 2
                                                                  (n_theta = 4 352)

Every kind that the persistent kernel takes (walk, cos) is timed on it and, PSMF_STEP_PERSISTENT=0, on the launched form; fourier
runs the launched form only.  One process, one series and mask for all of them.  PYTHONPATH in front selects another checkout's
library (a checkout from before masked dynamics runs `walk` only)."""
import os
import sys
import numpy as np
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpsmf_amd import _capi as c

modes = sys.argv[1:] or ["walk", "cos", "fourier"]
d, r, T = 100_000, 32, 1000
rng = np.random.default_rng(1)
Y = (np.cumsum(0.3 * rng.standard_normal((T, d), dtype=np.float32), axis=0) + 3.0).astype(np.float32)
M = (rng.random((T, d), dtype=np.float32) > 0.4).astype(np.uint8)
C0 = rng.random((d, r))
build = c.load_library().psmf_build_id().decode()[:16]


def config(mode):
    if mode == "walk":
        return dict(), None
    if mode == "cos":
        return dict(dyn_kind=c.DYN_COS_PHASE), 1e-3 * np.arange(1, r + 1)
    N = 2                                        # theta = [A_1, D_1, A_2, D_2 (r x r each)] then per n [b_n, c_n, e_n, f_n (r each)]
    th = 0.1 * rng.random(N * (2 * r * r + 4 * r))
    for t in range(2 * N):
        th[t * r * r:(t + 1) * r * r] = (0.5 * np.eye(r) + 0.05 * rng.standard_normal((r, r))).reshape(-1) / N
    return dict(dyn_kind=c.DYN_FOURIER, dyn_terms=N), th


for mode in modes:
    kw, theta = config(mode)
    for persistent in (("1", "0") if mode != "fourier" else ("0",)):
        os.environ["PSMF_STEP_PERSISTENT"] = persistent
        f = c.DeviceFilter(d, r, storage="f32", masked=4 if kw else 1, engine="step", **kw)      # 4 = MASKED_DYNAMICS: a masked handle with f_theta
        f.upload_series(Y)
        f.upload_mask(M)
        f.set_state(C0, 2 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.full(r, 0.3), rho=10.0, theta=theta)
        if theta is not None:
            f.zero_gradsum()
        f.run(0, T)
        ms = [f.run_timed(0, T) for _ in range(3)]
        s = f.get_state(want_C=False)
        assert np.all(np.isfinite(s["mu"])) and np.all(np.isfinite(s["gradsum"]))
        print(f"mode={mode} kernel={f.geometry()['filter_kernel']} d={d} r={r} f32 T={T} n_theta={f.n_theta}: run_timed ms "
              f"{[round(x, 3) for x in ms]} -> {1e3 * min(ms) / T:.2f} us per timestep (best of 3), library {build}", flush=True)
        f.close()
