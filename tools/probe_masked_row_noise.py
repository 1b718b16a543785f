"""GPU-box probe: us per masked timestep of the large-d handle at d = 1e5, r = 32, float32 storage (psmf_run_timed, 1 000 steps after a
warm-up run, best of three):  python tools/probe_masked_row_noise.py uniform|rows   -- `uniform`: R = 10 I (set PSMF_STEP_PERSISTENT=0
for the launched form), `rows`: per-row noise over a 100 x spread (nonuniform_R: always the launched form, one Gram pass more).
PYTHONPATH in front selects another checkout's library."""
import os
import sys
import numpy as np
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpsmf_amd import _capi as c

mode = sys.argv[1]
d, r, T = 100_000, 32, 1000
rng = np.random.default_rng(1)
Y = (np.cumsum(0.3 * rng.standard_normal((T, d), dtype=np.float32), axis=0) + 3.0).astype(np.float32)
M = (rng.random((T, d), dtype=np.float32) > 0.4).astype(np.uint8)
C0 = rng.random((d, r))
rows = mode == "rows"
f = c.DeviceFilter(d, r, storage="f32", masked=1, engine="step", nonuniform_R=rows)
f.upload_series(Y)
f.upload_mask(M)
if rows:
    f.set_row_noise(10.0 * 100.0 ** (rng.random(d) - 0.5))
f.set_state(C0, 2 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.full(r, 0.3), rho=1.0 if rows else 10.0)
f.run(0, T)
ms = [f.run_timed(0, T) for _ in range(3)]
print(f"mode={mode} kernel={f.geometry()['filter_kernel']} d={d} r={r} f32 T={T}: run_timed ms {ms} -> {1e3 * min(ms) / T:.2f} us per timestep (best of 3), "
      f"library {c.load_library().psmf_build_id().decode()[:16]}")
f.close()
