"""GPU-box probe: per-pass time of psmf_blk_filter4 (per-step schedules, r = 24, d = 20 000, T = 3 200): event-timed pass and the
in-situ duration of a block, for comparing two builds on one box."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rpsmf_amd import _capi
import bench

d, r, T = 20000, 24, 3200
ser = bench.Series(d, r, T, 4711, 0, d, False)
st0 = bench.init_state(d, r, 4711)
f = _capi.DeviceFilter(d, r, storage="f32")
f.set_schedules(np.ones(T + 1), np.linspace(1.0, 1.2, T + 1))
for a, Yc in ser.chunks():
    f.upload_series(Yc, t0=a, T_total=T)
f.set_state(st0["C"], st0["V"], st0["P"], st0["Q"], st0["mu"], rho=st0["rho"], lambda0=st0["lam"])
for i in range(6):
    f.counters(reset=True)
    ms = f.run_timed(0, T)
    c = f.counters()
    print(f"pass {i}: {f.geometry()['filter_kernel']} {1e3 * ms / T:.3f} us/step (event) | in-situ per block {c['filter_us_mean']:.1f} us, gap {c['filter_gap_us_mean']:.1f} us "
          f"({c['filter_launches']} blocks, {c['filter_kernel_launches']} launches) ns/sw/it/fail={c['ns_steps']}/{c['sweep_steps']}/{c['ns_iterations']}/{c['ns_failed']}", flush=True)
f.close()
