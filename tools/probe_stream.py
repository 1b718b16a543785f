"""GPU-box probe: timesteps/s of DeviceFilter.run_stream (series ring, psmf_series_ring) against the resident handle of the same
build, blocked engine, r = 32, float32, T = 10 000, chunks of 960 rows.  Streamed, every timestep moves 4 d bytes to the device
and 4 d bytes back, so at d = 1e5 (resident: ~300 k timesteps/s = 120 GB/s each way) the figure IS the host link; what the ring
itself costs shows at d = 2e4 and with store_y_pred=False.  Warm-up pass, then the two handles alternate; medians and the spread.
One JSON line per configuration.

    python tools/probe_stream.py [--d 20000 100000] [--T 10000] [--chunk 960] [--slots 2] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpsmf_amd import _capi as c


def state(f, C0, r):
    f.set_state(C0, 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0, lambda0=1.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--r", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=960)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if c.device_count() < 1:
        raise SystemExit("probe_stream: no HIP device (nothing is measured without one)")
    T, r, ch = a.T, a.r, a.chunk
    for d in a.d:
        rng = np.random.default_rng(d)
        Ct = rng.standard_normal((d, r)).astype(np.float32)
        Y = np.empty((T, d), dtype=np.float32)
        for t0 in range(0, T, 500):
            n = min(500, T - t0)
            Y[t0:t0 + n] = rng.standard_normal((n, r)).astype(np.float32) @ Ct.T + 0.3 * rng.standard_normal((n, d), dtype=np.float32)
        C0 = 0.1 * rng.standard_normal((d, r))
        chunks = [Y[k:k + ch] for k in range(0, T, ch)]
        res = c.DeviceFilter(d, r, storage="f32", engine="block")
        t = time.perf_counter()
        res.upload_series(Y)
        res.sync()
        up_s = time.perf_counter() - t
        state(res, C0, r)
        rings = {yp: c.DeviceFilter(d, r, storage="f32", engine="block", store_y_pred=yp) for yp in (True, False)}
        for f in rings.values():
            f.series_ring(ch, a.slots)

        def resident():
            state(res, C0, r)
            t = time.perf_counter()
            res.run(0, T)
            return time.perf_counter() - t

        def streamed(yp):
            f = rings[yp]
            state(f, C0, r)
            t = time.perf_counter()
            for _ in f.run_stream(chunks, y_pred_dtype=np.float32):
                pass
            return time.perf_counter() - t

        times = {"resident": [], True: [], False: []}
        resident(), streamed(True), streamed(False)          # warm-up: every kernel, every buffer, the copy paths
        for _ in range(a.reps):
            times["resident"].append(resident())
            times[True].append(streamed(True))
            times[False].append(streamed(False))
        t = time.perf_counter()
        yp = res.y_pred(0, ch, dtype=np.float32)
        down_s = time.perf_counter() - t
        ring_last = rings[True].y_pred(T - len(chunks[-1]), len(chunks[-1]), dtype=np.float32)
        same = bool(np.array_equal(ring_last, res.y_pred(T - len(chunks[-1]), len(chunks[-1]), dtype=np.float32)))

        # a chunk from pageable and from pinned host memory into the resident buffer (its runs are over): what a pair of pinned
        # staging buffers owned by the handle could gain on this box
        def chunk_copy_GBps(a_, reps=5):
            res.upload_series(a_, 0, T_total=T)
            res.sync()
            t = time.perf_counter()
            for _ in range(reps):
                res.upload_series(a_, 0, T_total=T)
            res.sync()
            return round(reps * a_.nbytes / (time.perf_counter() - t) / 1e9, 2)

        h2d_chunk_pageable = chunk_copy_GBps(np.ascontiguousarray(chunks[0]))
        try:
            import torch

            pinned = torch.empty((ch, d), dtype=torch.float32).pin_memory().numpy()
            pinned[:] = chunks[0]
            h2d_chunk_pinned = chunk_copy_GBps(pinned)
            t = time.perf_counter()
            for _ in range(5):
                pinned[:] = chunks[1]
            host_copy_GBps = round(5 * pinned.nbytes / (time.perf_counter() - t) / 1e9, 2)
            del pinned
        except ImportError:
            h2d_chunk_pinned = host_copy_GBps = None

        def rate(v):
            v = sorted(v)
            return dict(median=round(T / v[len(v) // 2]), best=round(T / v[0]), worst=round(T / v[-1]))

        # the link bounds the streamed figure at (pageable host-to-device rate) / (4 d bytes per timestep); within 20 % of it the
        # run has measured the link
        link_rate, streamed_rate = Y.nbytes / up_s / (4 * d), rate(times[True])["median"]
        out = dict(probe="stream", d=d, r=r, T=T, chunk=ch, n_slots=a.slots, reps=a.reps, kernel=res.geometry()["filter_kernel"],
                   resident_steps_per_s=rate(times["resident"]), streamed_steps_per_s=rate(times[True]),
                   streamed_no_y_pred_steps_per_s=rate(times[False]),
                   h2d_GBps_pageable=round(Y.nbytes / up_s / 1e9, 2), d2h_GBps_pageable=round(yp.nbytes / down_s / 1e9, 2),
                   link_bound_steps_per_s=round(link_rate), pinned_staging=False,
                   h2d_chunk_GBps_pageable=h2d_chunk_pageable, h2d_chunk_GBps_pinned=h2d_chunk_pinned, host_copy_into_pinned_GBps=host_copy_GBps,
                   resident_pass_and_streamed_pass_agree_on_last_chunk_bits=same,
                   note="the streamed figure is the host link's, not the ring's" if streamed_rate >= 0.8 * link_rate else "")
        print(json.dumps(out), flush=True)
        res.close()
        for f in rings.values():
            f.close()


if __name__ == "__main__":
    main()
