"""Device memory returns after the handle does.  Every device buffer, event and stream of the native library belongs to an owning
object (rpsmf_amd/csrc/psmf_own.h) and psmf_destroy deletes the handle; a member that were not of such a type would stay behind at
every close.  Each lifecycle below creates, uses and closes handles (or calls a handle-free entry point) the way the other GPU tests
do -- no bad argument, no failure path -- and free device memory, read with hipMemGetInfo, must not keep falling: after one warm-up
cycle (code objects, the runtime's own pools) it is read after 5 further cycles and after 10 (1029 for the per-step engine), and

    free(5) - free(10) <= PARENT_DRIFT + GRANULE.

PARENT_DRIFT is what the same script measured on the parent commit, whose success paths free everything by hand: 0 bytes for every
lifecycle, the reading the same after each of the ten cycles.  GRANULE is the smallest non-zero step hipMemGetInfo showed on that
MI355X: 2 MiB.  Smaller allocations share a 2 MiB block of the runtime and do not move the reading until a block is full: five 2 KiB
allocations that are never freed -- the size of the smallest buffer of a handle, (b)'s theta block of 4 x 64 doubles -- left it
unchanged, every 512th took 2 MiB from it (4 KiB each), and so did not even a 1 MiB allocation behind them.  With a margin of one
granule the loss of that buffer shows for certain only once two blocks have gone, 1024 cycles later.  The per-step lifecycle (b), at
5 ms a cycle, therefore reads after 5 and after 1029 cycles (5 s; the parent's drift over them: 0 bytes as well); the others, whose handles own the same members and cost up to
60 ms a cycle, stay at 5 and 10 and catch what moves the reading there: a lost series, dictionary or staging buffer, a handle that
is not deleted.  The member-by-member statement is tests/test_native_ownership.py.  docs/MEASUREMENTS.md has the figures.
GPU only: `pytest -m gpu`."""

import ctypes as C

import numpy as np
import pytest

from oracle import psmf_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

PARENT_DRIFT = 0            # bytes: free(first) - free(last) of every lifecycle on the parent commit
GRANULE = 2 << 20           # bytes: the smallest non-zero step of hipMemGetInfo's free memory
CYCLES = (5, 10)
CYCLES_SMALLEST_BUFFER = (5, 5 + 2 * 512)       # per_step: two 2 MiB blocks of 4 KiB allocations apart


def free_bytes():
    """free device memory by hipMemGetInfo, from the HIP runtime the native library has loaded already"""
    from rpsmf_amd import _capi as c

    c.load_library()
    hip = C.CDLL(None)                  # (libpsmf_hip.so is loaded RTLD_GLOBAL: its libamdhip64.so answers)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def _state(f, d, r, seed):
    f.set_state(0.1 * np.random.default_rng(seed).standard_normal((d, r)), 0.1 * np.eye(r), np.eye(r), 0.1 * np.eye(r), np.zeros(r), rho=1.0, lambda0=1.8)


def _timed(kw, d, r, T, whiches):
    from rpsmf_amd import _capi as c

    Y = O.synthetic_series(d, r, T, 4100 + r, dtype=np.float64)
    f = c.DeviceFilter(d, r, **kw)
    try:
        f.upload_series(Y)
        _state(f, d, r, r)
        f.run(0, T // 2)
        for which in whiches:
            assert f.time_kernel(which, 3) > 0.0
        assert f.get_state()["k"] == T // 2
    finally:
        f.close()


def blocked():
    _timed(dict(engine="block", storage="f64"), 777, 12, 110, (0, 1, 2))


def per_step():
    _timed(dict(engine="step", storage="f64"), 1000, 20, 40, (0, 1))


def masked():
    from rpsmf_amd import _capi as c

    d, r, T = 600, 6, 30
    rng = np.random.default_rng(5)
    Y = O.synthetic_series(d, r, T, 77, dtype=np.float64)
    M = rng.random((T, d)) > 0.3
    held = ~M & (rng.random((T, d)) > 0.5)
    f = c.DeviceFilter(d, r, masked=True, engine="step", storage="f64")
    try:
        f.upload_series(Y)
        f.upload_mask(M)
        _state(f, d, r, 3)
        f.run(0, T)
        a = f.masked_metrics(held[:10], 2.0, 0)
        b = f.masked_metrics(held, 2.0, 0)            # longer than the first: the staging buffer of the held-out mask grows
        assert b[3] >= a[3] > 0
    finally:
        f.close()


def ring():
    from rpsmf_amd import _capi as c

    d, r, T, chunk = 300, 8, 80, 16
    Y = O.synthetic_series(d, r, T, 78, dtype=np.float64)      # float64 rows into float32 storage: converted through the ring's staging buffer
    f = c.DeviceFilter(d, r, engine="step", storage="f32")
    try:
        f.series_ring(chunk, 2)
        _state(f, d, r, 4)
        ends = [ke for _kb, ke, _yp in f.run_stream(Y[j:j + chunk] for j in range(0, T, chunk))]
        assert ends[-1] == T
    finally:
        f.close()


def impute_small():
    from rpsmf_amd import impute

    d, n, r, B = 19, 200, 4, 3
    rng = np.random.default_rng(6)
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, n)), axis=1)
    M = (rng.random((B, d, n)) > 0.4).astype(int)
    M[:, 0, :] = 1
    Mmiss = ((1 - M) * (rng.random((B, d, n)) > 0.2)).astype(float)
    C0, X0 = rng.random((B, d, r)), rng.random((B, r, n))
    V, Q, P = 2 * np.eye(r), 0.1 * np.eye(r), np.eye(r)
    for R in (10.0, 10.0 * (1.0 + rng.random(d))):        # psmf_impute_run, psmf_impute_run_rows
        res = impute.impute_batch(Yorig, M, Mmiss, C0, X0, V, Q, R, P, 2, 2, want_bands=True)
        assert np.all(res["status"] == 0)


def reupload_and_schedules():
    from rpsmf_amd import _capi as c

    d, r = 200, 5
    Y = O.synthetic_series(d, r, 40, 79, dtype=np.float64)
    f = c.DeviceFilter(d, r, engine="step", storage="f64")
    try:
        f.upload_series(Y[:20])
        f.upload_series(Y)                 # from t0 = 0 and longer: the series buffers are allocated again
        _state(f, d, r, 5)
        f.set_schedules(np.ones(50), None)
        f.run(0, 40)
        f.set_schedules(np.ones(45), 1.0 + np.arange(45.0) / 45.0)
        f.run(0, 40)
    finally:
        f.close()


LIFECYCLES = [blocked, per_step, masked, ring, impute_small, reupload_and_schedules]


def free_after_cycles(cycle, counts):
    """free device memory after counts[0], counts[1], ... cycles, following one warm-up cycle"""
    cycle()
    out, done = [], 0
    for n in counts:
        for _ in range(n - done):
            cycle()
        done = n
        out.append(free_bytes())
    return out


@pytest.mark.parametrize("cycle", LIFECYCLES, ids=[f.__name__ for f in LIFECYCLES])
def test_free_memory_does_not_fall_from_cycle_to_cycle(cycle):
    counts = CYCLES_SMALLEST_BUFFER if cycle is per_step else CYCLES
    first, last = free_after_cycles(cycle, counts)
    print(f"\n{cycle.__name__}: free after {counts[0]} cycles {first}, after {counts[1]} cycles {last}, fell by {first - last} bytes")
    assert first - last <= PARENT_DRIFT + GRANULE, (cycle.__name__, counts, first, last)
