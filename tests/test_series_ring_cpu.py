"""The series ring without a GPU: the slot arithmetic run_stream and the library share, the header's statement of the new entry
points, the argument checks that need no device, and the conditioning of the series tests/test_hip_series_ring.py runs."""

import os
import re

import numpy as np
import pytest

import ring_cases as RC
from conftest import ROOT


def test_ring_place_against_a_brute_force_table():
    from rpsmf_amd._capi import ring_place

    for chunk in (1, 2, 5, 37):
        for n_slots in (2, 3, 4):
            # fill the ring row by row the slow way: which buffer row a stream row lands in, and which chunk owns it
            buf = [None] * (n_slots * chunk)
            for t in range(5 * n_slots * chunk + 3):
                c = len([a for a in range(0, t + 1) if a % chunk == 0]) - 1          # chunks begun so far
                slot = c
                while slot >= n_slots:
                    slot -= n_slots
                row = slot * chunk + (t - c * chunk)
                buf[row] = t
                got = ring_place(t, chunk, n_slots)
                assert got == (c, slot, row, t - row), (t, chunk, n_slots, got)
                # the window the kernels see: every row of the chunk so far sits at t' - series_t0
                assert all(buf[u - got[3]] == u for u in range(c * chunk, t + 1))
    for bad in ((-1, 5, 2), (0, 0, 2), (0, 5, 1)):
        with pytest.raises(ValueError):
            ring_place(*bad)


def test_the_header_states_the_ring_entry_points():
    from rpsmf_amd import _capi

    text = open(os.path.join(ROOT, "include", "psmf_hip.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("int psmf_series_ring(psmf_handle h, int64_t chunk, int n_slots);",
                   "int psmf_series_ring_info(psmf_handle h, int64_t* out);",
                   "slot (t / chunk) % n_slots at row offset t % chunk",
                   "PSMF_ERR_ARG across a chunk boundary",
                   "does not synchronise the compute stream",
                   "is no longer resident",
                   "nothing of the call is launched",
                   "psmf_cast_rows"):
        assert phrase in flat, phrase
    assert "#define PSMF_ABI_VERSION 3" in text and _capi.ABI_VERSION == 3
    for name in ("psmf_series_ring", "psmf_series_ring_info"):
        assert name in _capi.SIGNATURES
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_run_stream_checks_its_arguments_before_it_touches_the_device():
    from rpsmf_amd import _capi

    f = object.__new__(_capi.DeviceFilter)          # no handle: these checks come first
    f._h, f.ring, f.masked, f.store_y_pred, f.d_local = None, None, 0, True, 4
    with pytest.raises(ValueError, match="series_ring"):
        f.run_stream([np.zeros((5, 4))])
    f.ring = (5, 2)
    for k0 in (-5, 3):
        with pytest.raises(ValueError, match="multiple of the chunk"):
            f.run_stream([np.zeros((5, 4))], k0=k0)


def test_step_stream_refuses_what_is_not_streamed_by_name():
    import rpsmf_amd as psmf

    d, r = 6, 2
    args = (np.zeros((0, 1)), np.ones((d, r)), np.eye(r), np.zeros((r, 1)), np.eye(r))
    chunks = [np.zeros((4, d))]
    f = psmf.PSMFIter(*args, {0: np.eye(r)}, {0: 1.0}, psmf.RandomWalk(), backend="numpy")
    with pytest.raises(NotImplementedError, match='backend="numpy"'):
        f.step_stream(chunks, 4)
    f = psmf.PSMFIter(*args, {k: (1.0 + k) * np.eye(r) for k in range(4)}, {k: 1.0 for k in range(4)}, psmf.RandomWalk())
    with pytest.raises(NotImplementedError, match="schedules that vary with k"):
        f.step_stream(chunks, 4)
    f = psmf.PSMFIter(np.zeros((r, 1)), *args[1:], {0: np.eye(r)}, {0: 1.0}, lambda th, x, t: np.tanh(x + th), recognise=False)
    with pytest.raises(NotImplementedError, match="host-stepped"):
        f.step_stream(chunks, 4)


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.IDS)
def test_the_streams_of_the_gpu_test_are_well_conditioned(i):
    """the oracle's own answer to a last-bit change of the inputs, and to float32 storage of C where the case stores float32, sits
    16 x inside the bar the device is held to"""
    cs = RC.CASES[i]
    assert len(RC.spans(cs)) == RC.N_CHUNKS and RC.spans(cs)[-1][1] - RC.spans(cs)[-1][0] < cs["chunk"]
    B = min(64 - cs["r"], 48)
    assert cs["chunk"] % B != 0 and {c["chunk"] for c in RC.CASES} == {37, 100} and {c["n_slots"] for c in RC.CASES} == {2, 3}
    inputs, stored = RC.sensitivity(cs)
    print(f"{cs['name']}: sensitivity to the inputs {inputs:.2e}, to float32 storage {stored:.2e}, bar {RC.bar(cs):.0e}")
    assert max(inputs, stored) <= RC.bar(cs) / 16, (cs["name"], inputs, stored)


def test_the_graph_case_is_well_conditioned():
    cs = RC.GRAPH_CASE
    assert cs["chunk"] > 256 and len(RC.spans(cs)) == RC.N_CHUNKS
    inputs, stored = RC.sensitivity(cs)
    print(f"{cs['name']}: sensitivity to the inputs {inputs:.2e}, to float32 storage {stored:.2e}, bar {RC.bar(cs):.0e}")
    assert max(inputs, stored) <= RC.bar(cs) / 16, (cs["name"], inputs, stored)
