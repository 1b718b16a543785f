"""tests/blocked_cases.py without a GPU: (1) the seeded case list of the blocked engine's random-configuration net covers what it
claims to cover -- every coefficient-space kernel, both families and both instantiations of the d-sized kernels, every tiny row
count, horizon edge and cut edge, every dynamics kind on every kernel that can take it -- so that the net cannot go thin
unnoticed; (2) every case is well enough conditioned for its tolerance to mean something: the float64 oracle runs it to finite
values, and its answer moves by at most 1/16 of the case's bar when C0, Y and theta move by a relative 2^-50 (float32 storage:
2^-23, after the rounding to float32).  DESIGN 2c: the full cos-phase filter amplifies a last-bit difference by 1e5 per 50
steps -- such a case would fail on the device for no fault of a kernel.  A case that is not admissible is halved (not below
B + 1 steps, at most twice), then redrawn; blocked_cases.RESOLUTION records the outcome and this file recomputes it.
Wall time: about two and a half minutes on one core (the oracle differentiates the dynamics by complex step).
Reference: pypsmf/psmf/psmf.py:85-180, rpsmf.py:116-184 (through oracle/psmf_oracle.py)."""

from collections import Counter

import numpy as np
import pytest

import blocked_cases as BC

CASES = [BC.device_case(i) for i in range(BC.N_CASES)]


def test_the_case_list_is_what_the_table_says():
    assert BC.N_CASES == 3 * len(BC.TARGETS) and set(k for k, _ in BC.TARGETS) == set(BC.KERNELS) and len(BC.KERNELS) == 10
    for i, cs in enumerate(CASES):
        assert (BC.expected_kernel(cs), cs["dyn"]) == BC.TARGETS[i % len(BC.TARGETS)], i
        assert cs["parts"][0][0] == 0 and cs["parts"][-1][1] == cs["T"] and all(a <= b for a, b in cs["parts"])
        assert all(p[1] == q[0] for p, q in zip(cs["parts"][:-1], cs["parts"][1:])), cs["parts"]
        assert 1 <= cs["r"] <= 32 and cs["B"] == min(64 - cs["r"], 48) and cs["d"] >= 1 and cs["T"] >= 1
        if cs["shards"]:
            assert sum(cs["shards"]) == cs["d"] and min(cs["shards"]) in (1, 2, 3) and len(cs["shards"]) in (2, 3)
        assert not (cs["sched"] and cs["robust"]) and not (cs["recursive"] and cs["dyn"] == "random_walk")


def test_every_kernel_and_both_bulk_families():
    kernels = Counter(BC.expected_kernel(cs) for cs in CASES)
    print("\ncases per kernel:", dict(kernels))
    assert set(kernels) == set(BC.KERNELS) and min(kernels.values()) >= 6, kernels
    # (the general kernel's three instantiations <8>, <16>, <32>: padded rank 8, 16, 32)
    general = Counter(8 if cs["r"] <= 8 else (16 if cs["r"] <= 16 else 32) for cs in CASES if BC.expected_kernel(cs) == "psmf_blk_filter")
    assert set(general) == {8, 16, 32}, general
    bulk = Counter()
    for cs in CASES:
        for dl in (cs["shards"] or [cs["d"]]):
            bulk[BC.expected_bulk(cs, dl)] += 1
    print("handles per bulk-kernel choice:", dict(bulk))
    assert bulk[("streaming", 2)] >= 3 and bulk[("streaming", 3)] >= 3 and bulk[("mfma", None)] >= 3, bulk
    # the MFMA family on a float32 row stride with general dynamics (float32 storage, d not a multiple of 4)
    assert any(cs["storage"] == "f32" and cs["d"] % 4 and cs["dyn"] in BC.DENSE_KINDS and not cs["shards"] for cs in CASES)
    # ... and the same across a block edge (T > B): the affine kinds, the only device-evaluated dynamics that are admissible on
    # float32 inputs over more than a few steps
    across = [cs["i"] for cs in CASES if cs["storage"] == "f32" and cs["d"] % 4 and cs["dyn"] in BC.LINEAR_KINDS and not cs["shards"] and cs["T"] > cs["B"]]
    print("float32 storage, d % 4 != 0, ScaledWalk, T > B:", across)
    assert across
    assert {cs["d"] % 4 for cs in CASES if cs["storage"] == "f32"} == {0, 1, 2, 3}


def test_every_row_horizon_and_cut_edge():
    tiny = Counter()
    for cs in CASES:
        if cs["d"] in BC.tiny_rows(cs["r"]):
            tiny[cs["d"]] += 1
    for d in (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513):
        assert tiny[d] >= 1, (d, tiny)
    assert any(cs["d"] == cs["r"] - 1 for cs in CASES) and any(cs["d"] == cs["r"] for cs in CASES) and any(cs["d"] == cs["r"] + 1 for cs in CASES)
    assert any(cs["d"] < cs["r"] for cs in CASES) and any(cs["d"] > 4096 for cs in CASES)
    t_edges = Counter()
    c_edges = Counter()
    for cs in CASES:
        B, T = cs["B"], cs["T"]
        for name, v in (("1", 1), ("2", 2), ("B-1", B - 1), ("B", B), ("B+1", B + 1), ("2B", 2 * B), ("2B+1", 2 * B + 1), ("3B-1", 3 * B - 1)):
            t_edges[name] += T == v
        cuts = {b for _, b in cs["parts"][:-1]}
        for name, v in (("1", 1), ("B-1", B - 1), ("B", B), ("B+1", B + 1), ("T-1", T - 1)):
            c_edges[name] += (v in cuts and 1 <= v <= T - 1)
    print("\nhorizon edges:", dict(t_edges), "\ncut edges:", dict(c_edges))
    assert min(t_edges.values()) >= 1 and len(t_edges) == 8, t_edges
    assert min(c_edges.values()) >= 1 and len(c_edges) == 5, c_edges
    # a cut at every edge for every kernel family at least where the horizon admits it: B - 1, B, B + 1 each on >= 4 kernels
    for name in ("B-1", "B", "B+1"):
        ks = {BC.expected_kernel(cs) for cs in CASES for _, b in cs["parts"][:-1]
              if b == {"B-1": cs["B"] - 1, "B": cs["B"], "B+1": cs["B"] + 1}[name] and 1 <= b <= cs["T"] - 1}
        assert len(ks) >= 4, (name, ks)
    assert sum(1 for cs in CASES if any(a == b for a, b in cs["parts"])) >= 5          # empty runs
    assert sum(1 for cs in CASES if cs["second_pass"]) >= 20 and sum(1 for cs in CASES if cs["shards"]) >= 10


def test_every_kind_on_every_kernel_that_takes_it_and_the_other_axes():
    seen = {(BC.expected_kernel(cs), cs["dyn"]) for cs in CASES}
    for kernel in BC.KERNELS:
        for kind in BC.kinds_of(kernel):
            assert (kernel, kind) in seen, (kernel, kind)
    assert {cs["hooks"] for cs in CASES} == set(BC.HOOKS)
    assert {cs["recursive"] for cs in CASES} == {0, 1, 2} and len({cs["update_every"] for cs in CASES if cs["recursive"]}) >= 3
    assert any(cs["robust"] and cs["fixed_lambda"] for cs in CASES) and any(cs["robust"] and cs["alpha"] != 1.0 for cs in CASES)
    assert any(cs["sched"] for cs in CASES) and any(cs["general_Q"] for cs in CASES)
    for name in ("PSMF_FILTER6_DUAL", "PSMF_FILTER6", "PSMF_FILTER3", "PSMF_FILTER7", "PSMF_BULK2", "PSMF_BLOCK_CHAIN", "PSMF_BLOCK_PIPE", "PSMF_CHAIN_CARRY"):
        assert any(cs["env"].get(name) == "0" for cs in CASES), name
    assert {cs["storage"] for cs in CASES} == {"f32", "f64"}


def test_at_most_a_tenth_of_the_cases_was_shortened_or_replaced():
    print("\nshortened or replaced (case: (salt, times halved)):", BC.RESOLUTION)
    assert len(BC.RESOLUTION) <= BC.N_CASES // 10, len(BC.RESOLUTION)


@pytest.mark.parametrize("i", range(BC.N_CASES))
def test_case_is_admissible_by_the_oracle_alone(i):
    """No LinAlgError, finite, and the oracle's response to a last-bit change of the inputs is at most bar / 16: for the recorded
    resolution of the case, and -- for the cases the table lists -- not for the draw it replaced."""
    (salt, halved), log = BC.resolve(i)
    for line in log:
        print("\nnot admissible:", line)
    assert (salt, halved) == BC.RESOLUTION.get(i, (0, 0)), (i, salt, halved, log)
