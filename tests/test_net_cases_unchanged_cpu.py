"""The cases of the random-configuration nets are what they were: tests/golden/net_cases_parent.json holds, per net and per case
index, one SHA-256 over the case dict (canonical JSON) and every array of problem(device_case(i)) in sorted key order, recorded
by tests/golden/make_golden_net_cases.py before the nets were moved onto tests/netlib.py (pmf_net and bpmf_net: when they were added).  A change to a draw, to a table
(RESOLUTION, REPLACED, TARGETS, ...) or to the order of the random draws inside a `problem` shows here, without a GPU.
Wall time: about 15 s, most of it the step net's big-d series."""

import hashlib
import importlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_cases_parent.json")
NETS = {"blocked": "blocked_cases", "step": "step_cases", "impute": "impute_cases", "gram": "gram_cases", "ssm_net": "ssm_net_cases",
        "pmf_net": "pmf_net_cases", "bpmf_net": "bpmf_net_cases"}


def _plain(o):
    if isinstance(o, (np.integer, np.floating, np.bool_)):
        return o.item()
    raise TypeError(type(o))


def case_digest(cs):
    return hashlib.sha256(json.dumps(cs, sort_keys=True, default=_plain).encode()).hexdigest()


def _feed(h, key, v):
    """arrays by dtype, shape and bytes; numbers and None by repr; any other object (the dynamics callable) by its type's name"""
    if isinstance(v, dict):
        for k in sorted(v):
            _feed(h, f"{key}/{k}", v[k])
    elif isinstance(v, (list, tuple)):
        for n, x in enumerate(v):
            _feed(h, f"{key}/{n}", x)
    elif isinstance(v, np.ndarray):
        h.update(f"{key}:{v.dtype.str}:{v.shape}:".encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (np.integer, np.floating, np.bool_)):
        h.update(f"{key}={v.item()!r};".encode())
    elif v is None or isinstance(v, (bool, int, float, str)):
        h.update(f"{key}={v!r};".encode())
    else:
        h.update(f"{key}<{type(v).__name__}>;".encode())


def problem_digest(pb):
    h = hashlib.sha256()
    _feed(h, "", pb)
    return h.hexdigest()


def record(net):
    """one digest per case of a net, as the device test runs it: the SHA-256 of the case's digest followed by its problem's"""
    m = importlib.import_module(NETS[net])
    out = []
    for i in range(m.N_CASES):
        cs = m.device_case(i)
        out.append(hashlib.sha256((case_digest(cs) + problem_digest(m.problem(cs))).encode()).hexdigest())
    return out


@pytest.mark.parametrize("net", sorted(NETS))
def test_cases_and_problems_are_bit_identical(net):
    with open(GOLDEN) as f:
        want = json.load(f)[net]
    got = record(net)
    assert len(got) == len(want), (net, len(got), len(want))
    moved = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not moved, (net, moved[:10])
