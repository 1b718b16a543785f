"""Sub-ranges of the series buffers: the downloads and reductions of a resident handle and of a 2-slot series ring over the same
inputs, at ranges that do not start at step 0 and that straddle a chunk boundary of the ring.  GPU only: `pytest -m gpu`; `-s` shows
the figures (each prints before it asserts).

Cases of tests/ring_cases.py cut to T = 75 rows in chunks of 37 (chunk 0 = steps 1 .. 37, chunk 1 = 38 .. 74), float32 storage at
d = 257, r = 8 -- unmasked on the blocked engine, masked on the per-step engine -- and the d = 1 case as it stands.  Both handles
run (0, 37) and (37, 70), so that the masked handle's look-ahead row stays inside chunk 1, and every question is asked while
chunks 0 and 1 are both resident.

1. sq_error(t0, nt) at t0 = 5 and across row 37 against the host's sum over the downloaded rows (1e-10, the bar of
   test_hip_series_ring.py for the same comparison), on both handles; both handles bit for bit where the range lies in one chunk.
   Across a chunk boundary the ring adds the partial sums of two launches and the resident handle those of one, and float64
   addition does not associate: 957.111198906622 against 957.1111989066222 for (30, 20), 5585.441258501167 against
   5585.441258501165 for (5, 50) of the masked case -- one unit in the last place, so no bit-for-bit claim is made there.
2. y_pred(t0, nt, dtype=other) for t0 > 0 is numpy's cast of the native download, exactly, on both handles.
3. A resident upload of the other element type in two blocks gives the bits of one block converted by numpy beforehand.
4. masked_metrics and step_scalars at t0 = 5, nt = 50: step_scalars of resident and ring bit for bit; the ring's four sums are
   bit for bit the resident handle's over the ring's two pieces, (5, 32) + (37, 18), added in that order (one launch over all 50
   steps adds the same partial sums in another association and differs in the last place, as in 1.); the resident sums against
   numpy over y_pred, mu_history, step_scalars and the final C (1e-9 on the sums, the counts exact: tests/test_hip_masked_large.py).
5. mu_history from k0 = 37, the mean chunk 1 starts from: resident and ring bit for bit."""

import numpy as np
import pytest

import ring_cases as RC
import netlib
from conftest import relerr
from test_hip_series_ring import STATE_KEYS, _handle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

T, CH, K_END = 75, 37, 70
RANGES = ((5, 20), (5, 50), (30, 20))          # inside chunk 0; across row 37 from t0 = 5; across row 37, short
SIG = 2.0


def _named(name):
    return next(c for c in RC.CASES if c["name"] == name)


CASES = {
    "block f32": dict(_named("block r=5 random walk"), r=8, T=T),
    "masked step f32": dict(_named("masked persistent"), storage="f32", n_slots=2, T=T),
    "block d=1": dict(_named("block filter7 scaled walk"), T=T),
}
assert all(c["chunk"] == CH and c["n_slots"] == 2 for c in CASES.values())


def _ask(f, cs, pb, held):
    native, other = (np.float32, np.float64) if cs["storage"] == "f32" else (np.float64, np.float32)
    out = dict(sq={rg: f.sq_error(*rg) for rg in RANGES}, yp={rg: f.y_pred(*rg, dtype=native) for rg in RANGES},
               yp_other={rg: f.y_pred(*rg, dtype=other) for rg in RANGES}, mu={kn: f.mu_history(*kn) for kn in ((37, 1), (37, 20), (6, 50))})
    if cs["masked"]:
        out.update(metrics=f.masked_metrics(held[5:55], SIG, 5), sc=f.step_scalars(5, 50), C=f.get_state()["C"],
                   metrics_by_chunk=f.masked_metrics(held[5:CH], SIG, 5) + f.masked_metrics(held[CH:55], SIG, CH))
    return out


_RUNS = {}


def _runs(name):
    """what the resident handle and the ring answer, asked once for the tests that share it"""
    if name not in _RUNS:
        c, cs = netlib.capi(), CASES[name]
        pb = RC.problem(cs)
        held = ((np.random.default_rng(5).random((T, cs["d"])) < 0.3) & (pb["M"] == 0)).astype(np.uint8) if cs["masked"] else None
        res, ring = _handle(c, cs, pb, ring=False), _handle(c, cs, pb, ring=True)
        try:
            res.upload_series(pb["Y"])
            for j in range(2):
                ring.upload_series(pb["Y"][j * CH:(j + 1) * CH], j * CH)
            if cs["masked"]:
                res.upload_mask(pb["M"])
                for j in range(2):
                    ring.upload_mask(pb["M"][j * CH:(j + 1) * CH], j * CH)
            for f in (res, ring):
                f.run(0, CH)
                f.run(CH, K_END)
            assert ring.series_ring_info()["slots"] == [0, 1]
            _RUNS[name] = dict(cs=cs, pb=pb, held=held, res=_ask(res, cs, pb, held), ring=_ask(ring, cs, pb, held))
        finally:
            res.close()
            ring.close()
    return _RUNS[name]


def _stored(cs, Y):
    return Y.astype(np.float32).astype(np.float64) if cs["storage"] == "f32" else Y


@pytest.mark.parametrize("name", list(CASES))
def test_sq_error_of_a_sub_range(name):
    run = _runs(name)
    Y = _stored(run["cs"], run["pb"]["Y"])
    for t0, nt in RANGES:
        want = {k: float(np.sum((run[k]["yp"][t0, nt].astype(np.float64) - Y[t0:t0 + nt]) ** 2)) for k in ("res", "ring")}
        got = {k: run[k]["sq"][t0, nt] for k in ("res", "ring")}
        print(f"\nSUBRANGE {name} sq_error({t0}, {nt}): resident {got['res']!r} ring {got['ring']!r} host {want['res']!r}")
        assert relerr(got["res"], want["res"]) < 1e-10 and relerr(got["ring"], want["ring"]) < 1e-10
        if t0 // CH == (t0 + nt - 1) // CH:
            assert got["res"] == got["ring"]


@pytest.mark.parametrize("name", list(CASES))
def test_y_pred_in_the_other_dtype_is_numpys_cast(name):
    run = _runs(name)
    for k in ("res", "ring"):
        for rg in RANGES:
            native, other = run[k]["yp"][rg], run[k]["yp_other"][rg]
            assert native.dtype != other.dtype and np.array_equal(other, native.astype(other.dtype)), (name, k, rg)
    for rg in RANGES:
        assert np.array_equal(run["res"]["yp"][rg], run["ring"]["yp"][rg]), (name, rg)


def test_a_resident_upload_of_the_other_dtype_in_two_blocks():
    c, cs = netlib.capi(), CASES["block f32"]
    pb = RC.problem(cs)
    Y = pb["Y"]
    assert Y.dtype == np.float64 and Y.shape == (T, cs["d"])
    got = []
    for blocks in (((0, Y.astype(np.float32)),), ((0, Y[:40]), (40, Y[40:]))):
        f = _handle(c, cs, pb, ring=False)
        try:
            for t0, rows in blocks:
                f.upload_series(rows, t0, T_total=T)
            f.run(0, T)
            got.append((f.get_state(), f.y_pred(0, T, dtype=np.float32)))
        finally:
            f.close()
    (s0, yp0), (s1, yp1) = got
    diff = [k for k in STATE_KEYS if not np.array_equal(np.asarray(s0[k]), np.asarray(s1[k]))]
    assert not diff and np.array_equal(yp0, yp1), diff


def test_masked_metrics_and_step_scalars_of_a_sub_range():
    run = _runs("masked step f32")
    cs, pb, res, ring = run["cs"], run["pb"], run["res"], run["ring"]
    t0, nt = 5, 50
    held = run["held"][t0:t0 + nt].astype(np.float64)
    Y = _stored(cs, pb["Y"])[t0:t0 + nt]
    yp = res["yp"][t0, nt].astype(np.float64)
    X = res["mu"][6, 50]                         # row t + 1 of the mean history = x_t
    sc = res["sc"]
    band = SIG * np.sqrt(sc[:, 0] + sc[:, 1])[:, None]
    want = np.array([np.sum(held * (yp - Y) ** 2), np.sum(held * (X @ res["C"].T - Y) ** 2),
                     np.sum(held * ((Y < yp + band) & (yp - band < Y))), held.sum()])
    print(f"\nSUBRANGE masked_metrics({t0}, {nt}): resident {res['metrics']} ring {ring['metrics']} host {want}")
    assert want[3] > 0
    assert relerr(np.sqrt(res["metrics"][0] / want[3]), np.sqrt(want[0] / want[3])) < 1e-9
    assert relerr(np.sqrt(res["metrics"][1] / want[3]), np.sqrt(want[1] / want[3])) < 1e-9
    assert abs(res["metrics"][2] / want[3] - want[2] / want[3]) < 1e-12 and res["metrics"][3] == want[3]
    assert np.array_equal(res["sc"], ring["sc"])
    assert np.array_equal(res["metrics_by_chunk"], ring["metrics"]) and np.array_equal(ring["metrics_by_chunk"], ring["metrics"])
    assert np.array_equal(res["metrics"][2:], ring["metrics"][2:])      # the counts are exact in any order


@pytest.mark.parametrize("name", list(CASES))
def test_mu_history_from_the_mean_a_chunk_starts_from(name):
    run = _runs(name)
    for kn in run["res"]["mu"]:
        assert np.array_equal(run["res"]["mu"][kn], run["ring"]["mu"][kn]), (name, kn)
    assert np.array_equal(run["res"]["mu"][37, 1][0], run["res"]["mu"][6, 50][31])      # row 37, read in two ways
