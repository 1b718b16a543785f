"""The BPMF baseline without a GPU: the case list of tests/bpmf_cases.py is admitted whole and the bar of the device tests follows from
what the model shows, the draw protocol of rpsmf_amd.bpmf.draw_bpmf is scipy's and the reference's, the numpy model of
tests/bpmf_model.py reproduces the reference's stored answers, the fixture belongs to the inputs the other known-answer fixtures hold,
rpsmf_amd.bpmf refuses what it documents before it looks for a device, bpmf() has the reference's parameter list, and psmf_bpmf.hip
stands on the host scaffold as the other entry points without a handle do (the rules of tests/test_native_batch.py, through its
helpers)."""

import inspect
import re

import numpy as np
import pytest

import bpmf_cases as BC
import kat_replay
from conftest import load_golden
from test_native_batch import BATCH, SCAFFOLD_CALLS, _host_part, _read

UNIT = "psmf_bpmf.hip"
# ExperimentImpute/BPMF.py:121-134
REFERENCE_PARAMETERS = ("Y", "C", "X", "num_p", "num_m", "num_feat", "M", "Mmiss", "YorigInt", "Einit", "epochs", "beta")
REFERENCE_DEFAULTS = dict(epochs=50, beta=2)
ISSUE_SHAPES = [(2, 5, 2, 1, 1), (3, 23, 2, 2, 2), (19, 700, 10, 2, 3), (27, 257, 10, 2, 2), (80, 130, 16, 3, 2), (200, 70, 7, 2, 2), (505, 96, 10, 2, 2),
                (512, 33, 16, 1, 1), (17, 3000, 5, 2, 4)]


@pytest.mark.parametrize("i", range(len(BC.CASES)), ids=[c["name"] for c in BC.CASES])
def test_every_case_is_admitted(i):
    ok, text, _ = BC.admission(i)
    print(text)
    assert ok, text


def test_the_list_is_the_issue_s_and_covers_what_it_says():
    shapes = [(c["d"], c["n"], c["r"], c["epochs"], c["batch"]) for c in BC.CASES]
    assert shapes[:9] == ISSUE_SHAPES
    assert {(n, r) for d, n, r, ep, B in shapes[9:]} == {(16, 15), (17, 15), (33, 15)}
    assert all((c["warm_start"] is not None) == (c["d"] * c["n"] < BC.TINY) for c in BC.CASES), "only the tiny shapes run another warm start"
    for c in BC.CASES:
        pb = BC.problem(c["i"])
        if c["batch"] > 1:
            assert not np.array_equal(pb["M"][0], pb["M"][1]) and not np.array_equal(pb["C0"][0], pb["C0"][1])
            assert not np.array_equal(pb["draws"][0]["normals"], pb["draws"][1]["normals"])
        for b in range(c["batch"]):
            M, Mm = pb["M"][b] != 0, pb["Mmiss"][b] != 0
            assert Mm.any()
            if c["n"] > 5:
                assert np.any(~M.any(axis=0) & Mm.any(axis=0)), f"{c['name']}: a column without a training entry but with a probe entry"
            if c["d"] > 2:
                assert np.any(~M.any(axis=1)), f"{c['name']}: a row without a training entry"
        for arr in (pb["M"], pb["Mmiss"]):
            assert set(np.unique(arr)) <= {0, 1}


def test_the_device_bar_is_fifty_times_what_the_model_shows():
    """bpmf_cases.TOL by its rule.  The largest disagreement between the model's algebras and orders, here over every case and the
    first three repeats of LondonAir_PM25 at 20 % (8.1e-14), is the figure written beside it (9.7e-14, over five repeats of all nine
    files) within a factor of two: BLAS builds differ, and this test takes three repeats of one file to stay quick."""
    worst = max(BC.admission(c["i"])[2] for c in BC.CASES)
    for dr in BC.kat_inputs("pm25", 20, 3):
        worst = max(worst, BC.disagreement(BC.kat_model(dr), [BC.kat_model(dr, a, o) for a, o in BC.VARIANTS]))
    print(f"largest disagreement of the model with itself: {worst:.2e} (written down: {BC.MEASURED:.2e}); the bar: {BC.TOL:.2e}")
    assert BC.MEASURED / 2 <= worst <= 2 * BC.MEASURED
    assert BC.TOL == max(1e-12, 50 * BC.MEASURED)


def test_the_nonspd_replica_raises_in_the_model_and_its_neighbour_does_not():
    pb, cs = BC.nonspd()
    with pytest.raises(np.linalg.LinAlgError):
        BC.run_model(pb, 0, cs)
    assert all(np.all(np.isfinite(BC.run_model(pb, 1, cs)[k])) for k in BC.KEYS)


# ---- the draw protocol
@pytest.mark.parametrize("r,df", ((2, 7), (10, 4403), (16, 49)))
def test_bartlett_factor_is_scipy_s_wishart_draw(r, df):
    """C A A^T C^T on draw_bpmf's Bartlett factor is scipy.stats.wishart.rvs(df, scale) from the same seed, and the RNG is left in
    the same state"""
    wishart = pytest.importorskip("scipy.stats").wishart
    from rpsmf_amd.bpmf import _bartlett

    rng = np.random.default_rng(r)
    G = rng.standard_normal((r, 2 * r))
    scale = G @ G.T / (2 * r)
    keep = np.random.get_state()
    try:
        np.random.seed(1000 + r)
        want = wishart.rvs(df, scale)
        after_scipy = np.random.get_state()
        np.random.seed(1000 + r)
        A = _bartlett(df, r)
        after_ours = np.random.get_state()
    finally:
        np.random.set_state(keep)
    CA = np.dot(np.linalg.cholesky(scale), A)
    assert np.array_equal(np.triu(A, 1), np.zeros((r, r))) and np.all(np.diag(A) > 0)
    assert np.allclose(np.dot(CA, CA.T), want, rtol=1e-13, atol=0)
    assert after_ours[0] == after_scipy[0] and np.array_equal(after_ours[1], after_scipy[1]) and after_ours[2:] == after_scipy[2:]


def test_n_column_normals_are_one_matrix_of_normals():
    n, r = 37, 5
    keep = np.random.get_state()
    try:
        np.random.seed(5)
        one_by_one = np.stack([np.random.randn(r, 1)[:, 0] for _ in range(n)])
        np.random.seed(5)
        at_once = np.random.randn(n, r)
    finally:
        np.random.set_state(keep)
    assert np.array_equal(one_by_one, at_once)


def test_draw_bpmf_follows_the_protocol():
    from rpsmf_amd.bpmf import _bartlett, draw_bpmf

    d, n, r, N, epochs = 3, 7, 4, 11, 2
    keep = np.random.get_state()
    try:
        np.random.seed(8)
        got = draw_bpmf(d, n, r, N, epochs)
        after = np.random.get_state()
        np.random.seed(8)
        perms = [np.random.permutation(N) for _ in range(epochs)]
        for e in range(epochs):
            assert np.array_equal(got["bartlett"][e, 0], _bartlett(r + n, r))
            assert np.array_equal(got["hyper_normals"][e, 0], np.random.randn(r, 1)[:, 0])
            assert np.array_equal(got["bartlett"][e, 1], _bartlett(r + d, r))
            assert np.array_equal(got["hyper_normals"][e, 1], np.random.randn(r, 1)[:, 0])
            for s in range(2):
                assert np.array_equal(got["normals"][e, s, :n], np.random.randn(n, r))
                assert np.array_equal(got["normals"][e, s, n:], np.random.randn(d, r))
        assert all(np.array_equal(p, q) for p, q in zip(got["perms"], perms))
        assert np.array_equal(np.random.get_state()[1], after[1])
    finally:
        np.random.set_state(keep)


def test_model_reproduces_the_stored_answers():
    """error_full of repeats 0-2 of LondonAir_PM25_20_BPMF.json, to 1e-12 relative; the draws are made behind each repeat's inputs and
    the RNG state is put back, as BPMF.py:361-375 does."""
    g = load_golden("impute_kat_bpmf")
    want = g["pm25_20_error_full"]
    worst = 0.0
    for k, dr in enumerate(BC.kat_inputs("pm25", 20, 3)):
        assert (dr["hY"], dr["hC"], dr["hX"]) == tuple(str(g[f"pm25_20_hash_{nm}"][k]) for nm in "YCX"), k
        got = BC.kat_model(dr)
        worst = max(worst, abs(got["Efull"][-1] - want[k]) / abs(want[k]))
    print(f"pm25_20: model against the stored error_full, 3 repeats: {worst:.2e}")
    assert worst <= 1e-12


def test_fixture_hashes_are_those_of_the_existing_fixtures():
    g = load_golden("impute_kat_bpmf")
    for ds, pct in BC.KAT_FILES:
        other = kat_replay.fixture(ds)
        assert g[f"{ds}_{pct}_error_full"].shape == (100,)
        assert kat_replay.json.loads(str(g[f"{ds}_{pct}_params"])) == {"Iter": BC.KAT_EPOCHS, "r": BC.KAT_R}
        for nm in "YCX":
            assert np.array_equal(g[f"{ds}_{pct}_hash_{nm}"], other[f"PSMF_{pct}_hash_{nm}"]), (ds, pct, nm)


# ---- refusals: ValueError with a message that names the limit, before a device (or the library) is looked for
def _small(d=4, n=30, r=2, B=2, seed=3):
    rng = np.random.default_rng(seed)
    Y = 40.0 + rng.standard_normal((d, n))
    M = (rng.random((B, d, n)) < 0.7).astype(np.uint8)
    Mm = ((rng.random((B, d, n)) < 0.5) & (M == 0)).astype(np.uint8)
    return [Y, M, Mm, rng.random((B, d, r)), rng.random((B, r, n))]


def _refusals():
    a = _small()
    yield "shape of M", (a[0], a[1][:, :, :-1], a[2], a[3], a[4]), {}, "inconsistent shapes"
    yield "shape of X0", (a[0], a[1], a[2], a[3], a[4][:, :, :-1]), {}, "inconsistent shapes"
    yield "rank mismatch", (a[0], a[1], a[2], a[3][:, :, :1], a[4]), {}, "inconsistent shapes"
    yield "M not 0/1", (a[0], a[1] * 2, a[2], a[3], a[4]), {}, "M must hold 0 and 1"
    yield "Mmiss not 0/1", (a[0], a[1], a[2] * 0.5, a[3], a[4]), {}, "Mmiss must hold 0 and 1"
    few = a[1].copy()
    few[1] = 0
    few[1, 0, :5] = 1
    yield "N < num_batches", (a[0], few, a[2], a[3], a[4]), {}, "fewer than num_batches = 9"
    yield "no probe entry", (a[0], a[1], a[2] * np.array([1, 0], dtype=np.uint8)[:, None, None], a[3], a[4]), {}, "no probe entry"
    z = a[0].copy()
    z[:] = np.where(np.arange(z.size).reshape(z.shape) % 2, 1.0, -1.0)
    full = np.ones_like(a[1])
    probe = np.zeros_like(a[2])
    probe[:, 0, 0] = 1
    yield "mu == 0", (z, full, probe, a[3], a[4]), {}, "divided by it"
    yield "d > 512", tuple(_small(d=513, n=12, r=2, B=1)), {}, "d <= 512"
    yield "r > 16", tuple(_small(d=4, n=30, r=17, B=1)), {}, "r <= 16"
    yield "d < 2", tuple(_small(d=1, n=30, r=2, B=1)), {}, "d >= 2 and n >= 2"
    yield "n < 2", tuple(_small(d=4, n=1, r=2, B=1)), {}, "d >= 2 and n >= 2"
    yield "r < 2", tuple(_small(d=4, n=30, r=1, B=1)), {}, "r >= 2"
    yield "epochs = 0", tuple(a), dict(epochs=0), "epochs must be >= 1"
    yield "warm_start keyword", tuple(a), dict(warm_start=dict(rate=1)), "warm_start takes the keywords"
    yield "draws of another length", tuple(a) + ([],), {}, "one record per replica"
    yield "draws without a key", tuple(a) + ([dict(perms=[]), dict(perms=[])],), {}, "must be a dict with the keys"
    from rpsmf_amd.bpmf import draw_bpmf

    keep = np.random.get_state()
    wrong = [draw_bpmf(4, 30, 2, int(a[1][b].sum()), 2) for b in range(2)]
    np.random.set_state(keep)
    wrong[1]["normals"] = wrong[1]["normals"][:, :, :-1]
    yield "draws of another shape", tuple(a) + (wrong,), {}, "draws[1]['normals'] must have the shape (2, 2, 34, 2)"


@pytest.mark.parametrize("what,args,kwargs,message", list(_refusals()), ids=[r[0] for r in _refusals()])
def test_refusals_come_before_the_device(monkeypatch, what, args, kwargs, message):
    from rpsmf_amd import _capi, bpmf

    def no_library():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_capi, "load_library", no_library)
    before = [np.array(x, copy=True) for x in args[:5]]
    with pytest.raises(ValueError, match=re.escape(message)):
        bpmf.bpmf_batch(*args, **kwargs)
    assert all(np.array_equal(x, y) for x, y in zip(args[:5], before))


def test_bpmf_refuses_a_Y_that_is_not_the_masked_data(monkeypatch):
    from rpsmf_amd import _capi, bpmf

    monkeypatch.setattr(_capi, "load_library", lambda: (_ for _ in ()).throw(AssertionError("loaded")))
    Y, M, Mm, C0, X0 = _small(B=1)
    with pytest.raises(ValueError, match="Y == YorigInt"):
        bpmf.bpmf(Y + 1.0, C0[0], X0[0], 4, 30, 2, M[0], Mm[0], Y, 1.0, epochs=2)


def test_signature_of_bpmf_is_the_reference_s():
    import rpsmf_amd
    from rpsmf_amd import bpmf

    sig = inspect.signature(bpmf.bpmf)
    assert tuple(sig.parameters) == REFERENCE_PARAMETERS
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == REFERENCE_DEFAULTS
    kw = inspect.signature(bpmf.bpmf_batch).parameters
    assert [k for k, p in kw.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["epochs", "beta", "device", "want_rec", "warm_start"]
    assert list(kw)[:6] == ["YorgInt", "M", "Mmiss", "C0", "X0", "draws"] and kw["draws"].default is None
    assert (kw["epochs"].default, kw["beta"].default, kw["device"].default, kw["want_rec"].default, kw["warm_start"].default) == (2, 2, 0, False, None)
    assert tuple(inspect.signature(bpmf.draw_bpmf).parameters) == ("d", "n", "r", "N", "epochs")
    assert "from rpsmf_amd.bpmf import bpmf, bpmf_batch, draw_bpmf" in rpsmf_amd.__doc__ and bpmf.__all__ == ["bpmf_batch", "bpmf", "draw_bpmf"]
    assert "LinAlgError" in bpmf.__doc__ and "simple fit" in bpmf.__doc__, "the module says what the port cannot raise"


# ---- the native unit: the rules tests/test_native_batch.py enforces for the other entry points, by its helpers
def test_the_unit_is_built_and_bound():
    from rpsmf_amd import _capi, build

    assert UNIT in build.UNITS
    assert "psmf_bpmf_run" in _capi.SIGNATURES and _capi.ABI_VERSION == 3, "the entry point is additive: the ABI version stays"


def test_the_unit_obeys_the_scaffold_rules():
    host = _host_part(UNIT)
    assert "__global__" not in host and 'extern "C"' in host and "EntryFail" in host
    assert "int bpmf_run(" in host and "psmf_bpmf_metric_kernel(BpmfParams p)" not in host
    assert f'#include "{BATCH}"' in _read(UNIT)
    for call in SCAFFOLD_CALLS:
        assert call not in host, f"{UNIT}: {call} outside {BATCH}"
    by_hand = [m.group(0).strip() for m in re.finditer(r"[^;{}\n]*\*\s*[48]\b[^;\n]*", host)]
    assert not by_hand, f"{UNIT}: an element size written by hand: {by_hand}"
    assert not re.search(r"\bstruct\s+(\w*)\s*\{[^}]*operator\(\)", host), "the failure functor is EntryFail"
    assert "g_create_error" not in host
    for helper in ("open_device(", "slot(", "alloc_all(", "copy_in_all(", "timed.create(", "timed.start(", "timed.finish(", "replica_status("):
        assert helper in host, helper


def test_no_atomics_no_graphs_no_flags_no_generator_in_the_unit():
    text = _read(UNIT)
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("atomic", "hipGraph", "hipStream", "__threadfence", "rocrand", "hiprand", "philox", "curand"):
        assert word not in code, word
    assert code.count("volatile") == code.count('asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")') == 1, "the one wave-local LDS fence"
    assert code.count("__builtin_amdgcn_mfma_f64_16x16x4f64") >= 5, "the two Grams of a sweep with their right-hand sides, and the covariance of W"
