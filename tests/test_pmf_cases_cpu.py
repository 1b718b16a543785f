"""The PMF baseline without a GPU: the case list of tests/pmf_cases.py is admitted whole, the numpy model of tests/pmf_model.py reproduces
the reference's stored answers, the fixture belongs to the inputs the other known-answer fixtures hold, rpsmf_amd.pmf refuses what it
documents before it looks for a device, pmf() has the reference's parameter list, and psmf_pmf.hip stands on the host scaffold as the
other entry points without a handle do (the rules of tests/test_native_batch.py, through its helpers)."""

import inspect
import re

import numpy as np
import pytest

import kat_replay
import pmf_cases as PC
import pmf_model
from conftest import load_golden
from test_native_batch import BATCH, SCAFFOLD_CALLS, _host_part, _read

UNIT = "psmf_pmf.hip"
# ExperimentImpute/PMF.py:43-59
REFERENCE_PARAMETERS = ("Y", "C", "X", "num_p", "num_m", "num_feat", "M", "Mmiss", "YorigInt", "Einit", "epochs", "epsilon", "lmd", "momentum",
                        "num_batches")
REFERENCE_DEFAULTS = dict(epochs=50, epsilon=50, lmd=0.01, momentum=0.8, num_batches=9)


@pytest.mark.parametrize("i", range(len(PC.CASES)), ids=[c["name"] for c in PC.CASES])
def test_every_case_is_admitted(i):
    ok, text = PC.admission(i)
    print(text)
    assert ok, text


def test_the_list_is_the_issue_s_and_covers_what_it_says():
    assert [(c["d"], c["n"], c["r"], c["nb"], c["epochs"], c["batch"]) for c in PC.CASES[:8]] == [
        (1, 40, 1, 1, 1, 1), (3, 23, 2, 4, 2, 2), (19, 700, 10, 9, 2, 3), (27, 257, 10, 9, 2, 2), (80, 130, 16, 9, 3, 2), (505, 96, 10, 9, 2, 2),
        (512, 33, 16, 5, 1, 1), (17, 3000, 5, 9, 2, 4)]
    assert {c["d"] for c in PC.CASES[8:]} == {200}, "beyond the issue's eight: the instance none of them reaches"
    assert all(c["epsilon"] == 50 for c in PC.CASES if c["d"] != 3), "only the tiny shape runs at a small epsilon"
    both = 0
    for c in PC.CASES:
        pb = PC.problem(c["i"])
        Ns = [int(m.sum()) for m in pb["M"]]
        assert len(set(Ns)) == len(Ns), (c["name"], Ns)
        if c["nb"] > 1:
            assert all(N % c["nb"] for N in Ns), (c["name"], Ns)
        for b in range(c["batch"]):
            M, Mm = pb["M"][b] != 0, pb["Mmiss"][b] != 0
            assert Mm.any()
            if c["n"] > 5:
                assert np.any(~M.any(axis=0) & Mm.any(axis=0)), f"{c['name']}: a column without a training entry but with a probe entry"
            if c["d"] > 2:
                assert np.any(~M.any(axis=1)), f"{c['name']}: a row without a training entry"
            both += int(np.any(M & Mm))
        for arr in (pb["M"], pb["Mmiss"]):
            assert set(np.unique(arr)) <= {0, 1}
    assert both == 1, "one replica has a probe entry that is also a training entry"


def test_the_diverging_replica_diverges_in_the_model_and_its_neighbour_does_not():
    pb, cs, ref = PC.diverging()
    assert not np.all(np.isfinite(ref[0]["Efull"])) or not np.all(np.isfinite(ref[0]["W"])) or not np.all(np.isfinite(ref[0]["P"]))
    assert all(np.all(np.isfinite(ref[1][k])) for k in PC.KEYS)


@pytest.mark.parametrize("ds,pct", PC.KAT_FILES, ids=[f"{ds}_{pct}" for ds, pct in PC.KAT_FILES])
def test_model_reproduces_the_stored_answers(ds, pct):
    """error_full of the first 10 repeats of <ds>_<pct>_PMF.json, to 1e-12 relative; the permutations are drawn behind each repeat's
    inputs and the RNG state is put back, as PMF.py:218-224 does."""
    g = load_golden("impute_kat_pmf")
    want = g[f"{ds}_{pct}_error_full"]
    worst = 0.0
    for k, dr in enumerate(PC.kat_inputs(ds, pct, 10)):
        assert (dr["hY"], dr["hC"], dr["hX"]) == tuple(str(g[f"{ds}_{pct}_hash_{nm}"][k]) for nm in "YCX"), (ds, pct, k)
        got = pmf_model.pmf_model(dr["YorigInt"], dr["M"], dr["Mmiss"], dr["C"], dr["X"], dr["perms"], epochs=PC.KAT_EPOCHS)
        worst = max(worst, abs(got["Efull"][-1] - want[k]) / abs(want[k]))
    print(f"{ds}_{pct}: model against the stored error_full, 10 repeats: {worst:.2e}")
    assert worst <= 1e-12


def test_fixture_hashes_are_those_of_the_existing_fixtures():
    g = load_golden("impute_kat_pmf")
    for ds, pct in PC.KAT_FILES:
        other = kat_replay.fixture(ds)
        assert g[f"{ds}_{pct}_error_full"].shape == (100,)
        assert kat_replay.json.loads(str(g[f"{ds}_{pct}_params"])) == {"Iter": PC.KAT_EPOCHS, "r": PC.KAT_R}
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
    yield "num_batches = 0", tuple(a), dict(num_batches=0), "num_batches must be 1 .. 254"
    yield "num_batches = 255", tuple(a), dict(num_batches=255), "num_batches must be 1 .. 254"
    big = _small(d=513, n=12, r=2, B=1)
    yield "d > 512", tuple(big), {}, "d <= 512"
    wide = _small(d=4, n=30, r=17, B=1)
    yield "r > 16", tuple(wide), {}, "r <= 16"


@pytest.mark.parametrize("what,args,kwargs,message", list(_refusals()), ids=[r[0] for r in _refusals()])
def test_refusals_come_before_the_device(monkeypatch, what, args, kwargs, message):
    from rpsmf_amd import _capi, pmf

    def no_library():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_capi, "load_library", no_library)
    before = [np.array(x, copy=True) for x in args]
    with pytest.raises(ValueError, match=re.escape(message)):
        pmf.pmf_batch(*args, **kwargs)
    assert all(np.array_equal(x, y) for x, y in zip(args, before))


def test_pmf_refuses_a_Y_that_is_not_the_masked_data(monkeypatch):
    from rpsmf_amd import _capi, pmf

    monkeypatch.setattr(_capi, "load_library", lambda: (_ for _ in ()).throw(AssertionError("loaded")))
    Y, M, Mm, C0, X0 = _small(B=1)
    with pytest.raises(ValueError, match="Y == YorigInt"):
        pmf.pmf(Y + 1.0, C0[0], X0[0], 4, 30, 2, M[0], Mm[0], Y, 1.0, epochs=2)


def test_signature_of_pmf_is_the_reference_s():
    from rpsmf_amd import pmf

    sig = inspect.signature(pmf.pmf)
    assert tuple(sig.parameters) == REFERENCE_PARAMETERS
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == REFERENCE_DEFAULTS
    kw = inspect.signature(pmf.pmf_batch).parameters
    assert [k for k, p in kw.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["epochs", "epsilon", "lmd", "momentum", "num_batches", "device", "want_rec"]
    assert list(kw)[:6] == ["YorgInt", "M", "Mmiss", "C0", "X0", "perms"] and kw["perms"].default is None
    assert (kw["epochs"].default, kw["epsilon"].default, kw["lmd"].default, kw["momentum"].default, kw["num_batches"].default) == (2, 50, 0.01, 0.8, 9)


def test_batch_sizes_are_array_split_s():
    from rpsmf_amd.pmf import _batch_sizes

    for N, nb in ((23, 1), (29, 4), (9041, 9), (254, 254), (1000, 7)):
        assert list(_batch_sizes(N, nb)) == [len(x) for x in np.array_split(np.arange(N), nb)]


# ---- the native unit: the rules tests/test_native_batch.py enforces for the other three, by its helpers
def test_the_unit_is_built_and_bound():
    from rpsmf_amd import _capi, build

    assert UNIT in build.UNITS
    assert "psmf_pmf_run" in _capi.SIGNATURES and _capi.ABI_VERSION == 3, "the entry point is additive: the ABI version stays"


def test_the_unit_obeys_the_scaffold_rules():
    host = _host_part(UNIT)
    assert "__global__" not in host and 'extern "C"' in host and "EntryFail" in host
    assert "int pmf_run(" in host and "psmf_pmf_metric_kernel(PmfParams p)" not in host
    assert f'#include "{BATCH}"' in _read(UNIT)
    for call in SCAFFOLD_CALLS:
        assert call not in host, f"{UNIT}: {call} outside {BATCH}"
    by_hand = [m.group(0).strip() for m in re.finditer(r"[^;{}\n]*\*\s*[48]\b[^;\n]*", host)]
    assert not by_hand, f"{UNIT}: an element size written by hand: {by_hand}"
    assert not re.search(r"\bstruct\s+(\w*)\s*\{[^}]*operator\(\)", host), "the failure functor is EntryFail"
    assert "g_create_error" not in host
    for helper in ("open_device(", "slot(", "alloc_all(", "copy_in_all(", "timed.create(", "timed.start(", "timed.finish(", "replica_status("):
        assert helper in host, helper


def test_no_atomics_no_graphs_no_flags_in_the_unit():
    text = _read(UNIT)
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("atomic", "hipGraph", "hipStream", "__threadfence", "volatile"):
        assert word not in code, word
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in code
