"""psmf_ssm_run / psmf_ssm_run_ex (rpsmf_amd/ssm.py: linear_psmf_batch; psmf_ssm_kernel<robust, masked>) on configurations drawn at
random (seeded, tests/ssm_net_cases.py): all four kernel instances, batches of two or three DIFFERENT replicas (own Y, C0, x0, mask,
and for every second case own dense V0 and P0), alpha and beta other than 1, r from 1 to 16, p from r to 32, d from 1 to 512 with
the wave and second-row edges, n from 1 to 60, four lambda0, fixed and growing, four rho, three observed fractions and three
structured masks.  The engine's hand-picked tests (test_hip_ssm.py, test_hip_ssm_robust.py) hold almost all of these at one value;
this is the net under them.
Each replica is compared with its own run of the line-for-line float64 model (ssm_robust_cases.literal_model, the d x d S formed and
divided by) at 5e-9 in conftest.relerr, the suite's float64 bar for the one-workgroup engines; tests/test_ssm_net_cases_cpu.py has
shown every case conditioned 500 x below it.  Every third case runs again with want_pred=False: the same bits in everything else.
After every case the caller's arrays are what they were.
GPU only: `pytest -m gpu`; `-s` shows one NET line per case (printed before it asserts) and, at the end, the worst error / bar per
kernel instance."""

import numpy as np
import pytest

import ssm_net_cases as NC
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

WORST = {}          # instance -> (error / bar, quantity, case)


@pytest.mark.parametrize("i", range(NC.N_CASES))
def test_ssm_random_configuration(i):
    from rpsmf_amd.ssm import linear_psmf_batch

    cs, pbs, refs = NC.reference(i)
    args, kw = NC.device_args(cs, pbs), NC.device_kw(cs, pbs)
    named = dict(zip(("Y", "C0", "x0", "V0", "P0", "A", "Q", "H"), args[:8]))
    if "mask" in kw:
        named["mask"] = kw["mask"]
    kept = {k: np.array(v, copy=True) for k, v in named.items()}
    res = linear_psmf_batch(*args, want_pred=True, **kw)
    res2 = linear_psmf_batch(*args, want_pred=False, **kw) if i % 3 == 0 else None
    keys, tol = NC.compared(cs), NC.bar(cs)
    errs = []          # (quantity, replica, error)
    for b, ref in enumerate(refs):
        for k in keys:
            got = res[k][b]
            errs.append((k, b, relerr(got, ref[k]) if got.shape == ref[k].shape and np.all(np.isfinite(got)) else np.inf))
    worst = max(errs, key=lambda e: e[2])
    print(f"\nNET case={i} sub={cs['sub']} {NC.describe(cs)} bar={tol:.0e} worst={worst[0]}@{worst[1]} err={worst[2]:.3e} "
          f"ratio={worst[2] / tol:.3g} status={list(res['status'])}")
    name = NC.instance(cs)
    if name not in WORST or not worst[2] / tol <= WORST[name][0]:
        WORST[name] = (worst[2] / tol, worst[0], i)
    assert list(res["status"]) == [0] * cs["batch"], res["status"]
    assert ("omega" in res) == (name != "plain")
    bad = [e for e in errs if not e[2] <= tol]
    assert not bad, (NC.describe(cs), bad)
    if res2 is not None:
        assert res2["Ypred"] is None and list(res2["status"]) == [0] * cs["batch"]
        for k in keys:
            if k != "Ypred":
                assert np.array_equal(res[k], res2[k]), ("want_pred changes", k)
    for k, v in named.items():
        assert np.array_equal(v, kept[k], equal_nan=True), f"the call modified the caller's {k}"
    for b, pb in enumerate(pbs):          # ... and the replicas the batch was stacked from are what the reference ran on
        assert np.array_equal(np.asarray(args[0])[b], pb["Y"])


def test_worst_error_over_bar_per_instance():
    """The table of the net: worst error / bar over every compared quantity per kernel instance, over the cases that ran before
    this test (all of them in a whole-file run)."""
    print("\nworst error / bar per kernel instance:")
    for name in NC.INSTANCES:
        if name in WORST:
            ratio, what, i = WORST[name]
            print(f"WORST {name:14s} ratio={ratio:.3g} ({what}, case {i})")
    assert all(ratio < 1.0 for ratio, _, _ in WORST.values())
