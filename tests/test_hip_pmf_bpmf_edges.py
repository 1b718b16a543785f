"""The entry checks of psmf_pmf_run and psmf_bpmf_run, called through ctypes (rpsmf_amd._capi) past the Python wrappers, which refuse
the same things first: a regression in the library's own checks would be an out-of-bounds launch for a C caller.  Every call has
valid arguments except for one fault; it returns PSMF_ERR_ARG, psmf_last_error names the limit, and P, W, Efull and status keep the
sentinel they were filled with.  These refusals come before the device is opened.  The buffers are sized for the largest shape a
fault names, so that a check that failed to refuse would still read and write inside them."""

import ctypes as C

import numpy as np
import pytest

from netlib import env

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
D, N, R, B, EPOCHS, NB = 6, 5, 3, 2, 2, 2                # the valid shape
D_MAX, N_MAX, R_MAX, NB_MAX = 513, 5, 17, 255            # what the buffers are sized for


def _common():
    from rpsmf_amd import _capi

    rng = np.random.default_rng(3)
    a = dict(Y=40.0 + rng.standard_normal((N_MAX, D_MAX)), M=np.ones((B, N_MAX, D_MAX), dtype=np.uint8), Mmiss=np.ones((B, N_MAX, D_MAX), dtype=np.uint8),
             mean=np.full(B, 40.0), mbar=np.zeros(B), P=np.full((B, D_MAX, R_MAX), SENTINEL), W=np.full((B, N_MAX, R_MAX), SENTINEL),
             Efull=np.full((B, EPOCHS), SENTINEL), Yrec=np.zeros((B, N_MAX, D_MAX)), status=np.full(B, 12345, dtype=np.int32))
    return _capi, a


def _untouched(a):
    return (np.all(a["P"] == SENTINEL) and np.all(a["W"] == SENTINEL) and np.all(a["Efull"] == SENTINEL) and np.all(a["status"] == 12345))


def _pmf(cfg=None, null_rec=False, **arrays):
    """(return code, last error, the buffers were left alone) of one psmf_pmf_run"""
    _capi, a = _common()
    a.update(maps=np.zeros((B, EPOCHS, N_MAX, D_MAX), dtype=np.uint8), sizes=np.full(B * NB_MAX, 7, dtype=np.int32),
             counts=np.ones((B, EPOCHS, NB_MAX, D_MAX), dtype=np.int32))
    a.update(arrays)
    kw = dict(abi_version=_capi.ABI_VERSION, d=D, n=N, r=R, batch=B, epochs=EPOCHS, num_batches=NB, device=0, want_rec=0, epsilon=2.0, lmd=0.01, momentum=0.8)
    kw.update(cfg or {})
    lib, ptr = _capi.load_library(), _capi._ptr
    ms = C.c_float()
    rc = lib.psmf_pmf_run(C.byref(_capi.PsmfPmfConfig(**kw)), ptr(a["Y"]), ptr(a["maps"]), ptr(a["Mmiss"]), ptr(a["sizes"]), ptr(a["counts"]), ptr(a["mean"]),
                          ptr(a["mbar"]), ptr(a["P"]), ptr(a["W"]), ptr(a["Efull"]), None if null_rec else ptr(a["Yrec"]), ptr(a["status"]), C.byref(ms))
    return rc, lib.psmf_last_error(None).decode(), _untouched(a)


def _bpmf(cfg=None, null_rec=False, **arrays):
    """(return code, last error, the buffers were left alone) of one psmf_bpmf_run"""
    _capi, a = _common()
    a.update(bart=np.ones((B, EPOCHS, 2, R_MAX, R_MAX)), hz=np.zeros((B, EPOCHS, 2, R_MAX)), Z=np.zeros((B, EPOCHS, 2, N_MAX + D_MAX, R_MAX)))
    a.update(arrays)
    kw = dict(abi_version=_capi.ABI_VERSION, d=D, n=N, r=R, batch=B, epochs=EPOCHS, device=0, want_rec=0, beta=2.0)
    kw.update(cfg or {})
    lib, ptr = _capi.load_library(), _capi._ptr
    ms = C.c_float()
    rc = lib.psmf_bpmf_run(C.byref(_capi.PsmfBpmfConfig(**kw)), ptr(a["Y"]), ptr(a["M"]), ptr(a["Mmiss"]), ptr(a["mean"]), ptr(a["mbar"]), ptr(a["bart"]),
                           ptr(a["hz"]), ptr(a["Z"]), ptr(a["P"]), ptr(a["W"]), ptr(a["Efull"]), None if null_rec else ptr(a["Yrec"]), ptr(a["status"]),
                           C.byref(ms))
    return rc, lib.psmf_last_error(None).decode(), _untouched(a)


def _sizes_with_a_zero():
    s = np.full(B * NB_MAX, 7, dtype=np.int32)
    s[1 * NB + 1] = 0          # batch 1 of replica 1 in the (B, NB) array the library reads from the front of the buffer
    return s


# (what, keywords of _pmf / _bpmf, the environment, what the last error must name)
PMF_FAULTS = (
    ("d=513", dict(cfg=dict(d=513)), {}, "d <= 512"),
    ("r=17", dict(cfg=dict(r=17)), {}, "r <= 16"),
    ("r=0", dict(cfg=dict(r=0)), {}, "1 <= r"),
    ("num_batches=0", dict(cfg=dict(num_batches=0)), {}, "num_batches <= 254"),
    ("num_batches=255", dict(cfg=dict(num_batches=255)), {}, "num_batches <= 254"),
    ("batch_sizes entry 0", dict(sizes=_sizes_with_a_zero()), {}, "empty batch"),
    ("mean=0", dict(mean=np.array([40.0, 0.0])), {}, "mean"),
    ("mean=NaN", dict(mean=np.array([40.0, np.nan])), {}, "mean"),
    ("want_rec, Yrec=NULL", dict(cfg=dict(want_rec=1), null_rec=True), {}, "Yrec"),
    ("epochs=0", dict(cfg=dict(epochs=0)), {}, "epochs >= 1"),
    ("abi_version", dict(cfg=dict(abi_version=10 ** 6)), {}, "ABI version"),
    ("PSMF_PMF_COLS=-1", {}, {"PSMF_PMF_COLS": "-1"}, "PSMF_PMF_COLS"),
)
BPMF_FAULTS = (
    ("d=513", dict(cfg=dict(d=513)), {}, "d <= 512"),
    ("r=17", dict(cfg=dict(r=17)), {}, "r <= 16"),
    ("r=0", dict(cfg=dict(r=0)), {}, "2 <= r"),
    ("d=1", dict(cfg=dict(d=1)), {}, "2 <= d"),
    ("r=1", dict(cfg=dict(r=1)), {}, "2 <= r"),
    ("n=1", dict(cfg=dict(n=1)), {}, "n >= 2"),
    ("mean=0", dict(mean=np.array([40.0, 0.0])), {}, "mean"),
    ("mean=NaN", dict(mean=np.array([40.0, np.nan])), {}, "mean"),
    ("want_rec, Yrec=NULL", dict(cfg=dict(want_rec=1), null_rec=True), {}, "Yrec"),
    ("epochs=0", dict(cfg=dict(epochs=0)), {}, "epochs >= 1"),
    ("abi_version", dict(cfg=dict(abi_version=10 ** 6)), {}, "ABI version"),
    ("PSMF_BPMF_CHUNK=-1", {}, {"PSMF_BPMF_CHUNK": "-1"}, "PSMF_BPMF_CHUNK"),
)


@pytest.mark.parametrize("what,kw,envv,names", PMF_FAULTS, ids=[f[0] for f in PMF_FAULTS])
def test_psmf_pmf_run_refuses(what, kw, envv, names):
    from rpsmf_amd._capi import ERR_ARG

    with env(envv):
        rc, msg, untouched = _pmf(**kw)
    print(f"\npsmf_pmf_run, {what}: {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith("psmf_pmf_run") and names in msg, (rc, msg)
    assert untouched, "P, W, Efull and status keep their sentinel"


@pytest.mark.parametrize("what,kw,envv,names", BPMF_FAULTS, ids=[f[0] for f in BPMF_FAULTS])
def test_psmf_bpmf_run_refuses(what, kw, envv, names):
    from rpsmf_amd._capi import ERR_ARG

    with env(envv):
        rc, msg, untouched = _bpmf(**kw)
    print(f"\npsmf_bpmf_run, {what}: {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith("psmf_bpmf_run") and names in msg, (rc, msg)
    assert untouched, "P, W, Efull and status keep their sentinel"
