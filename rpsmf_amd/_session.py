"""The device handle a filter object (psmf.py) currently has: which kind it is, what is resident on it, and the one way it goes.

A handle's kind is fixed when it is created (include/psmf_hip.h: `masked`, the engine, a series ring cannot be taken off again), so an
epoch that needs another kind replaces the handle.  `DeviceSession.ensure(kind)` is where that is decided and `drop()` the only place the
classes close a handle: it first brings a device-resident C to the host, so the next handle can be given it."""

from typing import NamedTuple, Optional, Tuple

import numpy as np


def _content_hash(a):
    try:
        from xxhash import xxh3_128_hexdigest
    except ImportError:
        import hashlib

        return hashlib.blake2b(a.data, digest_size=16).hexdigest()
    return xxh3_128_hexdigest(a.data)


class _Lazy:
    """A value that lives on the device until somebody asks for it: the C that the session `owner` left there in its epoch `epoch`."""

    def __init__(self, owner, epoch):
        self.owner, self.epoch = owner, epoch

    def fetch(self):
        return self.owner.fetch_C(self.epoch)


class _StateDict(dict):
    """dict k -> array whose values may be device-resident (_Lazy) until first read."""

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if isinstance(v, _Lazy):
            v = v.fetch()
            dict.__setitem__(self, k, v)
        return v

    def raw(self, k):
        return dict.__getitem__(self, k)


class Kind(NamedTuple):
    """What cannot change on a live handle."""
    masked: bool = False                            # cfg.masked = PSMF_MASKED_DYNAMICS, per-step engine
    ring: Optional[Tuple[int, int]] = None          # series ring (chunk, n_slots) of step_stream; None: resident series buffers
    q_matrices: bool = False                        # Q[k] uploaded matrix by matrix (psmf_set_q_matrix_schedule): per-step engine
    host_forced: bool = False                       # host-stepped although f is a device kind (a Q[k] schedule too large to upload)


def _time_major(y, T, d, what, rows):
    """y[k], k = 1..T -- dict {k: (d, 1)} as in the reference, or any array-like indexed the same way (row 0 unused), exactly what the
    numpy back end reads -- as a (T, d) array."""
    if isinstance(y, dict):
        Y = np.concatenate([np.asarray(y[k]).reshape(1, -1) for k in range(1, T + 1)], axis=0)
    else:
        Y = np.asarray(y)[1:T + 1].reshape(T, -1)
    if Y.shape != (T, d):
        raise ValueError(f"{what}: expected {T} {rows} of length {d}, got an array of shape {Y.shape}")
    return Y


class DeviceSession:
    """`owner`: the filter object; it states the handle's options (`_open_device`) and holds the state dictionaries (`_C`)."""

    def __init__(self, owner):
        self.owner = owner
        self.dev = None                 # no handle until the first device epoch
        self.kind = Kind()              # of `dev`, or of the handle the next ensure() creates
        self.epoch = 0                  # counts pull_state(): a _Lazy of an earlier epoch is stale
        self.series_key = self.mask_key = self.qmat_key = None      # content keys of what is resident on `dev`
        self.sched_key = (None, None)

    def drop(self):
        """Close the handle.  A C that is still on it (a _Lazy of the current epoch in the owner's `_C`) is fetched first."""
        if self.dev is not None:
            C = self.owner._C
            for k in [k for k in C if isinstance(C.raw(k), _Lazy) and C.raw(k).owner is self and C.raw(k).epoch == self.epoch]:
                C[k]
            self.dev.close()
        self.dev = None
        self.series_key = self.mask_key = self.qmat_key = None
        self.sched_key = (None, None)

    def ensure(self, kind):
        """The handle of this kind: the one there is, or a new one in place of a handle of another kind."""
        if kind != self.kind:
            self.drop()
            self.kind = kind
        if self.dev is None:
            self.dev = self.owner._open_device(kind.ring)
        return self.dev

    def fetch_C(self, epoch):
        if epoch != self.epoch:
            raise RuntimeError("stale device reference to C (the device state has moved on)")
        return self.dev.get_state(want_C=True)["C"]

    def upload_series(self, y, T, d):
        """y[1..T] onto the device.  The resident copy is reused only if the CONTENT is unchanged (a checksum of the T observations;
        object identity says nothing: ids are recycled and containers are refilled in place)."""
        Y = np.ascontiguousarray(_time_major(y, T, d, "series", "observations"))
        if not self.holds_series(Y, T):
            self.dev.upload_series(Y, t0=0, T_total=T)
            self.series_key = (T, Y.dtype.str, _content_hash(Y))

    def holds_series(self, Y, T):
        """Is the contiguous (T, d) array Y, dtype and all, the series resident on the handle?"""
        return self.series_key == (T, Y.dtype.str, _content_hash(Y))

    def upload_mask(self, mask, T, d):
        """mask[1..T] onto the device behind the series; as upload_series, the resident copy is reused only if the content (and the
        series it belongs to) is unchanged."""
        M = np.ascontiguousarray(_time_major(mask, T, d, "mask", "rows") != 0, dtype=np.uint8)
        key = (self.series_key, _content_hash(M))
        if self.mask_key != key:
            self.dev.upload_mask(M)
            self.mask_key = key

    def push_state(self, C0, V, P, Q, mu, rho, lambda0, theta, rho_s, q_s, Qm):
        """The epoch's starting state and schedules onto the handle.  C0 may be the _Lazy this handle left behind: then C stays where
        it is.  rho_s, q_s: scalar schedules or None (q_s "host": none for the device); Qm: the [T + 1, r, r] stack or None."""
        dev = self.dev
        same_C = isinstance(C0, _Lazy) and C0.owner is self and C0.epoch == self.epoch
        dev.set_state(None if same_C else np.asarray(C0, dtype=float), V, P, Q, mu, rho=rho, lambda0=lambda0,
                      theta=theta if (theta.size and dev.n_theta) else None)
        if isinstance(q_s, str):
            q_s = None
        sched = (None if rho_s is None else tuple(rho_s), None if q_s is None else tuple(q_s))
        if sched != self.sched_key:
            dev.set_schedules(rho_s, q_s)
            self.sched_key = sched
        if Qm is not None:
            key = (Qm.shape, _content_hash(Qm))
            if key != self.qmat_key:
                dev.set_q_matrix_schedule(Qm)
                self.qmat_key = key

    def pull_state(self):
        """(the state after a run without C, the _Lazy that stands for C): C stays on the device until somebody reads it."""
        s = self.dev.get_state(want_C=False)
        self.epoch += 1
        return s, _Lazy(self, self.epoch)
