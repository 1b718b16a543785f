"""The cases of the series-ring tests (tests/test_hip_series_ring.py on the GPU, tests/test_series_ring_cpu.py without one): one
per engine path that can read the series through a ring window, the inputs of each, and the float64 oracle over the whole stream.
Streams of 7 chunks, the last one short; chunks of 37 and 100 rows -- one below and one above a block of the blocked engine
(min(64 - r, 48) steps), neither a multiple of it -- in rings of 2 and 3 slots; d = 1 and d = 257.

`kernel` is what psmf_filter_kernel must report (select_filter_kernel).  The random walk with Q = q I at r = 5 goes to
psmf_blk_filter6d (r <= 16: the small-rank kernel takes it), so psmf_blk_filter3 has a case of its own at r = 20.

Bars against the oracle: float64 storage 1e-9, float32 storage 1e-5 (conftest.relerr).  The cases with device-evaluated dynamics
store float64: with float32 storage the oracle's own response to the rounding of the inputs is 1e-6 .. 1e-5 over these horizons.
`sensitivity` is the oracle's own response to what the number formats force on any engine, and the CPU test keeps it 16 x inside
the bar: a relative 2^-50 (float32 storage: 2^-23) change of the inputs, and, with float32 storage, the rounding of C to float32
where the engine writes it (the blocked engine once per block of B steps, the per-step engine once per step).  The second
is what rules out d = 1 at r = 20 with float32 storage: one observation per step leaves nineteen directions of the mean that no
later step pulls back, and the oracle itself, with nothing but C rounded once per block, is 1e-6 off in the mean history (5.8e-5
rounded once per step) -- so psmf_blk_filter3, which float32 storage alone reaches, runs d = 257, and the blocked engine's d = 1
case is the float64 psmf_blk_filter7 one at the same rank."""

import numpy as np

import blocked_cases as BC
from oracle import psmf_oracle as O

N_CHUNKS = 7

ADAM_LR = 1e-4       # the recursive case: 242 steps of 1e-3 carry theta (0.1 * rand) onto the projection's kink at 0, where the oracle
                     # itself answers a last-bit change of the inputs with 1e-8 .. 1e-4; at 1e-4 with 1e-12


def _case(name, kernel, d, r, chunk, n_slots, storage, engine, dyn="random_walk", robust=False, recursive=0, masked=False, nonuniform=False, seed=0):
    T = (N_CHUNKS - 1) * chunk + chunk // 2 + 2          # the last chunk is short
    return dict(name=name, kernel=kernel, d=d, r=r, chunk=chunk, n_slots=n_slots, storage=storage, engine=engine, dyn=dyn, robust=robust,
                recursive=recursive, masked=masked, nonuniform=nonuniform, T=T, seed=1000 + seed,
                # what blocked_cases.problem reads; V0 = v I as blocked_cases draws it: every entry of a float32 series carries its
                # own last-bit error and C sums their effect over the steps, so float32 storage takes the stiffer prior
                general_Q=False, sched=False, v0=0.02 if storage == "f32" else 0.1)


CASES = [
    _case("block r=5 random walk", "psmf_blk_filter6d", 257, 5, 37, 2, "f32", "block", seed=1),
    _case("block filter3", "psmf_blk_filter3", 257, 20, 100, 3, "f32", "block", seed=2),
    _case("block filter6 cos-phase", "psmf_blk_filter6", 257, 6, 37, 3, "f64", "block", dyn="cos_phase", seed=3),
    _case("block filter7 scaled walk", "psmf_blk_filter7", 1, 20, 37, 2, "f64", "block", dyn="scaled_walk", seed=4),
    _case("step persistent PSMF", "psmf_pstep_k", 257, 8, 100, 2, "f64", "step", seed=5),
    _case("step persistent rPSMF", "psmf_pstep_k", 257, 8, 37, 3, "f64", "step", robust=True, seed=6),
    _case("step launched row noise", "psmf_sweep_solve", 1, 9, 37, 2, "f64", "step", nonuniform=True, seed=7),
    _case("masked persistent", "psmf_pstep_k", 257, 8, 37, 3, "f64", "step", masked=True, seed=8),
    _case("masked launched", "psmf_sweep_solve", 257, 40, 37, 2, "f64", "step", masked=True, seed=9),
    _case("recursive cos-phase", "psmf_blk_filter6", 257, 6, 37, 2, "f64", "block", dyn="cos_phase", recursive=1, seed=10),
]
IDS = [c["name"] for c in CASES]

# the launched per-step engine replays a captured graph from 256 steps on: chunks of 260 steps, so that every chunk captures anew
GRAPH_CASE = _case("step launched, graph per chunk", "psmf_sweep_solve", 257, 9, 260, 2, "f64", "step", nonuniform=True, seed=11)


def bar(cs):
    return 1e-5 if cs["storage"] == "f32" else 1e-9


def spans(cs):
    """(k_begin, k_end) of the chunks of the stream"""
    return [(a, min(a + cs["chunk"], cs["T"])) for a in range(0, cs["T"], cs["chunk"])]


def problem(cs, perturb=None):
    """Y (T, d) time-major, C0, V0, P0, Q, mu0, theta, rho, lam, the dynamics object; masked: M (T, d); nonuniform: rho_rows (d)."""
    if not cs["masked"]:
        pb = BC.problem(cs, perturb)
        if cs["nonuniform"]:
            pb["rho_rows"] = 0.3 + 2.0 * np.random.default_rng(cs["seed"] ^ 0xD1A6).random(cs["d"])
        return pb
    d, r, T = cs["d"], cs["r"], cs["T"]
    rng = np.random.default_rng(cs["seed"])
    Y = (np.cumsum(0.3 * rng.standard_normal((d, T)), axis=1) + 3.0 * rng.random((d, 1))).T.copy()
    M = (rng.random((T, d)) > 0.4).astype(np.uint8)
    M[1] = 0                      # a step without any observation
    M[:, 3] = 0                   # a row that is never observed
    M[cs["chunk"]] = 1            # the first step of the second chunk: fully observed, unlike its neighbours
    C0, mu0 = rng.random((d, r)), rng.random(r)
    if perturb is not None:
        prng = np.random.default_rng(perturb[0])
        Y = Y * (1.0 + perturb[1] * prng.uniform(-1, 1, Y.shape))
        C0 = C0 * (1.0 + perturb[1] * prng.uniform(-1, 1, C0.shape))
    return dict(nl=BC._nl("random_walk", r), Y=Y, M=M, C0=C0, V0=2 * np.eye(r), P0=np.eye(r), Q=0.1 * np.eye(r), mu0=mu0, theta=np.zeros(0),
                rho=10.0, lam=1.8)


def reference(cs, pb, round_C_every=0):
    """The oracle over the whole stream: final state, y_pred (T, d), the mean history (T + 1, r), (s, eta) of every step (T, 2).
    `round_C_every` = n > 0 rounds C to float32 after every n-th step: the least a handle that stores float32 does."""
    dyn = BC.dynamics_of(pb)
    n_theta = dyn.n_theta
    T = cs["T"]
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(),
                 rho=pb["rho_rows"].copy() if cs["nonuniform"] else pb["rho"], lam=pb["lam"], theta=pb["theta"].copy(), gradsum=np.zeros(n_theta))
    mode = O.Mode(robust=cs["robust"])
    Yp, mu, sc = np.empty((T, cs["d"])), np.empty((T + 1, cs["r"])), np.empty((T, 2))
    mu[0] = st.mu
    m = v = np.zeros(n_theta)
    for k in range(1, T + 1):
        st, info = O.lowrank_step(st, pb["Y"][k - 1], k, mode, dyn, mask=pb["M"][k - 1] if cs["masked"] else None, want_grad=n_theta > 0)
        Yp[k - 1], mu[k], sc[k - 1] = info.y_pred, st.mu, (info.s, info.eta)
        if round_C_every and k % round_C_every == 0:
            st.C = st.C.astype(np.float32).astype(np.float64)
        if cs["recursive"]:               # psmf.py:299-304, update_every = 1
            st.theta, m, v = O.adam_update(st.theta, st.gradsum, m, v, k, lr=ADAM_LR)
            st.gradsum = np.zeros(n_theta)
    return dict(C=st.C, V=st.V, P=st.P, Q=np.array(st.Q, dtype=float), mu=st.mu, theta=st.theta, gradsum=st.gradsum, rho=st.rho, lam=st.lam,
                y_pred=Yp, mu_hist=mu, sc=sc)


COMPARED = ("C", "V", "P", "mu", "y_pred", "mu_hist")


def sensitivity(cs):
    """(to the inputs' last bit, to float32 storage of C); the second is 0 with float64 storage"""
    f32 = cs["storage"] == "f32"
    a = reference(cs, problem(cs))
    b = reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, 2.0 ** -23 if f32 else 2.0 ** -50)))
    for k in COMPARED:
        if not np.all(np.isfinite(a[k])):
            raise FloatingPointError(f"{cs['name']}: non-finite {k} in the oracle")
    inputs = max(BC.relerr(b[k], a[k]) for k in COMPARED)
    if not f32:
        return inputs, 0.0
    c = reference(cs, problem(cs), round_C_every=BC.block_steps(cs["r"]) if cs["engine"] == "block" else 1)
    return inputs, max(BC.relerr(c[k], a[k]) for k in COMPARED)
