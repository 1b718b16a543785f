"""Seeded random configurations of the per-step engine (engine = 1 of include/psmf_hip.h) aimed at the persistent kernel
psmf_pstep_k (rpsmf_amd/csrc/psmf_pstep.hip), the problem each one runs and the float64 oracle carried across the same run parts.
Pure Python: tests/test_step_cases_cpu.py checks the list's coverage and the conditioning of every case without a GPU,
tests/test_hip_step_engine_net.py runs the same list on the device.

The kernel has 44 instances: padded rank RPAD = 8, 16, 32 (r <= 8, 16, 32) x NP = 4, 8, 12 row passes x float32 / float64
storage x unmasked / masked, and RPAD = 64 (33 <= r <= 48) x NP = 4, 8, 12, 16 x storage, unmasked.  `plan` restates the host
planner that picks NP and the launch geometry (pstep_plan), `expected_kernel` restates as a table which handles take the
persistent kernel at all (init_pstep, pstep_usable); the device test asserts that the handle reports both.

The planner, in numbers.  A row pass is rpw = 2048 / RPAD rows (512 threads, RPAD / 4 lanes per row); a row workgroup runs NP
passes, so it holds NP x rpw rows; there are at most n_cu - 1 row workgroups (one compute unit is the hub's), and no more than
the hub's fan-in sums: 17 partial rows per segment and min(24, 256 / ceil((r + 1) / 2)) segments -- at least 255 for every
r <= 32 -- and at RPAD = 64 20 rows per segment, at most 12 segments: 240 workgroups for r <= 41, 220 for r <= 45, 200 for
r <= 48.  The planner takes the smallest NP whose workgroups fit both counts.  Largest d_local per NP on 256 compute units:

    RPAD  rpw      NP = 4      NP = 8     NP = 12     NP = 16
       8  256     261 120     522 240     783 360
      16  128     130 560     261 120     391 680
      32   64      65 280     130 560     195 840
      64   32      30 720      61 440      92 160     122 880      r = 33 .. 41
      64   32      28 160      56 320      84 480     112 640      r = 42 .. 45
      64   32      25 600      51 200      76 800     102 400      r = 46 .. 48

Beyond the last column of its row a handle keeps the launched form (psmf_sweep_solve + psmf_serial: two launches per timestep).

`case(i)` is stratified: case i is aimed at TARGETS[i mod len(TARGETS)] -- a persistent instance or one reason for the launched
form -- and the other axes are redrawn until `plan` / `expected_kernel` name that target.  The rows of a case come from the edge
list (EDGES: the geometry edges, each on a fixed case) or from the smallest range of d that reaches the instance; the mode of an
unmasked case (hook configuration, dynamics, in-loop optimiser, schedules, general Q) follows a fixed rotation, one for NP = 4
and one for NP > 4, so that every mode meets the big-d instances whatever the seed.
Reference: pypsmf/psmf/psmf.py:85-180,287-304, rpsmf.py:116-184; ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148."""

import numpy as np

import blocked_cases as BC
import netlib
from blocked_cases import HOOKS, gradsum_bar, mode_of, passes_of, relerr, theta_for  # noqa: F401  (the device test takes them from here)
from oracle import psmf_oracle as O
from oracle.impute_oracle import impute_filter

N_CU = 256                                   # the device the coverage claims are made for
RANKS = {8: (1, 2, 3, 5, 7, 8), 16: (9, 13, 15, 16), 32: (17, 22, 27, 31, 32), 64: (33, 37, 40, 41, 44, 45, 48)}
LAUNCHED_RANKS = (49, 56, 64)
R_LIST = tuple(r for rp in (8, 16, 32, 64) for r in RANKS[rp]) + LAUNCHED_RANKS
ADAM_LR, SGD_LR = BC.ADAM_LR, BC.SGD_LR
MAX_SERIES = 8 * 525_000                     # T x d of the biggest input
BIG_D = 30_000                               # rows beyond which a case runs 3 .. 8 steps


# ---- the planner (pstep_plan, psmf_pstep.hip)
NT, NP_MAX, NP_MAX_BIG, FANIN_ROWS, FANIN_ROWS_BIG = 512, 12, 16, 17, 20


def rpad_of(r):
    return 8 if r <= 8 else (16 if r <= 16 else (32 if r <= 32 else 64))


def rows_per_pass(rpad):
    return NT // (rpad // 4)


def np_variant(rpad, np_):
    """the instance that runs at least np_ passes"""
    return 4 if np_ <= 4 else (8 if np_ <= 8 else (NP_MAX if np_ <= NP_MAX or rpad <= 32 else NP_MAX_BIG))


def fan_in(r):
    """partial rows the hub's fan-in sums: segments x rows per segment"""
    rpad = rpad_of(r)
    npair = ((r + 2) & ~1) // 2
    return min((4 * 64) // npair, 12 if rpad > 32 else 24) * (FANIN_ROWS_BIG if rpad > 32 else FANIN_ROWS)


def plan(d_local, r, n_cu=N_CU, masked=False):
    """pstep_plan step by step: dict(rpad, rpw, np, n_row_wg, rows_per_wg, fan_in), or None where the kernel does not apply."""
    if r < 1 or r > 48 or (r > 32 and masked) or d_local < 1 or n_cu < 2:
        return None
    rpad = rpad_of(r)
    rpw = rows_per_pass(rpad)
    nwg = min(-(-d_local // rpw), n_cu - 1)
    rows = -(-d_local // nwg)
    np_ = -(-rows // rpw)
    np_max = NP_MAX_BIG if rpad > 32 else NP_MAX
    if np_ > np_max:
        return None
    np_ = np_variant(rpad, np_)
    while True:          # more workgroups than the fan-in takes: the next variant
        rows = np_ * rpw
        nwg = -(-d_local // rows)
        if nwg <= fan_in(r):
            break
        if np_ >= np_max:
            return None
        np_ = np_variant(rpad, np_ + 1)
    return dict(rpad=rpad, rpw=rpw, np=np_, n_row_wg=nwg, rows_per_wg=rows, fan_in=fan_in(r))


def d_max(r, np_, n_cu=N_CU):
    """the table of the module docstring: the largest d_local the NP = np_ instance takes at rank r"""
    return min(n_cu - 1, fan_in(r)) * np_ * rows_per_pass(rpad_of(r))


def np_list(rpad):
    return (4, 8, 12) + ((16,) if rpad == 64 else ())


# ---- which handles take the persistent kernel (init_pstep, pstep_usable: psmf_step.hip)
def _on(cs, name):
    return cs["env"].get(name) != "0"


def facts(cs, n_cu=N_CU):
    return dict(
        persistent_switch=_on(cs, "PSMF_STEP_PERSISTENT"),
        rank_fits=cs["r"] <= 32 or (cs["r"] <= 48 and not cs["masked"] and _on(cs, "PSMF_PSTEP_BIG")),
        uniform_R=not cs["nonuniform"],
        walk_or_cos_phase=cs["dyn"] in ("random_walk", "cos_phase"),
        rows_fit=plan(cs["d"], cs["r"], n_cu, cs["masked"]) is not None,
    )


# The first row whose condition fails keeps the launches per timestep; a handle that passes them all runs psmf_pstep_k.
# (One rank, no host-evaluated dynamics, no Q_k matrix schedule and the wave-local solve are further conditions of
# pstep_usable; no case of this list sets them otherwise -- tests/test_hip_switches.py, test_hip_multishard.py do.)
LAUNCHED_TABLE = [
    ("switch_off", "persistent_switch"),          # PSMF_STEP_PERSISTENT=0: two launches per timestep
    ("rank", "rank_fits"),                        # r <= 32; 33 <= r <= 48 unmasked unless PSMF_PSTEP_BIG=0; r > 48 never
    ("nonuniform_R", "uniform_R"),                # a non-uniform diagonal R
    ("dense_kind", "walk_or_cos_phase"),          # the persistent kernel takes the random walk and cos-phase
    ("rows", "rows_fit"),                         # rows beyond the largest plan
]


def launched_reason(cs, n_cu=N_CU):
    f = facts(cs, n_cu)
    return next((name for name, fact in LAUNCHED_TABLE if not f[fact]), None)


def expected_kernel(cs, n_cu=N_CU):
    return "psmf_sweep_solve" if launched_reason(cs, n_cu) else "psmf_pstep_k"


def instance_of(cs, n_cu=N_CU):
    """(RPAD, NP, storage, masked) of the persistent instance the case runs, None on the launched form"""
    if launched_reason(cs, n_cu):
        return None
    return (rpad_of(cs["r"]), plan(cs["d"], cs["r"], n_cu, cs["masked"])["np"], cs["storage"], cs["masked"])


INSTANCES = ([(rp, n, s, m) for rp in (8, 16, 32) for n in (4, 8, 12) for s in ("f32", "f64") for m in (False, True)]
             + [(64, n, s, False) for n in (4, 8, 12, 16) for s in ("f32", "f64")])
# the launched-form targets: (name, what launched_reason answers for them)
LAUNCHED = [("rank_49_to_64", "rank"), ("nonuniform_R", "nonuniform_R"), ("masked_rank_above_32", "rank"), ("persistent_switch_off", "switch_off"),
            ("big_switch_off_rank_33_to_48", "rank"), ("rows_beyond_the_plan", "rows"), ("dense_jacobian_kind", "dense_kind")]


# ---- the edge list: (r, d) pairs that each sit on one case
def _edges():
    out = []
    for rpad in (8, 16, 32, 64):
        rpw, ranks = rows_per_pass(rpad), RANKS[rpad]
        rr = {8: 5, 16: 13, 32: 27, 64: 37}[rpad]          # r mod 4 != 0: a lane group partly empty
        out += [(rr, rr - 1), (rr, rr), (rr, rr + 1)]
        out += [(ranks[j % len(ranks)], d) for j, d in enumerate((1, 2, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1))]
        # the NP thresholds: the last shape of a variant and the first of the next (its last workgroup ends in a pass of one row)
        rt = {8: 7, 16: 16, 32: 32, 64: 40}[rpad]          # (r = 32: 255 = 15 segments x 17 rows; r = 40: 240 = 12 x 20)
        for n in np_list(rpad):
            out += [(rt, d_max(rt, n)), (ranks[(n // 4) % len(ranks)] if rpad < 64 else rt, d_max(rt, n) + 1)]
    # the three windows of d that the planner used to refuse at 33 <= r <= 48, for two fan-in classes
    out += [(r, d) for r in (37, 48) for d in (31_999, 64_001, 95_003)]
    return out


EDGES = _edges()


def masked_ok(r, d):
    """Shapes a masked case takes: eight rows at least (the marked rows and columns of its mask), and r >= 2 -- at r = 1 the
    column without observations takes V to zero exactly (N = s there: V - w w^T / N), and a relative error on V has no scale."""
    return d >= 8 and r >= 2


def _assign_edges():
    """edge -> the target that runs it: the instances of its (RPAD, NP) in turn (masked ones where masked_ok)"""
    per = {t: [] for t in INSTANCES + ["rows_beyond_the_plan"]}
    for r, d in EDGES:
        p = plan(d, r)
        if p is None:
            per["rows_beyond_the_plan"].append((r, d))
            continue
        cand = [t for t in INSTANCES if t[:2] == (p["rpad"], p["np"]) and (not t[3] or masked_ok(r, d))]
        per[min(cand, key=lambda t: (len(per[t]), INSTANCES.index(t)))].append((r, d))
    return per


EDGE_OF = _assign_edges()
# every target as often as it has edges, and once more; twice at least for a persistent instance
TARGETS = [t for t in INSTANCES for _ in range(max(2, len(EDGE_OF[t]) + 1))] + [name for name, _ in LAUNCHED for _ in range(max(1, len(EDGE_OF.get(name, ())), len(LAUNCHED_RANKS) if name == "rank_49_to_64" else 0))]
N_CASES = len(TARGETS)

# the mode of an unmasked case: hooks, dynamics, in-loop optimiser (1 Adam, 2 SGD), schedules, general Q (None: drawn)
MODES = [
    dict(hooks="full", dyn="random_walk", recursive=0),
    dict(hooks="simplified", dyn="random_walk", recursive=0),
    dict(hooks="no_update", dyn="random_walk", recursive=0),
    dict(hooks="eta_R", dyn="random_walk", recursive=0),
    dict(hooks="pbar_P", dyn="random_walk", recursive=0),
    dict(hooks="full", dyn="cos_phase", recursive=0),
    dict(hooks="full", dyn="cos_phase", recursive=1),
    dict(hooks="full", dyn="cos_phase", recursive=2),
    dict(hooks="full", dyn="random_walk", recursive=0, sched=True),
    dict(hooks="full", dyn="random_walk", recursive=0, general_Q=True),
    dict(hooks="simplified", dyn="cos_phase", recursive=1),
    dict(),
]


def _mode_slots():
    """case -> its place in the rotation: the unmasked persistent cases counted separately at NP = 4 and beyond"""
    slot, count = {}, {False: 0, True: 0}
    for i, t in enumerate(TARGETS):
        if isinstance(t, tuple) and not t[3]:
            big = t[1] > 4
            slot[i] = count[big]
            count[big] += 1
    return slot


MODE_SLOT = _mode_slots()


def occurrence(i):
    """which of its target's cases case i is"""
    return sum(1 for t in TARGETS[:i] if t == TARGETS[i])


# ---- the draw
def _horizon(rng, cs):
    d = cs["d"]
    if d > BIG_D:
        T = int(rng.integers(3, 9))
        return max(3, min(T, MAX_SERIES // d))
    if cs["dyn"] != "random_walk" and cs["storage"] == "f32":
        # a trigonometric f on float32 inputs: the oracle's own answer moves by more than 1e-5 / 16 within ten steps or so
        return int(rng.integers(2, 9))
    return int(rng.integers(12, 37))


def _parts(rng, T, empty=True):
    """one to three launches, the cuts biased to 1 and T - 1; one case in eight with an empty run between parts"""
    cuts = set()
    want = min(int(rng.integers(0, 3)), T - 1)
    while len(cuts) < want:
        cuts.add(int(rng.choice([1, T - 1])) if rng.random() < 0.6 else int(rng.integers(1, T)))
    pts = [0] + sorted(cuts) + [T]
    parts = list(zip(pts[:-1], pts[1:]))
    if empty and rng.random() < 0.125:
        a = int(rng.choice(pts))
        k = next((j + 1 for j, p in enumerate(parts) if p[1] == a), 0)
        parts.insert(k, (a, a))
    return parts


def _rows(rng, r, n, occ, edges):
    """rows of a case aimed at the NP = n instance at rank r: its edge if it has one left, else the smallest range"""
    if occ < len(edges):
        return edges[occ]
    if n == 4:
        return r, int(rng.integers(2, 6 * 4 * rows_per_pass(rpad_of(r)) + 1))
    lo = d_max(r, {8: 4, 12: 8, 16: 12}[n])
    return r, int(rng.integers(lo + 1, lo + 721))


def _base(rng, r, d, storage, masked):
    robust = bool(rng.random() < 0.5)
    scaled = robust and rng.random() < 0.3
    return dict(r=r, d=d, storage=storage, masked=masked, robust=robust, nonuniform=False, env={}, dyn="random_walk", hooks="full", recursive=0,
                update_every=1, sched=False, general_Q=False, second_pass=False, v0=0.02 if storage == "f32" else 0.1,
                fixed_lambda=bool(robust and rng.random() < 0.25), alpha=float(rng.choice([0.95, 1.05])) if scaled else 1.0,
                beta=float(rng.choice([0.95, 1.05])) if scaled else 1.0)


def _draw_modes(rng, cs, mode):
    """the axes of an unmasked case that the rotation leaves open"""
    cs["hooks"] = mode.get("hooks", str(rng.choice(list(HOOKS), p=[0.52, 0.18, 0.1, 0.1, 0.1])))
    cs["dyn"] = mode.get("dyn", "cos_phase" if rng.random() < 0.35 else "random_walk")
    u = rng.random()
    cs["recursive"] = mode.get("recursive", (0 if u < 0.5 else (1 if u < 0.8 else 2)) if cs["dyn"] == "cos_phase" else 0)
    cs["update_every"] = int(rng.choice([1, 3, 7])) if cs["recursive"] else 1
    if mode.get("sched"):
        cs["robust"], cs["fixed_lambda"], cs["alpha"], cs["beta"] = False, False, 1.0, 1.0      # R_k / Q_k schedules: PSMF only
    cs["sched"] = bool(mode.get("sched", (not cs["robust"]) and rng.random() < 0.25))
    cs["general_Q"] = bool(mode.get("general_Q", rng.random() < 0.3))


def _draw(rng, i):
    t, occ = TARGETS[i], occurrence(i)
    if isinstance(t, tuple):
        rpad, n, storage, masked = t
        r = int(rng.choice(RANKS[rpad]))
        r, d = _rows(rng, r, n, occ, EDGE_OF[t])
        cs = _base(rng, r, d, storage, masked)
        if masked:
            if not masked_ok(r, d):
                return None
        else:
            _draw_modes(rng, cs, MODES[MODE_SLOT[i] % len(MODES)])
    else:
        storage = "f32" if rng.random() < 0.3 else "f64"
        small = lambda r: int(rng.integers(max(r + 3, 20), 2500))          # noqa: E731
        if t == "rank_49_to_64":
            r = LAUNCHED_RANKS[occ % len(LAUNCHED_RANKS)]
            cs = _base(rng, r, small(r), storage, False)
        elif t == "nonuniform_R":
            r = int(rng.choice(R_LIST))
            cs = dict(_base(rng, r, small(r), storage, False), nonuniform=True)
        elif t == "masked_rank_above_32":
            r = int(rng.choice(RANKS[64]))
            cs = _base(rng, r, small(r), storage, True)
        elif t == "persistent_switch_off":
            r = int(rng.choice(R_LIST[:-3]))
            cs = dict(_base(rng, r, small(r), storage, False), env={"PSMF_STEP_PERSISTENT": "0"})
            _draw_modes(rng, cs, {})
        elif t == "big_switch_off_rank_33_to_48":
            r = int(rng.choice(RANKS[64]))
            cs = dict(_base(rng, r, small(r), storage, False), env={"PSMF_PSTEP_BIG": "0"})
            _draw_modes(rng, cs, {})
        elif t == "rows_beyond_the_plan":
            r, d = EDGE_OF[t][occ]
            cs = _base(rng, r, d, storage, False)
        else:      # a dense-Jacobian dynamics kind: the affine one (few parameters at a small rank)
            r = int(rng.choice(RANKS[8] + RANKS[16]))
            cs = dict(_base(rng, r, small(r), "f64", False), dyn=str(rng.choice(["scaled_walk", "scaled_walk_bias"])))
    cs["T"] = _horizon(rng, cs)
    if cs["masked"]:
        cs["T"] = max(cs["T"], 3)          # the three marked columns of the mask
    cs["second_pass"] = bool(not cs["masked"] and cs["d"] <= BIG_D and rng.random() < 1 / 3)
    cs["seed"] = int(rng.integers(1 << 30))
    return cs


def target_of(cs, n_cu=N_CU):
    """what a configuration lands on: an instance, or the launched-form reason"""
    return instance_of(cs, n_cu) or launched_reason(cs, n_cu)


def case(i, salt=0):
    """Configuration number i; `salt` > 0 gives the replacements the conditioning check may ask for."""
    t = TARGETS[i % len(TARGETS)]
    want = t if isinstance(t, tuple) else dict(LAUNCHED)[t]
    rng = np.random.default_rng([8200 + i, salt])
    for _ in range(2000):
        cs = _draw(rng, i)
        if cs is not None and target_of(cs) == want:
            break
    else:
        raise AssertionError(f"no draw reaches {t}")
    cs["parts"] = _parts(rng, cs["T"], empty=not cs["masked"])
    cs["i"], cs["salt"], cs["shortened"], cs["target"] = i, salt, 0, t
    return cs


def shorten(cs):
    """The same case over half the horizon (not below 2 steps; masked: 3), its cut points redrawn; None when it cannot be halved."""
    T = max(cs["T"] // 2, 3 if cs["masked"] else 2)
    if T >= cs["T"] or cs["shortened"] >= 2:
        return None
    out = dict(cs, T=T, shortened=cs["shortened"] + 1)
    out["parts"] = _parts(np.random.default_rng([8200 + cs["i"], cs["salt"], out["shortened"]]), T, empty=not cs["masked"])
    return out


# ---- tolerances: the bars the suite states for this engine
def bar(cs):
    if cs["storage"] == "f32":
        return 1e-5
    return 5e-9 if cs["masked"] else 1e-9


# ---- the problem of a case
def problem(cs, perturb=None):
    """Unmasked: blocked_cases.problem (Y, C0, V0, P0, Q, mu0, theta, schedules), and diag(R) of a non-uniform case.
    Masked: the inputs of the reference's masked filter, (d, T) column-major in time as it takes them, and the mask."""
    if cs["masked"]:
        return _masked_problem(cs, perturb)
    pb = BC.problem(cs, perturb)
    if cs["nonuniform"]:
        pb["rho_rows"] = 0.3 + 2.0 * np.random.default_rng(cs["seed"] ^ 0xD1A6).random(cs["d"])
    return pb


def _mask(cs, rng):
    """The observation mask (d, T): 60 % observed; row 3 never; column 1 not at all; in column 0 one whole row workgroup
    unobserved; in column 2 the rows of the last workgroup observed alone (both where the plan has two workgroups or more)."""
    d, T = cs["d"], cs["T"]
    M = (rng.random((d, T)) > 0.4).astype(int)
    p = plan(d, min(cs["r"], 32), N_CU, True)
    if p["n_row_wg"] >= 2:
        w, R = p["n_row_wg"] // 2, p["rows_per_wg"]
        M[w * R:(w + 1) * R, 0] = 0
        M[:, 2] = 0
        M[(p["n_row_wg"] - 1) * R:, 2] = 1
    M[:, 1] = 0
    M[3] = 0
    return M


def _masked_problem(cs, perturb):
    d, r, T = cs["d"], cs["r"], cs["T"]
    rng = np.random.default_rng(cs["seed"])
    Yorig = np.cumsum(0.3 * rng.standard_normal((d, T)), axis=1) + 3.0 * rng.random((d, 1))
    M = _mask(cs, rng)
    Mmiss = ((1 - M) * (rng.random((d, T)) > 0.1)).astype(float)
    Mmiss[3, 0] = 1.0          # (held out whatever the draw: the metrics divide by the count)
    C0, X0 = rng.random((d, r)), rng.random((r, T))
    f32 = ("Yorig", "C0") if cs["storage"] == "f32" else ()
    if f32:
        Yorig, C0 = netlib.f32_round(Yorig), netlib.f32_round(C0)
    if perturb is not None:
        Yorig, C0 = netlib.perturbed(dict(Yorig=Yorig, C0=C0), *perturb, f32=f32).values()
    return dict(Yorig=Yorig, M=M, Mmiss=Mmiss, C0=C0, X0=X0, V0=2 * np.eye(r), Q=0.1 * np.eye(r), P0=np.eye(r), rho=10.0, lam=1.8, sig=2.0)


def reference(cs, pb):
    """Unmasked: one record per part (blocked_cases.reference: state after the part, y_pred of the part).  Masked: the end of
    the reference's masked filter after one pass -- dict(C, X (T, r), V, P, Epred, Efull, coverage)."""
    if cs["masked"]:
        X = pb["X0"].copy()
        ep, ef, inside, st = impute_filter(pb["Yorig"] * pb["M"], pb["C0"], X, pb["M"], pb["Mmiss"], pb["V0"], pb["Q"], pb["rho"], pb["P0"], pb["sig"], 1,
                                           pb["Yorig"], 0.0, robust=cs["robust"], lambda0=pb["lam"], return_state=True)
        return dict(C=st["C"], X=st["X"].T.copy(), V=st["V"], P=st["P"], Epred=float(ep[0, 1]), Efull=float(ef[0, 1]), coverage=float(inside))
    if not cs["nonuniform"]:
        return BC.reference(cs, pb)[0]
    # a non-uniform diagonal R (random walk, the full filter): the oracle's state carries diag(R) as a vector
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=pb["rho_rows"].copy(), lam=pb["lam"])
    out = []
    for ep in range(passes_of(cs)):
        if ep and cs["robust"]:
            st.Q, st.rho, st.lam = pb["Q"].copy(), pb["rho_rows"].copy(), pb["lam"]
        for a, b in cs["parts"]:
            Yp = np.empty((0, cs["d"]))
            if b > a:
                st, Yp, _ = O.run_epoch(st, pb["Y"][a:b], mode_of(cs), O.RandomWalkDyn(), k0=a, want_grad=False)
            out.append(dict(ep=ep, a=a, b=b, C=st.C.copy(), V=st.V.copy(), mu=st.mu.copy(), P=st.P.copy(), Q=np.array(st.Q, dtype=float),
                            rho=np.array(st.rho, dtype=float), lam=float(st.lam), theta=np.zeros(0), gradsum=np.zeros(0), y_pred=np.asarray(Yp).reshape(b - a, cs["d"])))
    return out


STATE_KEYS = ("C", "V", "mu", "P", "y_pred")
MASKED_KEYS = ("C", "X", "V", "P", "Epred", "Efull")


def sensitivity(cs):
    """relerr between the oracle on the case's inputs and on inputs moved by a relative 2^-50 (float32 storage: 2^-23, after the
    rounding): (the worst over the compared quantities, the worst gradsum; masked: the change of the coverage)."""
    eps = 2.0 ** -23 if cs["storage"] == "f32" else 2.0 ** -50
    ref0 = reference(cs, problem(cs))
    ref1 = reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, eps)))
    if cs["masked"]:
        netlib.require_finite(ref0, MASKED_KEYS, f"case {cs['i']}")
        return netlib.response(ref0, ref1, MASKED_KEYS), abs(ref1["coverage"] - ref0["coverage"])
    for part in ref0:
        netlib.require_finite(part, STATE_KEYS + ("gradsum",), f"case {cs['i']}")
    return netlib.response(ref0, ref1, STATE_KEYS), BC.grad_response(ref0, ref1)


def coverage_bar(cs):
    """masked cases: the coverage matches exactly with float64 storage, to 5e-4 with float32 (entries at a band edge)"""
    return 5e-4 if cs["storage"] == "f32" else 0.0


def admissible(cs):
    state, second = sensitivity(cs)
    what, second_bar = ("coverage", coverage_bar(cs)) if cs["masked"] else ("gradsum", gradsum_bar(cs))
    return state <= bar(cs) / 16 and second <= second_bar / 16, f"sensitivity {state:.2e} (bar {bar(cs):.0e}), {what} {second:.2e}"


def describe(cs):
    return f"T={cs['T']} d={cs['d']} r={cs['r']} {cs['storage']} {cs['dyn']} {cs['hooks']}"


# What `resolve` answers for the cases it does not leave alone, {i: (salt, times shortened)}: recorded here so that the device
# test need not run the oracle three times per case; tests/test_step_cases_cpu.py recomputes every entry (and every absence).
RESOLUTION = {117: (0, 1), 130: (0, 1), 131: (0, 1)}


def resolve(i):
    """netlib.resolve on this net (halving not below 2 steps; masked: 3): ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


def device_case(i):
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))
