"""Seeded random configurations of the per-step engine's launched form aimed at the matrix-core Gram mgram_body
(rpsmf_amd/csrc/psmf_masked.hip): the masked Gram sum m_i c_i c_i^T of every launched masked step (psmf_serial_mgram, MODE 0)
and the weighted Gram sum kappa_i c_i c_i^T of every step with a non-uniform or dense R (psmf_wgram_mfma, MODE 1); the problem
each case runs and the float64 oracle of it.  Pure Python: tests/test_gram_cases_cpu.py checks the list's coverage and the
conditioning of every case without a GPU, tests/test_hip_masked_gram_net.py runs the same list on the device.

The geometry, in numbers (`gram_plan`).  256 Gram workgroups of NW waves; a wave takes slabs of 16 rows, slab number
bid * NW + w first and then every (256 NW)-th: a wave makes a second trip through its slab loop -- the prefetched registers,
the reuse of its LDS image, the accumulation over slabs -- only beyond 16 * 256 * NW rows:

    kernel              padded rank           NT  NW    one slab per wave up to d_local =
    psmf_serial_mgram   8, 16                  1  16    65 536
    psmf_serial_mgram   32                     2   8    32 768
    psmf_serial_mgram   64 (r <= 48 / > 48)  3/4   4    16 384
    psmf_wgram_mfma     any (NT = 1 .. 4)   1..4   8    32 768

The list is stratified over TARGETS: a masked target is (padded-rank class, storage, the reason the handle keeps the launches
per timestep), a weighted one (NT, storage, matrix cores or the vector-unit twin).  The rows of a case come from the edge list
of its NW class (EDGES: each edge on one fixed case) or are drawn; the ranks are dealt per class so that every class edge and
an odd rank of every class is met whatever the seed.  SHARDED adds fixed sharded cases: the three masked methods and the
non-uniform-R step on 2 .. 4 uneven row shards, a shard below 16 rows, shards that straddle the one-slab bound.
Reference: ExperimentImpute/PSMF.py:40-95, rPSMF.py:40-148, MLESMF.py:40-92, TMF.py:30-73; pypsmf/psmf/psmf.py:140-152."""

import numpy as np

import netlib
from netlib import f32_round, relerr, spd  # noqa: F401  (the device tests take relerr from here)
from oracle import psmf_oracle as O
from oracle.impute_oracle import impute_filter, mle_smf_filter, tmf_filter

# ---- the geometry (psmf_masked.hip, psmf_step.hip)
N_WG = 256                 # kMGramWG, psmf_step.hip: "constexpr int kMGramWG = 256"
SLAB = 16                  # mgram_body: "const int nslab = (dl + 15) / 16"
WGRAM_NW = 8               # wgram_inst, psmf_step.hip: "psmf::psmf_wgram_mfma<T, NT, 8>"
# serial_mgram_for, psmf_step.hip: class -> (NT, NW); class = the padded rank, 64 split at r = 48 ("r <= 48 ? <64, T, 3, 4> : <64, T, 4, 4>")
MGRAM = {8: (1, 16), 16: (1, 16), 32: (2, 8), 48: (3, 4), 64: (4, 4)}
# wgram_for, psmf_step.hip: "rpad <= 16 -> NT 1; rpad == 32 -> 2; r <= 48 ? 3 : 4"
WGRAM_NT = {8: 1, 16: 1, 32: 2, 48: 3, 64: 4}
CLASSES = (8, 16, 32, 48, 64)
BIG_D = 16_000             # rows beyond which a case runs 3 .. 6 steps and one pass


def class_of(r):
    """the padded rank (geo.rpad), with 64 split where both kernels change their tile count"""
    return 8 if r <= 8 else (16 if r <= 16 else (32 if r <= 32 else (48 if r <= 48 else 64)))


def gram_plan(d_local, r, mode):
    """mgram_body's geometry for `mode` = "mgram" (psmf_serial_mgram) or "wgram" (psmf_wgram_mfma): dict(nt, nw, n_wg, n_slab,
    trips = the most slabs one wave takes, last_rows = rows of the last slab, bound = rows up to which trips == 1)."""
    cls = class_of(r)
    nt, nw = MGRAM[cls] if mode == "mgram" else (WGRAM_NT[cls], WGRAM_NW)
    n_slab = (d_local + SLAB - 1) // SLAB
    stride = N_WG * nw                      # mgram_body: "stride = nblk * NW"
    return dict(nt=nt, nw=nw, n_wg=N_WG, n_slab=n_slab, stride=stride, trips=-(-n_slab // stride),
                last_rows=d_local - SLAB * (n_slab - 1), bound=SLAB * stride)


# ---- targets
STORAGES = ("f32", "f64")
REASONS = ("mle_smf", "tmf", "big_rank", "switch_off", "shards")


def reasons_of(cls):
    return ("mle_smf", "tmf") + (("big_rank",) if cls > 32 else ("switch_off", "shards"))


MASKED_TARGETS = [("m", cls, s, why) for cls in CLASSES for s in STORAGES for why in reasons_of(cls)]
WEIGHTED_TARGETS = ([("w", nt, s, "mfma") for nt in (1, 2) for s in STORAGES] + [("w", 3, "f64", "mfma"), ("w", 3, "f32", "mfma")]
                    + [("w", 4, s, "mfma") for s in STORAGES] + [("w", 1, "f64", "valu"), ("w", 3, "f32", "valu")])
TARGETS = MASKED_TARGETS + WEIGHTED_TARGETS
# the NW classes: name -> (mode, NW, the targets that run on it)
GROUPS = {
    "mgram16": ("mgram", 16, [t for t in MASKED_TARGETS if t[1] in (8, 16)]),
    "mgram8": ("mgram", 8, [t for t in MASKED_TARGETS if t[1] == 32]),
    "mgram4": ("mgram", 4, [t for t in MASKED_TARGETS if t[1] in (48, 64)]),
    "wgram8": ("wgram", 8, WEIGHTED_TARGETS),
}
RANKS = {8: (2, 3, 5, 7, 8), 16: (9, 13, 15, 16), 32: (17, 23, 31, 32), 48: (33, 41, 47, 48), 64: (49, 55, 63, 64)}
WRANKS = {1: (1, 16, 9, 3, 15, 8, 2, 13), 2: (17, 31, 32, 23), 3: (33, 47, 48, 41), 4: (49, 63, 64, 55)}
RANK_EDGES = (1, 2, 3, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)


def edges_of(nw):
    """the row edges of an NW class: around one slab per wave, three trips, and the small end"""
    b = SLAB * N_WG * nw
    d3 = 2 * b + b // 2 + 7            # between 2 x and 3 x the bound, d mod 16 = 7: some waves make three trips
    return [b + 1, 8, b, 15, b + 17, 16, b - 1, 17, d3, SLAB * nw - 1, SLAB * nw + 1, SLAB * N_WG - 1, SLAB * N_WG + 1]


EDGES = {g: edges_of(nw) for g, (_, nw, _) in GROUPS.items()}

# fixed sharded cases: (target, rank, shard sizes, what it is there for)
SHARDED = [
    (("m", 16, "f64", "mle_smf"), 13, (700, 9, 1300), "MLE-SMF on three shards, one below 16 rows"),
    (("m", 32, "f64", "tmf"), 23, (300, 3, 801, 150), "TMF on four shards, one of three rows"),
    (("m", 32, "f64", "shards"), 17, (32_768 + 40, 5_000), "PSMF straddling the one-slab bound: two trips beside one"),
    (("m", 48, "f64", "big_rank"), 41, (9, 1_200), "r > 32 sharded, one shard of one partial slab"),
    (("m", 8, "f32", "mle_smf"), 5, (1_000, 1_003), "float32 storage, MLE-SMF on two shards"),
    (("w", 1, "f64", "mfma"), 15, (11, 1_500), "non-uniform R on two shards, one below 16 rows"),
    (("w", 2, "f64", "mfma"), 31, (400, 1_001, 600), "non-uniform R on three shards"),
    (("w", 3, "f64", "mfma"), 47, (32_768 + 33, 900), "non-uniform R straddling the one-slab bound"),
    (("w", 1, "f32", "mfma"), 8, (500, 7, 400, 93), "non-uniform R, float32 storage, four shards"),
]


def _specs():
    """(target, edge or None, sharded entry or None) of every case, in order"""
    out = []
    for g, (_, _, targets) in GROUPS.items():
        plain = [t for t in targets if t[3] != "shards"]
        for j in range(max(len(EDGES[g]), len(plain))):
            out.append((plain[j % len(plain)], EDGES[g][j] if j < len(EDGES[g]) else None, None))
        out += [(t, None, None) for t in targets if t[3] == "shards"]
    out += [(t, None, (r, sh)) for t, r, sh, _ in SHARDED]
    return out


SPECS = _specs()
N_CASES = len(SPECS)


def _rank(i):
    """dealt: the ranks of a class in turn over the cases of that class"""
    t = SPECS[i][0]
    same = sum(1 for s in SPECS[:i] if s[0][0] == t[0] and s[0][1] == t[1] and s[2] is None)
    ranks = RANKS[t[1]] if t[0] == "m" else WRANKS[t[1]]
    return ranks[same % len(ranks)]


# ---- the draw
def _parts(rng, T, marks=()):
    """two or three launches; the cuts biased to `marks` (right behind the empty and the full column of a mask)"""
    want = min(int(rng.integers(1, 3)), T - 1)
    cuts = set()
    while len(cuts) < want:
        free = [c for c in marks if 0 < c < T and c not in cuts]
        cuts.add(int(rng.choice(free)) if free and rng.random() < 0.7 else int(rng.integers(1, T)))
    pts = [0] + sorted(cuts) + [T]
    return list(zip(pts[:-1], pts[1:]))


CUT_MARKS = (2, 4)         # behind column 1 (no observation) and column 3 (every row observed)


def case(i, salt=0):
    """Configuration number i; `salt` > 0 gives the replacements the conditioning check may ask for."""
    t, edge, sharded = SPECS[i]
    rng = np.random.default_rng([9400 + i, salt])
    kind, cls_or_nt, storage, why = t
    masked = kind == "m"
    r = sharded[0] if sharded else _rank(i)
    shards = tuple(sharded[1]) if sharded else ()
    if shards:
        d = sum(shards)
    elif edge is not None:
        d = edge
    elif why == "shards":
        d = int(rng.integers(60, 3000))
        n = 2 + sum(1 for s in SPECS[:i] if s[0][3] == "shards") % 3
        cutp = sorted(int(c) for c in rng.choice(np.arange(5, d - 5), size=n - 1, replace=False))
        shards = tuple(b - a for a, b in zip([0] + cutp, cutp + [d]))
        if n == 3:                                   # one shard of one partial slab
            shards = (9, shards[1] + shards[0] - 9, shards[2]) if shards[0] > 9 else shards
    else:
        d = int(rng.integers(max(r + 3, 20), 2500))
    big = d > BIG_D
    # PSMF and rPSMF dealt in turn over the cases of a class, so that each class meets both whatever the seed
    turn = sum(1 for s in SPECS[:i] if s[0][:2] == t[:2] and s[0][3] not in ("mle_smf", "tmf"))
    method = why if why in ("mle_smf", "tmf") else ("psmf", "rpsmf")[turn % 2]
    cs = dict(kind=kind, masked=masked, method=method, robust=method == "rpsmf", r=r, d=d, storage=storage, shards=shards, env={},
              target=t, edge=edge)
    if why == "switch_off":
        cs["env"] = {"PSMF_STEP_PERSISTENT": "0"}
    if why == "valu":
        cs["env"] = {"PSMF_WGRAM_MFMA": "0"}
    if big:
        cs["T"] = int(rng.integers(5, 7)) if masked else int(rng.integers(3, 7))
        cs["passes"] = 1
    else:
        cs["T"] = int(rng.integers(8, 17)) if storage == "f32" else int(rng.integers(12, 31))
        cs["passes"] = int(rng.integers(1, 4))
    cs["general_Q"] = bool(rng.random() < 0.5)
    cs["rho"] = float(np.exp(rng.uniform(np.log(0.5), np.log(20.0)))) if masked else 1.0
    cs["lam"] = float(rng.uniform(0.5, 5.0))
    cs["sig"] = float(rng.uniform(0.5, 3.0))
    # a column with no observation: r >= 3 (at r = 2 V has no direction left after two such columns), never MLE-SMF (eta = 0)
    cs["empty_col"] = bool(masked and r >= 3 and method != "mle_smf")
    # the unsharded float64 cases beyond the one-workgroup engine that need no switch go through impute_batch (a quarter of the masked cases)
    cs["route"] = "batch" if (masked and not shards and storage == "f64" and not cs["env"] and (d > 512 or r > 16)) else "handle"
    if cs["route"] == "batch" and not big:
        cs["passes"] = max(cs["passes"], 2)          # the drop-in functions run several passes: the batch route is for those
    # the state handed back through set_state at every cut: the next run prepares again and re-forms the look-ahead Gram there
    cs["restate"] = bool(masked and cs["route"] == "handle" and rng.random() < 0.5)
    cs["rotated"] = bool(not masked and not shards and d <= 400 and why == "mfma" and rng.random() < 0.7)
    cs["wide_rho"] = bool(not masked and i == WIDE_RHO_CASE)
    cs["parts"] = [(0, cs["T"])] if cs["route"] == "batch" else _parts(rng, cs["T"], CUT_MARKS if masked else ())
    cs["seed"] = int(rng.integers(1 << 30))
    cs["i"], cs["salt"], cs["shortened"] = i, salt, 0
    return cs


WIDE_RHO_CASE = next(i for i, s in enumerate(SPECS) if s[0][0] == "w" and s[1] is not None and 1000 < s[1] < BIG_D)


def shorten(cs):
    """The same case over half the horizon (masked: not below the six marked columns; weighted: 3), one pass less; None when neither moves."""
    T = max(cs["T"] // 2, 6 if cs["masked"] else 3)
    passes = max(cs["passes"] - 1, 1)
    if (T >= cs["T"] and passes >= cs["passes"]) or cs["shortened"] >= 2:
        return None
    out = dict(cs, T=min(T, cs["T"]), passes=passes, shortened=cs["shortened"] + 1)
    rng = np.random.default_rng([9400 + cs["i"], cs["salt"], out["shortened"]])
    out["parts"] = [(0, out["T"])] if cs["route"] == "batch" else _parts(rng, out["T"], CUT_MARKS if cs["masked"] else ())
    return out


def reached(cs):
    """what a configuration lands on, restated from the dispatch: the masked handle's (class, storage, reason for the launched
    form) -- pstep_usable, psmf_step.hip: masked = 2 / 3 never, r > 32 never, a communicator never, PSMF_STEP_PERSISTENT=0 never --
    or the weighted Gram's (NT, storage, unit: enqueue_weighted_gram)"""
    if not cs["masked"]:
        return ("w", WGRAM_NT[class_of(cs["r"])], cs["storage"], "valu" if cs["env"].get("PSMF_WGRAM_MFMA") == "0" else "mfma")
    if cs["method"] in ("mle_smf", "tmf"):
        why = cs["method"]
    elif cs["r"] > 32:
        why = "big_rank"
    elif cs["shards"]:
        why = "shards"
    elif cs["env"].get("PSMF_STEP_PERSISTENT") == "0":
        why = "switch_off"
    else:
        why = None              # the persistent kernel: tests/step_cases.py
    return ("m", class_of(cs["r"]), cs["storage"], why)


def plan_of(cs, d_local=None):
    return gram_plan(cs["d"] if d_local is None else d_local, cs["r"], "mgram" if cs["masked"] else "wgram")


# ---- tolerances: the bars the suite states for these paths
def bar(cs):
    if cs["storage"] == "f32":
        return 1e-5
    return 5e-9 if cs["masked"] else 1e-9


def coverage_bar(cs):
    """masked cases: the coverage matches exactly with float64 storage, to 5e-4 with float32 (entries at a band edge)"""
    return 5e-4 if cs["storage"] == "f32" else 0.0


SHARD_BAR = 1e-11          # sharded against unsharded, float64 storage


# ---- the problem of a case
def mask_of(cs, rng):
    """The observation mask (d, T): 60 % observed; row 3 never; column 0: one whole wave's slab unobserved; column 1: no
    observation (`empty_col`); column 2: the rows of the last slab alone; column 3: every row; column 4, where a wave takes two
    slabs or more: only the slabs of a second or later trip -- a Gram that drops them has n_obs = 0 there.  Every other column
    keeps one observation at least."""
    d, T = cs["d"], cs["T"]
    p = plan_of(cs)
    M = (rng.random((d, T)) > 0.4).astype(int)
    s0 = p["n_slab"] // 2
    M[SLAB * s0:SLAB * (s0 + 1), 0] = 0
    M[:, 2] = 0
    M[SLAB * (p["n_slab"] - 1):, 2] = 1
    M[:, 3] = 1
    if p["trips"] >= 2:
        M[:, 4] = 0
        M[SLAB * p["stride"]:, 4] = 1
    M[3] = 0
    for t in np.flatnonzero(M.sum(axis=0) == 0):
        M[5, t] = 1
    if cs["empty_col"]:
        M[:, 1] = 0
    return M


def problem(cs, perturb=None):
    """Masked: the inputs of the reference's masked filters, (d, T) as they take them.  Weighted: Y (T, d), C0, V0, P0, Q, mu0,
    diag(R) (and U of a rotated case).  `perturb` = (seed, eps): C0 and Y times (1 + eps u), u uniform in [-1, 1] -- after the
    rounding to float32 where the device stores float32, and rounded again."""
    d, r, T = cs["d"], cs["r"], cs["T"]
    rng = np.random.default_rng(cs["seed"])
    f32 = cs["storage"] == "f32"
    if cs["masked"]:
        Y = np.cumsum(0.3 * rng.standard_normal((d, T)), axis=1) + 3.0 * rng.random((d, 1))
        M = mask_of(cs, rng)
        Mmiss = ((1 - M) * (rng.random((d, T)) > 0.1)).astype(float)
        Mmiss[3, 0] = 1.0
        C0, X0 = rng.random((d, r)), rng.random((r, T))
        pb = dict(M=M, Mmiss=Mmiss, X0=X0, V0=spd(rng, r, 2.0), P0=spd(rng, r, 1.0), Q=spd(rng, r, 0.05) if cs["general_Q"] else 0.1 * np.eye(r))
    else:
        Ct = rng.standard_normal((d, r))
        x = rng.standard_normal(r)
        Y = np.empty((T, d))
        for t in range(T):
            x = 0.9 * np.sin(x + 0.3) + 0.1 * rng.standard_normal(r)
            Y[t] = Ct @ x + 0.3 * (rng.standard_t(3.0, d) if cs["robust"] else rng.standard_normal(d))
        C0 = 0.1 * rng.standard_normal((d, r))
        rho_rows = 10.0 ** (3.0 * rng.random(d) - 1.5) if cs["wide_rho"] else 0.3 + 2.0 * rng.random(d)
        pb = dict(V0=spd(rng, r, 0.02 if f32 else 0.1), P0=spd(rng, r, 1.0), Q=spd(rng, r, 0.05) if cs["general_Q"] else 0.1 * np.eye(r),
                  mu0=0.2 * rng.standard_normal(r), rho_rows=rho_rows)
        if cs["rotated"]:
            pb["U"] = np.linalg.qr(rng.standard_normal((d, d)))[0]
    if f32:
        Y, C0 = f32_round(Y), f32_round(C0)
    if perturb is not None:
        Y, C0 = netlib.perturbed(dict(Y=Y, C0=C0), *perturb, f32=("Y", "C0") if f32 else ()).values()
    pb.update(Y=Y, C0=C0)
    return pb


def reference(cs, pb):
    """Masked: the end of the reference's filter after `passes` passes -- dict(C, X (T, r), Yrec (T, d), Epred, Efull (passes,),
    and V, P, coverage, YrecL, YrecH where the method has them).  Weighted: one record per part and pass (C, V, mu, P, y_pred)."""
    if cs["masked"]:
        Y, M, Mmiss, X = pb["Y"], pb["M"], pb["Mmiss"], pb["X0"].copy()
        n = cs["passes"]
        if cs["method"] == "mle_smf":
            ep, ef, inside, st = mle_smf_filter(Y * M, pb["C0"], X, M, Mmiss, pb["Q"], cs["rho"], pb["P0"], cs["sig"], n, Y, 0.0, return_state=True)
        elif cs["method"] == "tmf":
            ep, ef, st = tmf_filter(Y * M, pb["C0"], X, M, Mmiss, n, Y, 0.0, return_state=True)
            inside = None
        else:
            ep, ef, inside, st = impute_filter(Y * M, pb["C0"], X, M, Mmiss, pb["V0"], pb["Q"], cs["rho"], pb["P0"], cs["sig"], n, Y, 0.0,
                                               robust=cs["robust"], lambda0=cs["lam"], return_state=True)
        out = dict(C=st["C"], X=st["X"].T.copy(), Yrec=st["Yrec"].T.copy(), Epred=ep[0, 1:].copy(), Efull=ef[0, 1:].copy())
        for k in ("V", "P"):
            if k in st:
                out[k] = st[k]
        if inside is not None:
            out.update(coverage=float(inside), YrecL=st["YrecL"].T.copy(), YrecH=st["YrecH"].T.copy())
        return out
    R = (pb["U"] * pb["rho_rows"]) @ pb["U"].T if cs["rotated"] else pb["rho_rows"].copy()
    st = O.State(C=pb["C0"].copy(), V=pb["V0"].copy(), mu=pb["mu0"].copy(), P=pb["P0"].copy(), Q=pb["Q"].copy(), rho=R.copy(), lam=cs["lam"])
    kw = dict(step=O.literal_step) if cs["rotated"] else dict(want_grad=False)
    out = []
    for ep in range(cs["passes"]):
        if ep and cs["robust"]:
            st.Q, st.rho, st.lam = pb["Q"].copy(), R.copy(), cs["lam"]
        for a, b in cs["parts"]:
            st, Yp, _ = O.run_epoch(st, pb["Y"][a:b], O.Mode(robust=cs["robust"]), O.RandomWalkDyn(), k0=a, **kw)
            out.append(dict(ep=ep, a=a, b=b, C=st.C.copy(), V=st.V.copy(), mu=st.mu.copy(), P=st.P.copy(), y_pred=np.asarray(Yp).reshape(b - a, cs["d"])))
    return out


WEIGHTED_KEYS = ("C", "V", "mu", "P", "y_pred")
MASKED_KEYS = ("C", "X", "V", "P", "Yrec", "YrecL", "YrecH", "Epred", "Efull")


def sensitivity(cs):
    """relerr between the oracle on the case's inputs and on inputs moved by a relative 2^-50 (float32 storage: 2^-23, after the
    rounding): (the worst over the compared quantities, masked: the change of the coverage)."""
    eps = 2.0 ** -23 if cs["storage"] == "f32" else 2.0 ** -50
    with np.errstate(all="ignore"):
        ref0 = reference(cs, problem(cs))
        ref1 = reference(cs, problem(cs, perturb=(cs["seed"] ^ 0x5EED, eps)))
    if cs["masked"]:
        keys = [k for k in MASKED_KEYS if k in ref0]
        netlib.require_finite(ref0, keys, f"case {cs['i']}")
        return netlib.response(ref0, ref1, keys), abs(ref1["coverage"] - ref0["coverage"]) if "coverage" in ref0 else 0.0
    for part in ref0:
        netlib.require_finite(part, WEIGHTED_KEYS, f"case {cs['i']}")
    return netlib.response(ref0, ref1, WEIGHTED_KEYS), 0.0


def admissible(cs):
    try:
        state, cov = sensitivity(cs)
    except (np.linalg.LinAlgError, FloatingPointError, ZeroDivisionError) as e:
        return False, f"{type(e).__name__}: {e}"
    return state <= bar(cs) / 16 and cov <= coverage_bar(cs) / 16, f"sensitivity {state:.2e} (bar {bar(cs):.0e}), coverage {cov}"


def describe(cs):
    return f"{cs['method']} T={cs['T']} passes={cs['passes']} d={cs['d']} r={cs['r']} {cs['storage']}"


# What `resolve` answers for the cases it does not leave alone, {i: (salt, times shortened)}: recorded here so that the device
# test need not run the oracle three times per case; tests/test_gram_cases_cpu.py recomputes every entry (and every absence).
RESOLUTION = {45: (1, 0), 50: (0, 1)}


def resolve(i):
    """netlib.resolve on this net (halving the horizon, with a pass less): ((salt, times shortened), log)"""
    return netlib.resolve(i, case, shorten, admissible, describe)


def device_case(i):
    return netlib.device_case(i, case, shorten, RESOLUTION.get(i, (0, 0)))
