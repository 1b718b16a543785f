// Batched multivariate Bayesian online change-point detection (the BOCPD baseline of the change-point experiment,
// ExperimentChange/MVBOCPD.m with its Student-t predictive and its constant hazard), float64 throughout.
//
// A hypothesis is named by its BIRTH step b (0-based): it starts as the prior (mu = 0, Sigma = sigma0 I) in front of step b and has
// absorbed x_b .. x_{t-1} when step t begins, so its age there is a = t - b, kappa = kappa0 + a, nu = nu0 + a.  Its (mu, L) chain,
// L the Cholesky factor of Sigma, depends on the data alone and never on the run-length posterior R.  Hence two phases:
//
//   psmf_bocpd_chain_kernel<DIM>   one LANE per birth, one workgroup per (series, block of NL consecutive births), grid = blocks x
//       series; NL = the most of 256, 128, 64, 32 lanes whose factors fit the LDS (64 at dim 20, 32 at dim 32).  The lane's L, packed
//       by columns, lives in LDS for the whole launch, element-major and lane-minor (element e of lane l at e * NL + l: consecutive
//       lanes hit consecutive 8-byte words, no bank conflict); mu and the two work vectors of a step are registers (one instance per
//       dim, every loop over coordinates unrolled: no scratch memory).
//       Per step t >= b, with delta = x_t - mu and one fused pass over the columns of L that reads and writes every entry once:
//         forward substitution  L z = delta                              (column k: z_k = u_k / L_kk, u_i -= L_ik z_k)
//         rank-one update       L L^T += coef delta delta^T              (column k: r = sqrt(L_kk^2 + w_k^2), c = r / L_kk, s = w_k / L_kk,
//                                                                         L_ik' = L_ik / c + (s / c) w_i, w_i <- w_i / c - (s / c) L_ik)
//       with coef = kappa / (2 (kappa + 1)), w = sqrt(coef) delta, and
//         log p = cst[a] - ld - (nu + dim) / 2 * log1p(coef |z|^2),      sc = nu coef,  sc |z|^2 / nu = coef |z|^2,  ld = sum_j log L_jj
//       where cst[a] = lgamma((nu + dim) / 2) - lgamma(nu / 2) + dim / 2 (log sc - log(nu pi)) comes from a host table (it depends on the
//       age alone) and ld is carried: det(Sigma + coef delta delta^T) = det(Sigma) (1 + coef |z|^2), so ld += log1p(coef |z|^2) / 2.
//       The update of w_i is the textbook's w_i <- c w_i - s L_ik' with c^2 - s^2 = 1 put in.  The textbook's form subtracts two products of
//       size s^2 w_i to get a result of size w_i / c.  With a sample at 1e100 under a unit prior the rounding of that difference, 1e184,
//       went into the next column, whose square overflowed: a finite series failed with PSMF_ERR_NUMERIC; and with data at 1e3 under a
//       unit prior it cost log p three of its digits (4e-9 against 3e-12 at dim 5).  This form has no such difference, and with 1 / c = L_kk / r and s / c = w_k / r
//       (both at most 1) as the column's constants no product exceeds its operands: a sample fails only where its own square overflows.
//       The operation count is the textbook's (a multiplication and a fused multiply-add for each of L_ik', w_i); measured against it
//       at T = 801: -2 % at dim 20, +3 % at dim 32, +4 % at dim 28, +8 % at dim 12, equal at dim 3 (docs/MEASUREMENTS.md).
//       log p goes to table[series][t][b] (lanes = consecutive b: coalesced).  x_t is the same for the whole workgroup.  All lanes of a
//       block but those of its first NL steps are busy; the blocks of a series differ in length (T - first birth), and with about
//       batch * T / NL of them against 256 CUs the dispatcher evens that out.  Hypotheses that a truncation discards later cost their
//       work and nothing else.
//   psmf_bocpd_post_kernel    one 256-thread workgroup per series: the recursion on R, serial in t, O(live) per step.  log R lives in LDS
//       indexed by birth -- nothing shifts when hypotheses age, and a truncation only raises the lower bound `lo`.  Per step: the MAP
//       run length of column t (argmax over the stored column, ties to the lowest age), v_b = log R_b + log p_b, M = max v,
//       S = sum exp(v - M), then log R'_b = v_b - M - log S + log(1 - h) and log R'_{t+1} = log h; the detection heuristic runs on
//       every thread from the broadcast argmax.  Three barriers per step.  A step at which every p underflows changes nothing: v stays
//       finite in the log domain.
//
// No atomics, no flags between workgroups; the error flag of a series is a plain store of 1 (every writer stores the same value).
// Limits: dim <= 32, T <= 4096.  Scratch (the table: T * T doubles per series) is allocated per call; a batch whose scratch does not fit
// what is free on the device is processed in chunks of series.
#include "psmf_host.h"        // Switches
#include "psmf_batch.h"       // EntryFail, open_device, plan_chunk, per-item slots, TimedLaunch, all_finite, replica_status

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace psmf {

constexpr int BOCPD_MAX_DIM = 32;
constexpr int BOCPD_MAX_T = 4096;
constexpr int BOCPD_POST_WG = 256;
constexpr size_t BOCPD_LDS_MAX = 160 * 1024;
constexpr long long BOCPD_MAX_TABLE_DOUBLES = 1LL << 28;      // want_R / want_logpred: 2 GiB of output each

struct BocpdParams {
  int dim, T, drop, settle, confirm, max_cp, want_R, want_lp;
  double kappa0, nu0, sqrt_sigma0, log_h, log_1mh;
  const double* X;        // series x T x dim
  const double* cst;      // T: the age-only part of log p
  double* table;          // series x T x T: [t][birth]
  int* map_run;           // series x T
  int* cps;               // series x max_cp
  int* ncp;               // series
  double* R_last;         // series x (T + 1) or null (zero-filled by the host)
  double* R;              // series x (T + 1) x (T + 1) or null (zero-filled by the host)
  double* logpred;        // series x T x T, [t][age], or null
  int* err;               // series: non-zero on entry = skip (non-finite input); set to 1 on a non-finite state
};

// lanes (= births) per workgroup of the chain kernel: the most of 256, 128, 64, 32 whose factors, dim (dim + 1) / 2 doubles a lane, fit the LDS
__host__ __device__ constexpr int bocpd_lanes(int dim) {
  const size_t lane_bytes = (size_t)(dim * (dim + 1) / 2) * 8;
  return 256 * lane_bytes <= BOCPD_LDS_MAX ? 256 : 128 * lane_bytes <= BOCPD_LDS_MAX ? 128 : 64 * lane_bytes <= BOCPD_LDS_MAX ? 64 : 32;
}

// One instance per dimension: every loop over coordinates is unrolled, so mu and the two work vectors of a step are registers (3 DIM
// doubles, no scratch memory), every LDS address of L is an immediate, and the compiler moves a column's loads ahead of the column
// before it (no column of L touches another).  What stays serial is the chain w_k -> 1 / r -> w_{k+1} from column to column; the
// reciprocals of the old diagonal stand outside it and the square root is taken as x rsqrt(x), so no division lies on it.
template <int DIM>
__global__ __launch_bounds__(bocpd_lanes(DIM) < 64 ? 64 : bocpd_lanes(DIM)) void psmf_bocpd_chain_kernel(BocpdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int NL = bocpd_lanes(DIM);
  const int T = p.T, lane = threadIdx.x, ser = blockIdx.y;
  const int b = blockIdx.x * NL + lane;              // this lane's birth
  if (p.err[ser] != 0) return;                       // the host found a non-finite sample: the series is skipped (uniform per workgroup)
  if (lane >= NL) return;                            // NL = 32: the upper half of the wave has no state
  double* sL = reinterpret_cast<double*>(smem_raw) + lane;      // element e of the packed columns at sL[e * NL]
  double mu[DIM], u[DIM], w[DIM];
  {
    int e = 0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      mu[k] = 0.0;
#pragma unroll
      for (int i = k; i < DIM; ++i, ++e) sL[e * NL] = i == k ? p.sqrt_sigma0 : 0.0;
    }
  }
  double ld = DIM * log(p.sqrt_sigma0);
  const double* X = p.X + (size_t)ser * T * DIM;
  double* tab = p.table + (size_t)ser * T * T;
  bool bad = false;
  const int t0 = blockIdx.x * NL;
  for (int t = t0; t < T; ++t) {
    if (b > t) continue;                             // not born yet (only in the block's first NL steps); b <= t < T from here
    const double* x = X + (size_t)t * DIM;
    const int a = t - b;
    const double kap = p.kappa0 + a, nu = p.nu0 + a;
    const double kinv = 1.0 / (kap + 1.0), coef = 0.5 * kap * kinv, sq = sqrt(coef);
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      const double xj = x[j], dl = xj - mu[j];
      mu[j] = (kap * mu[j] + xj) * kinv;
      u[j] = dl;
      w[j] = sq * dl;
    }
    double zz = 0.0;
    int e = 0;                                       // index of L_kk in the packed columns (a constant once unrolled)
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const double lkk = sL[e * NL];
      const double linv = 1.0 / lkk;
      const double zk = u[k] * linv;
      zz = fma(zk, zk, zz);
      const double r2 = fma(lkk, lkk, w[k] * w[k]);
      const double rinv = rsqrt(r2), r = r2 * rinv;
      const double cinv = lkk * rinv, sc = w[k] * rinv;      // 1 / c and s / c
      sL[e * NL] = r;
      ++e;
#pragma unroll
      for (int i = k + 1; i < DIM; ++i, ++e) {
        const double l = sL[e * NL];
        u[i] = fma(-l, zk, u[i]);
        sL[e * NL] = fma(sc, w[i], l * cinv);
        w[i] = fma(-sc, l, w[i] * cinv);             // = c w_i - s L_ik' (c^2 - s^2 = 1), without its cancellation: see above
      }
    }
    const double lq = log1p(coef * zz);              // sc |z|^2 / nu = coef |z|^2
    const double lp = p.cst[a] - ld - 0.5 * (nu + DIM) * lq;
    ld += 0.5 * lq;
    tab[(size_t)t * T + b] = lp;
    bad = bad || !isfinite(lp);                      // a non-finite state or a non-positive pivot shows here
  }
  if (bad) p.err[ser] = 1;                           // (benign race: every writer stores 1)
}

// max with the index of the maximum; on a tie the HIGHER index wins (index = birth: the lowest age)
struct BocpdMax { double v; int i; };
__device__ __forceinline__ BocpdMax bocpd_max2(BocpdMax x, BocpdMax y) {
  return (y.v > x.v || (y.v == x.v && y.i > x.i)) ? y : x;
}

__global__ __launch_bounds__(BOCPD_POST_WG) void psmf_bocpd_post_kernel(BocpdParams p) {
  __shared__ double slogR[BOCPD_MAX_T + 1];
  __shared__ double sred[2 * (BOCPD_POST_WG / 64)], ssums[BOCPD_POST_WG / 64];
  __shared__ int sredi[BOCPD_POST_WG / 64];
  constexpr int NW = BOCPD_POST_WG / 64;
  const int T = p.T, tid = threadIdx.x, ser = blockIdx.x, wv = tid >> 6, lane = tid & 63;
  if (p.err[ser] != 0) return;                       // skipped or failed series (uniform per workgroup): its outputs stay zero
  const double* tab = p.table + (size_t)ser * T * T;
  const double ninf = -INFINITY, qnan = __builtin_nan("");
  int lo = 0, lo_col = 0;                            // live births [lo, t]; the stored column t covers [lo_col, t]
  int flag = 0, cnt = 0, mprev = 0, ncp = 0;
  if (tid == 0) slogR[0] = 0.0;
  if (p.R && tid == 0) p.R[(size_t)ser * (T + 1) * (T + 1)] = 1.0;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const double* lp = tab + (size_t)t * T;
    // ---- MAP run length of column t, and M = max v over the live births ----
    BocpdMax am{ninf, -1};
    double vmax = ninf;
    for (int b = lo_col + tid; b <= t; b += BOCPD_POST_WG) {
      const double lr = slogR[b];
      am = bocpd_max2(am, BocpdMax{lr, b});
      if (b >= lo) vmax = fmax(vmax, lr + lp[b]);
    }
    for (int off = 32; off > 0; off >>= 1) {
      BocpdMax o{__shfl_xor(am.v, off, 64), __shfl_xor(am.i, off, 64)};
      am = bocpd_max2(am, o);
      vmax = fmax(vmax, __shfl_xor(vmax, off, 64));
    }
    if (lane == 0) { sred[wv] = am.v; sredi[wv] = am.i; sred[NW + wv] = vmax; }
    __syncthreads();
    am = BocpdMax{sred[0], sredi[0]};
    vmax = sred[NW];
    for (int w = 1; w < NW; ++w) { am = bocpd_max2(am, BocpdMax{sred[w], sredi[w]}); vmax = fmax(vmax, sred[NW + w]); }
    // ---- S = sum exp(v - M) ----
    double ssum = 0.0;
    for (int b = lo + tid; b <= t; b += BOCPD_POST_WG) ssum += exp(slogR[b] + lp[b] - vmax);
    for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off, 64);
    if (lane == 0) ssums[wv] = ssum;
    __syncthreads();                                 // (every read of column t by another thread lies in front of this barrier)
    ssum = ssums[0];
    for (int w = 1; w < NW; ++w) ssum += ssums[w];
    const double shift = p.log_1mh - vmax - log(ssum);
    if (p.logpred) {                                 // [t][age], NaN where not live
      double* o = p.logpred + ((size_t)ser * T + t) * T;
      for (int a = tid; a < T; a += BOCPD_POST_WG) o[a] = a <= t - lo ? lp[t - a] : qnan;
    }
    // ---- column t + 1 ----
    double* Rrow = p.R ? p.R + ((size_t)ser * (T + 1) + (t + 1)) * (T + 1) : nullptr;
    for (int b = lo + tid; b <= t; b += BOCPD_POST_WG) {
      const double v = slogR[b] + lp[b] + shift;
      slogR[b] = v;
      if (Rrow) Rrow[t + 1 - b] = exp(v);
    }
    if (tid == 0) {
      slogR[t + 1] = p.log_h;
      if (Rrow) Rrow[0] = exp(p.log_h);
    }
    lo_col = lo;                                     // column t + 1 holds births [lo, t + 1], whatever is discarded below
    // ---- detection heuristic (every thread, from the broadcast argmax) ----
    const int m = 1 + (t - am.i);
    if (tid == 0) p.map_run[(size_t)ser * T + t] = m;
    if (t > 0) {
      const int dm = m - mprev;
      if (dm < -p.drop) {
        flag = 1;
      } else if (flag) {
        if (abs(dm) < p.settle) {
          if (++cnt > p.confirm) {
            if (tid == 0 && ncp < p.max_cp) p.cps[(size_t)ser * p.max_cp + ncp] = (t + 1) - m + 1;
            ++ncp;
            flag = 0; cnt = 0;
            lo = max(lo, min(t + 1, t - m + 2));     // ages >= m - 1 are discarded: births < t - (m - 2)
          }
        } else {
          flag = 0; cnt = 0;
        }
      }
    }
    mprev = m;
    __syncthreads();                                 // column t + 1 is complete
  }
  if (p.R_last) {
    double* o = p.R_last + (size_t)ser * (T + 1);
    for (int b = lo_col + tid; b <= T; b += BOCPD_POST_WG) o[T - b] = exp(slogR[b]);
  }
  bool bad = false;
  for (int b = lo_col + tid; b <= T; b += BOCPD_POST_WG) bad = bad || !isfinite(slogR[b]);
  if (bad) p.err[ser] = 1;                           // (benign race: every writer stores 1)
  if (tid == 0) p.ncp[ser] = ncp;
}

namespace {

template <int DIM>
int bocpd_launch_chain(const EntryFail& fail, const BocpdParams& bp, int nser) {
  if constexpr (DIM > BOCPD_MAX_DIM) {
    return fail(PSMF_ERR_ARG, "no chain kernel for this dim");
  } else {
    if (bp.dim != DIM) return bocpd_launch_chain<DIM + 1>(fail, bp, nser);
    constexpr int NL = bocpd_lanes(DIM);
    constexpr size_t lds = (size_t)(DIM * (DIM + 1) / 2) * sizeof(double) * NL;
    static_assert(lds <= BOCPD_LDS_MAX, "the factors of a workgroup's lanes fit the LDS");
    const void* kern = (const void*)psmf_bocpd_chain_kernel<DIM>;
    PSMF_TRY(lds_opt_in(fail, kern, lds));
    BocpdParams q = bp;
    return launch(fail, kern, dim3((bp.T + NL - 1) / NL, nser), dim3(NL < 64 ? 64 : NL), &q, lds);
  }
}

int bocpd_run(const psmf_bocpd_config* cfg, const double* X, int32_t* map_run, int32_t* changepoints, int32_t* n_changepoints,
              double* R_last, double* R, double* logpred, int32_t* status, float* elapsed_ms) {
  const EntryFail fail{"psmf_bocpd_run"};
  const Switches sw;      // no handle here: read at entry, on every call
  if (!cfg || !X || !map_run || !n_changepoints) return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const int dim = cfg->dim, T = cfg->T, B = cfg->batch, maxcp = cfg->max_changepoints;
  if (dim < 1 || dim > BOCPD_MAX_DIM) return fail(PSMF_ERR_ARG, "need 1 <= dim <= 32 (a lane holds the hypothesis' factor in LDS; dim = " + std::to_string(dim) + ")");
  if (T < 1 || T > BOCPD_MAX_T) return fail(PSMF_ERR_ARG, "need 1 <= T <= 4096 (the run-length column lives in LDS; T = " + std::to_string(T) + ")");
  if (B < 1) return fail(PSMF_ERR_ARG, "need batch >= 1 (batch = " + std::to_string(B) + ")");
  if (!std::isfinite(cfg->lambda) || !(cfg->lambda > 1.0)) return fail(PSMF_ERR_ARG, "need a finite lambda > 1 (the hazard is h = 1 / lambda, 0 < h < 1)");
  if (!std::isfinite(cfg->kappa0) || !(cfg->kappa0 > 0.0)) return fail(PSMF_ERR_ARG, "need a finite kappa0 > 0");
  if (!std::isfinite(cfg->nu0) || !(cfg->nu0 > dim - 1.0)) return fail(PSMF_ERR_ARG, "need a finite nu0 > dim - 1 (nu0 = " + std::to_string(cfg->nu0) + ", dim = " + std::to_string(dim) + ")");
  if (!std::isfinite(cfg->sigma0) || !(cfg->sigma0 > 0.0)) return fail(PSMF_ERR_ARG, "need a finite sigma0 > 0 (Sigma0 = sigma0 I)");
  if (cfg->drop < 0 || cfg->settle < 0 || cfg->confirm < 0) return fail(PSMF_ERR_ARG, "drop, settle and confirm must be >= 0");
  if (maxcp < 0 || (maxcp > 0 && !changepoints)) return fail(PSMF_ERR_ARG, "max_changepoints must be >= 0, and > 0 needs changepoints");
  if (sw.bocpd_chunk < 0) return fail(PSMF_ERR_ARG, "PSMF_BOCPD_CHUNK must be >= 0 (series per chunk; 0 = sized from free memory)");
  if (cfg->want_R && !R) return fail(PSMF_ERR_ARG, "want_R needs R");
  if (cfg->want_logpred && !logpred) return fail(PSMF_ERR_ARG, "want_logpred needs logpred");
  if (cfg->want_R && (long long)B * (T + 1) * (T + 1) > BOCPD_MAX_TABLE_DOUBLES)
    return fail(PSMF_ERR_ARG, "want_R: batch x (T + 1) x (T + 1) exceeds the limit of 2^28 doubles (2 GiB)");
  if (cfg->want_logpred && (long long)B * T * T > BOCPD_MAX_TABLE_DOUBLES)
    return fail(PSMF_ERR_ARG, "want_logpred: batch x T x T exceeds the limit of 2^28 doubles (2 GiB)");
  const bool wantR = cfg->want_R != 0, wantLp = cfg->want_logpred != 0;

  // the age-only part of log p, and which series hold a non-finite sample
  std::vector<double> cst(T);
  for (int a = 0; a < T; ++a) {
    const double kap = cfg->kappa0 + a, nu = cfg->nu0 + a, sc = nu * kap / (2.0 * (kap + 1.0));
    cst[a] = std::lgamma(0.5 * (nu + dim)) - std::lgamma(0.5 * nu) + 0.5 * dim * (std::log(sc) - std::log(nu * M_PI));
  }
  std::vector<int> herr(B, 0);
  for (int b = 0; b < B; ++b)
    if (!all_finite(X + (size_t)b * T * dim, (size_t)T * dim)) herr[b] = 1;
  PSMF_TRY(open_device(fail, cfg->device));

  // series per chunk (PSMF_BOCPD_CHUNK: smaller chunks than memory asks for)
  const size_t per_series = ((size_t)T * T + (size_t)T * dim + (wantR ? (size_t)(T + 1) * (T + 1) : 0) + (wantLp ? (size_t)T * T : 0) + (T + 1)) * sizeof(double) +
                            ((size_t)T + maxcp + 2) * sizeof(int);
  int chunk = 0;
  PSMF_TRY(plan_chunk(fail, B, 0, per_series, kNoItemCap, sw.bocpd_chunk, "series", &chunk));

  Dev<double> dX, dCst, dTab, dRl, dR, dLp;
  Dev<int> dMap, dCp, dNcp, dErr;
  TimedLaunch timed;
  const size_t nX = (size_t)T * dim, nTab = (size_t)T * T, nR = (size_t)(T + 1) * (T + 1), nRl = (size_t)T + 1, nT = T, nCp = maxcp;
  const auto items = std::make_tuple(      // buffer, filled from, read back to, elements per series, cleared for every chunk
      item_slot(dX, X, nullptr, nX), item_slot(dTab, nullptr, nullptr, nTab), item_slot(dMap, nullptr, map_run, nT, true),
      item_slot(dCp, nullptr, changepoints, nCp, true, 1),      // (one element more: max_changepoints may be 0)
      item_slot(dNcp, nullptr, n_changepoints, 1, true), item_slot(dErr, herr.data(), herr.data(), 1),
      item_slot(dRl, nullptr, R_last, R_last ? nRl : 0, true), item_slot(dR, nullptr, R, wantR ? nR : 0, true),
      item_slot(dLp, nullptr, logpred, wantLp ? nTab : 0, true));
  const auto shared = std::make_tuple(slot(dCst, cst.data(), nullptr, nT));      // what every chunk shares, filled once
  PSMF_TRY(alloc_all(fail, shared));
  PSMF_TRY(alloc_items(fail, items, chunk));
  PSMF_TRY(copy_in_all(fail, shared));
  PSMF_TRY(timed.create(fail));

  BocpdParams bp;
  bp.dim = dim; bp.T = T; bp.drop = cfg->drop; bp.settle = cfg->settle; bp.confirm = cfg->confirm; bp.max_cp = maxcp;
  bp.want_R = wantR; bp.want_lp = wantLp;
  bp.kappa0 = cfg->kappa0; bp.nu0 = cfg->nu0; bp.sqrt_sigma0 = std::sqrt(cfg->sigma0);
  bp.log_h = -std::log(cfg->lambda); bp.log_1mh = std::log1p(-1.0 / cfg->lambda);
  bp.X = dX; bp.cst = dCst; bp.table = dTab; bp.map_run = dMap; bp.cps = dCp; bp.ncp = dNcp;
  bp.R_last = R_last ? dRl.get() : nullptr; bp.R = wantR ? dR.get() : nullptr; bp.logpred = wantLp ? dLp.get() : nullptr; bp.err = dErr;

  float total_ms = 0.0f;
  for (int s0 = 0; s0 < B; s0 += chunk) {      // s0: the chunk's first series = its element offset in the host arrays, per series
    const size_t ns = std::min(chunk, B - s0);
    PSMF_TRY(fill_items(fail, items, s0, ns));
    PSMF_TRY(timed.start(fail));
    PSMF_TRY(bocpd_launch_chain<1>(fail, bp, (int)ns));      // the instance of this dim
    PSMF_TRY(launch(fail, (const void*)psmf_bocpd_post_kernel, dim3((unsigned)ns), dim3(BOCPD_POST_WG), &bp, 0));
    float ms = 0.0f;
    PSMF_TRY(timed.finish(fail, &ms));
    total_ms += ms;
    PSMF_TRY(read_items(fail, items, s0, ns));
  }
  if (elapsed_ms) *elapsed_ms = total_ms;
  // Per-replica outcome, as psmf_ssm_run; the other replicas are untouched by a bad one.
  return replica_status(fail, B, status, [&](int b) { return herr[b] != 0; }, [](int b) {
    return "non-finite input, a non-finite state or a non-positive pivot in replica " + std::to_string(b);
  });
}

}  // namespace
}  // namespace psmf

extern "C" int psmf_bocpd_run(const psmf_bocpd_config* cfg, const double* X, int32_t* map_run, int32_t* changepoints, int32_t* n_changepoints,
                              double* R_last, double* R, double* logpred, int32_t* status, float* elapsed_ms) {
  return psmf::bocpd_run(cfg, X, map_run, changepoints, n_changepoints, R_last, R, logpred, status, elapsed_ms);
}
