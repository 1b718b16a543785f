// Batched PSMF with linear-Gaussian dynamics and an observation map: the filter of the change-point experiment
//   PSMF                                      ExperimentChange/PSMF.m:6-45 (driven by ExperimentChange/main.m)
// for a whole batch of independent series.  The latent state x has its own dimension p >= r, moves by a linear map A (p x p) with
// process noise Q and reaches the dictionary through an observation map H (r x p): y ~ C H x.  A, Q, H and rho (R = rho I) are shared
// by the replicas; Y, C, V, x, P are per replica.  Per step
//   xbar = A x,  Pbar = A P_prev A^T + Q       (carry_P = 0: P_prev = P0 at the first step of a series, 0 afterwards -- PSMF.m:30 as written)
//   z = H xbar, w = V z, s = z^T w, yhat = C z, e = y - yhat,  P_z = H Pbar H^T,  S = C P_z C^T + (rho + s) I
//   x = xbar + Pbar H^T C^T S^-1 e,  P = Pbar - Pbar H^T C^T S^-1 C H Pbar
//   eta = trace(C P_z C^T + rho I) / d,  N = s + eta,  C += e w^T / N,  V -= w w^T / N
// No d x d matrix is formed.  With G = C^T C, h = C^T e, kappa = 1 / (rho + s):
//   P_z+ = (P_z^-1 + kappa G)^-1        two symmetric sweep inversions (wave_sweep16m), the first beside the Gram
//   B = P_z^-1 P_z+ = I - kappa G P_z+  formed as the PRODUCT: the textbook W = kappa G - kappa^2 G P_z+ G cancels 1e3-fold where rho
//                                       is small against C P_z C^T (the experiment's rho = 1e-3 with P0 = I)
//   u = kappa B h = C^T S^-1 e,  W = kappa sym(B G) = C^T S^-1 C,  eta = <G, P_z> / d + rho
//   x = xbar + Pbar H^T u,  P = Pbar - (Pbar H^T) W (Pbar H^T)^T
// One 256-thread workgroup per replica, grid = batch; C, V, x, P, Pbar and the shared A, Q, H live in LDS in float64 for the whole
// call (rows zero-padded: r to 16, p to 32, d to a multiple of 4), y_{t+1} is prefetched while step t runs, X[t], yhat and (s, eta)
// are stored from LDS, and the barriers inside the step loop order LDS only (solve_barrier<true>): the prefetch and the stores stay
// in flight across them.  G and h come from the augmented [C | e] product on the float64 matrix cores, recomputed every step, as in
// psmf_impute2.hip; the p x p and p x r products of the step (A P_prev, its product with A^T, Pbar H^T, its product with W, the update
// of P) run there too, one 16 x 16 output tile per wave.  Limits: d <= 512, r <= 16, r <= p <= 32.
#include "psmf_host.h"        // WG and the device headers
#include "psmf_batch.h"       // EntryFail, open_device, typed transfers, TimedLaunch, all_finite, replica_status
#include "psmf_sweep.h"       // solve_barrier
#include "psmf_wave16.hip"    // wave_sweep16m, Sw16K

#include <cmath>
#include <type_traits>
#include <string>
#include <vector>

namespace psmf {

constexpr int SR = 16;       // padded r
constexpr int SP = 32;       // padded p
constexpr int SLA = 33;      // row stride of A, H and the p x p matrices in LDS (read down a column by consecutive lanes)
constexpr int SLH = 17;      // row stride of Pbar H^T and of (Pbar H^T) W

struct SsmParams {
  int d, n, r, p, carry_P, first_step;
  double rho;
  const double* Y;         // batch x n x d
  double* C;               // batch x d x r
  double* V;               // batch x r x r
  double* x;               // batch x p
  double* P;               // batch x p x p
  const double* A;         // p x p (shared)
  const double* Q;         // p x p
  const double* H;         // r x p
  double* X;               // batch x n x p
  double* Ypred;           // batch x n x d or null
  double* scal;            // batch x n x 2 or null
  int* err;                // batch
};

// what the robust and the masked instances take beside it
struct SsmParamsEx : SsmParams {
  const unsigned char* mask;   // batch x n x d, 1 = observed (masked instances)
  double* rstate;              // batch x 2: (lambda, Omega) in / out (robust instances)
  double lambda0, alpha, beta;
  int fixed_lambda;
};

__host__ __device__ inline size_t ssm_lds_doubles(int d) {
  const size_t d4 = ((size_t)d + 3) & ~(size_t)3;
  return d4 * SR + SR * SR                 // C, V
         + 2 * (size_t)SP * SLA            // A, H (H uses SR rows of it)
         + 3 * (size_t)SP * SLA            // Q, P, Pbar
         + 3 * 2 * 256                     // A P_prev (phases 1-2), the Gram partials of waves 1-3 (5-6), (Pbar H^T) W (9-10)
         + (size_t)SP * SLH                // Pbar H^T
         + 7 * (size_t)SR * SR             // P_z, P_z^-1, P_z+, G, B, W, (spare)
         + 2 * SP + 5 * SR                 // x, xbar, z, w, h, u, (spare)
         + 2 * d4                          // e, yhat
         + 8 + 2;                          // scalars, error flag
}
inline size_t ssm_lds_bytes(int d) { return (ssm_lds_doubles(d) * 8 + 15) & ~(size_t)15; }
// the masked instances keep the step's mask column in front of it, a byte per row (at a fixed place: 512 bytes whatever d is)
constexpr int SSM_MASK_BYTES = 2 * WG;
inline size_t ssm_lds_bytes(int d, bool masked) { return ssm_lds_bytes(d) + (masked ? SSM_MASK_BYTES : 0); }

__device__ __forceinline__ void ssm_barrier() { solve_barrier<true>(); }

// ROB: rPSMF (ExperimentImpute/rPSMF.py:75-135, pypsmf/psmf/rpsmf.py:125-172).  Omega is the running product of omega (Q and rho are
// scaled by it), lambda the degrees of freedom:
//   Pbar = A P_prev A^T + Omega Q,  rho_t = Omega rho,  omega = (lambda + e^T S^-1 e) / (lambda + d),  P = beta omega (...)
//   phi = (lambda + e^T e / N) / (lambda + d),  V = alpha phi (V - w w^T / N),  Omega <- omega Omega,  lambda <- lambda + d unless fixed
// with e^T S^-1 e = kappa e^T e - kappa^2 h^T P_z+ h (S^-1 = kappa I - kappa^2 C_m P_z+ C_m^T).
// MSK: a 0/1 mask column m per step (a byte per row, prefetched with y): e_i = m_i (y_i - yhat_i) by selection, so that a NaN under a
// zero never enters; G = sum m_i c_i c_i^T, h = sum m_i c_i e_i (the mask multiplies the Gram's operand);
// eta = (rho_t sum m_i + <G, P_z>) / d; S keeps s I on every row (rPSMF.py:97-98), and yhat is written for every row.
// sum m_i is counted by ballot in phase 3; e^T e is reduced beside the Gram in phase 5 (waves 1-3), so phi is there for the update of V
// in phase 7; omega comes from wave 2, idle in phase 9, ahead of the store of P in phase 10 and of the next step's Omega Q and rho_t:
// the step has the plain instance's ten barriers and not one more.  With both off the step loop is the plain one, statement for statement.
template <bool ROB, bool MSK>
__global__ __launch_bounds__(WG) void psmf_ssm_kernel(typename std::conditional<ROB || MSK, SsmParamsEx, SsmParams>::type p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sm = reinterpret_cast<double*>(smem_raw + (MSK ? SSM_MASK_BYTES : 0));
  const int d = p.d, n = p.n, r = p.r, np = p.p, tid = threadIdx.x, rep = blockIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, lk = lane >> 4, lr = lane & 15;
  const int d4 = (d + 3) & ~3, p4 = (np + 3) & ~3;
  // ---- LDS carve (doubles); every padding entry is zero and stays zero ----
  double* sC = sm;                           // d4 x SR
  double* sV = sC + (size_t)d4 * SR;         // SR x SR
  double* sA = sV + SR * SR;                 // SP x SLA
  double* sH = sA + SP * SLA;                // SR x SLA
  double* sQ = sH + SP * SLA;                // SP x SLA each from here
  double* sP = sQ + SP * SLA;                // P_{t-1} / P_t
  double* sPb = sP + SP * SLA;               // Pbar
  double* sT = sPb + SP * SLA;               // 1536: A P_prev (row stride SLA) in phases 1-2; (Pbar H^T) W with row stride SLH in phases 9-10
  double* sgp = sT;                          // ... and in phases 5-6 the Gram partials, 3 waves x 2 tiles x 256 in the MFMA output layout
  double* sPH = sT + 3 * 2 * 256;            // SP x SLH: Pbar H^T
  double* sPz = sPH + SP * SLH;              // SR x SR each from here
  double* sPzi = sPz + SR * SR;
  double* sPp = sPzi + SR * SR;
  double* sG = sPp + SR * SR;
  double* sB = sG + SR * SR;
  double* sW = sB + SR * SR;
  double* sx = sW + 2 * SR * SR;             // SP
  double* sxb = sx + SP;                     // SP
  double* sz = sxb + SP;                     // SR each from here
  double* sw = sz + SR;
  double* sh = sw + SR;
  double* su = sh + SR;
  double* se = su + 2 * SR;                  // d4
  double* syh = se + d4;                     // d4
  double* ssc = syh + d4;                    // 8 scalars: 0 s, 1 eta, 2 N, 3 kappa
  int* errflag = reinterpret_cast<int*>(ssc + 8);
  double* sxt = su + SR;                     // (the spare vector) robust / masked instances: 0-2 e^T e of waves 1-3, 3 omega, 4-7 sum m_i per wave, 8-9 the next lambda, 1 / (lambda + d)
  unsigned char* smk = reinterpret_cast<unsigned char*>(smem_raw);      // masked instances: the mask column of the step, 512 bytes

  const double* Yg = p.Y + (size_t)rep * n * d;
  double* Cg = p.C + (size_t)rep * d * r;
  double* Vg = p.V + (size_t)rep * r * r;
  double* xg = p.x + (size_t)rep * np;
  double* Pg = p.P + (size_t)rep * np * np;
  double* Xg = p.X + (size_t)rep * n * np;

  {
    const int total = (int)ssm_lds_doubles(d);
    for (int idx = tid; idx < total; idx += WG) sm[idx] = 0.0;
    if constexpr (MSK)
      for (int idx = tid; idx < SSM_MASK_BYTES; idx += WG) smk[idx] = 0;
  }
  __syncthreads();
  for (int idx = tid; idx < d * r; idx += WG) { const int i = idx / r, l = idx - i * r; sC[i * SR + l] = Cg[idx]; }
  for (int idx = tid; idx < r * r; idx += WG) { const int i = idx / r, l = idx - i * r; sV[i * SR + l] = Vg[idx]; }
  for (int idx = tid; idx < np * np; idx += WG) {
    const int i = idx / np, l = idx - i * np;
    sA[i * SLA + l] = p.A[idx];
    sQ[i * SLA + l] = p.Q[idx];
    sP[i * SLA + l] = Pg[idx];
  }
  for (int idx = tid; idx < r * np; idx += WG) { const int i = idx / np, l = idx - i * np; sH[i * SLA + l] = p.H[idx]; }
  if (tid < np) sx[tid] = xg[tid];
  const double rho = p.rho, idd = 1.0 / (double)d;
  const bool one_tile = r < 16;       // the augmented column e fits the 16 x 16 tile
  const int r2 = r + (r & 1);         // sweep size: even, identity-padded
  bool inq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) inq[q] = (lk + 4 * q) < r && lr < r;
  Sw16K swk;
  if (wv == 0) sw16k_init(swk, lk, lr);
  bool bad = false;
  double A1[4] = {0.0, 0.0, 0.0, 0.0}, Pzr[4] = {0.0, 0.0, 0.0, 0.0}, s = 0.0, kappa = 0.0;      // wave 0: -P_z^-1, P_z, s, kappa of the step
  // prefetch row 0 of the series: unconditional loads (row index clamped, value used only where the row exists)
  int rowc[2];
  double ny[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    rowc[u] = min(tid + u * WG, d - 1);
    ny[u] = Yg[rowc[u]];
  }
  // the mask column of a step stands in LDS (smk): the one of step t + 1 is prefetched beside y's row t + 1 and replaces it in phase 10,
  // which no longer reads the present one (phases 3 and 5 do)
  const unsigned char* Mg = nullptr;
  if constexpr (MSK) {
    Mg = p.mask + (size_t)rep * n * d;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (tid + u * WG < d) smk[tid + u * WG] = Mg[tid + u * WG];
  }
  if constexpr (ROB)       // Omega, lambda and 1 / (lambda + d) of the step: ssc[4-6], moved on by one thread in phase 10 (nobody reads them there)
    if (tid == 0) {
      ssc[4] = p.first_step ? 1.0 : p.rstate[2 * rep + 1];
      ssc[5] = p.first_step ? p.lambda0 : p.rstate[2 * rep];
      ssc[6] = 1.0 / (ssc[5] + (double)d);
    }
  // The p x p products run on the float64 matrix cores, one 16 x 16 output tile per wave (first row ti, first column tj): the A operand
  // of v_mfma_f64_16x16x4_f64 is element (row lr, k-slot lk), the B operand (k-slot lk, column lr), the result rows lk + 4 q of column
  // lr.  The p x r products (Pbar H^T, its product with W) are the two tiles of waves 0 and 1.  Of the r x r products a thread forms
  // the element (rk0, rc).
  const int ti = (wv >> 1) << 4, tj = (wv & 1) << 4;
  const int rc = tid & 15, rk0 = tid >> 4;
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    double yv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) yv[u] = ny[u];
    {
      const size_t base = (size_t)min(t + 1, n - 1) * d;      // (the last row is simply loaded twice)
#pragma unroll
      for (int u = 0; u < 2; ++u) ny[u] = Yg[base + rowc[u]];
    }
    unsigned char nm[2] = {1, 1};
    if constexpr (MSK) {
      const unsigned char* mrow = Mg + (size_t)min(t + 1, n - 1) * d;
#pragma unroll
      for (int u = 0; u < 2; ++u) nm[u] = mrow[(unsigned)rowc[u]];
    }
    const bool usep = p.carry_P || (p.first_step && t == 0);      // else P_prev = 0: Pbar = Q
    if constexpr (ROB || MSK) {       // wave 0's values of phases 5-6 hold no registers outside them: these instances have none to spare
#pragma unroll
      for (int q = 0; q < 4; ++q) A1[q] = Pzr[q] = 0.0;
      s = kappa = 0.0;
    }
    // ---- phase 1: T = A P_prev; xbar = A x ----
    if (usep) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < p4; kk += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[(ti + lr) * SLA + kk + lk], sP[(kk + lk) * SLA + tj + lr], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) sT[(ti + lk + 4 * q) * SLA + tj + lr] = acc[q];
    }
    if (wv == 3 && lane < SP) {
      double a = 0.0;
#pragma unroll 4
      for (int k = 0; k < p4; ++k) a = fma(sA[lane * SLA + k], sx[k], a);
      sxb[lane] = a;
    }
    ssm_barrier();
    // ---- phase 2: Pbar = T A^T + Q; z = H xbar ----
    {
      f64x4 acc;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = ROB ? ssc[4] * sQ[(ti + lk + 4 * q) * SLA + tj + lr] : sQ[(ti + lk + 4 * q) * SLA + tj + lr];
      if (usep)
        for (int kk = 0; kk < p4; kk += 4)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sT[(ti + lr) * SLA + kk + lk], sA[(tj + lr) * SLA + kk + lk], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) sPb[(ti + lk + 4 * q) * SLA + tj + lr] = acc[q];
    }
    if (wv == 3 && lane < SR) {
      double a = 0.0;
#pragma unroll 4
      for (int k = 0; k < p4; ++k) a = fma(sH[lane * SLA + k], sxb[k], a);
      sz[lane] = a;
    }
    ssm_barrier();
    // ---- phase 3: Pbar H^T; w = V z; yhat = C z, e = y - yhat (a row per thread, two when d > 256) ----
    if (wv < 2) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < p4; kk += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sPb[(16 * wv + lr) * SLA + kk + lk], sH[lr * SLA + kk + lk], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) sPH[(16 * wv + lk + 4 * q) * SLH + lr] = acc[q];
    }
    if (wv == 3 && lane < SR) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int l = 0; l < SR; l += 2) { a0 = fma(sV[lane * SR + l], sz[l], a0); a1 = fma(sV[lane * SR + l + 1], sz[l + 1], a1); }
      sw[lane] = a0 + a1;
    }
    int nobs = 0;       // masked instances: the observed rows of this wave
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * WG;
      if constexpr (MSK) nobs += __popcll(__ballot(i < d && smk[i] != 0));
      if (i < d) {
        double cr[SR], zr[SR];
#pragma unroll
        for (int l = 0; l < SR; ++l) { cr[l] = sC[i * SR + l]; zr[l] = sz[l]; }
        double d0 = 0.0, d1 = 0.0;
#pragma unroll
        for (int l = 0; l < SR; l += 2) { d0 = fma(cr[l], zr[l], d0); d1 = fma(cr[l + 1], zr[l + 1], d1); }
        const double dot = d0 + d1;
        syh[i] = dot;
        if constexpr (MSK) {
          se[i] = smk[i] ? yv[u] - dot : 0.0;
          if (lane == 0) sxt[4 + wv] = (double)nobs;       // (with u = 1 the sum of both halves)
        } else {
          se[i] = yv[u] - dot;
        }
      }
    }
    ssm_barrier();
    // ---- phase 4: P_z = H (Pbar H^T), one element per thread ----
    {
      double a = 0.0;
#pragma unroll 4
      for (int k = 0; k < p4; ++k) a = fma(sH[rk0 * SLA + k], sPH[k * SLH + rc], a);
      sPz[rk0 * SR + rc] = a;
    }
    ssm_barrier();
    // ---- phase 5: wave 0: s, kappa, -P_z^-1 (needs no Gram); waves 1-3: the augmented Gram [C | e]^T [C | e] on the matrix cores ----
    if (wv == 0) {
      s = wave_sum_f64_dpp(lane < SR ? sz[lane & 15] * sw[lane & 15] : 0.0);
      kappa = fast_rcp((ROB ? ssc[4] * rho : rho) + s);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = lk + 4 * q;
        Pzr[q] = inq[q] ? 0.5 * (sPz[i * SR + lr] + sPz[lr * SR + i]) : 0.0;
        A1[q] = inq[q] ? Pzr[q] : (i == lr ? 1.0 : 0.0);
      }
      wave_sweep16m(A1, r2, swk, bad);          // -P_z^-1
#pragma unroll
      for (int q = 0; q < 4; ++q) sPzi[(lk + 4 * q) * SR + lr] = inq[q] ? -A1[q] : 0.0;
    } else {
      if constexpr (ROB)       // the next step's lambda and 1 / (lambda + d), in the shorter half of the phase; phase 10 moves them in
        if (tid == 192) {
          const double ln = p.fixed_lambda ? ssc[5] : ssc[5] + (double)d;
          sxt[8] = ln;
          sxt[9] = 1.0 / (ln + (double)d);
        }
      f64x4 acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
      double ee = 0.0;       // robust: this wave's share of e^T e, beside the Gram (wave 0's inversion is the longer half of the phase)
      const int ngrp = d4 >> 2;
      for (int g = wv - 1; g < ngrp; g += 3) {
        const int k = 4 * g + lk;                                     // < d4: padding rows hold zeros
        const double cval = MSK ? sC[k * SR + lr] * (smk[k] ? 1.0 : 0.0) : sC[k * SR + lr], ek = se[k];
        const double a = cval + ((one_tile && lr == r) ? ek : 0.0);   // augmented column r: e (C is zero there)
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc1, 0, 0, 0);
        if (!one_tile) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lr == 0 ? ek : 0.0, acc2, 0, 0, 0);
        if constexpr (ROB) ee = fma(lr == 0 ? ek : 0.0, ek, ee);
      }
      if constexpr (ROB) {
        ee = wave_sum_f64_dpp(ee);
        if (lane == 0) sxt[wv - 1] = ee;
      }
      double* o = sgp + (size_t)(wv - 1) * 512;
#pragma unroll
      for (int q = 0; q < 4; ++q) { o[q * 64 + lane] = acc1[q]; o[256 + q * 64 + lane] = acc2[q]; }
    }
    ssm_barrier();
    // ---- phase 6: wave 0: G, eta, N, P_z+ = (P_z^-1 + kappa G)^-1; waves 1-3: G and h row-major ----
    if (wv == 0) {
      double G[4], tr = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double g0 = (sgp[q * 64 + lane] + sgp[512 + q * 64 + lane]) + sgp[1024 + q * 64 + lane];
        G[q] = inq[q] ? g0 : 0.0;
        tr += G[q] * Pzr[q];
      }
      const double rho_t = ROB ? ssc[4] * rho : rho;
      double eta;
      if constexpr (MSK) {
        const double cnt = (sxt[4] + sxt[5]) + (sxt[6] + sxt[7]);       // sum m_i
        eta = fma(wave_sum_f64_dpp(tr), idd, cnt == (double)d ? rho_t : rho_t * (cnt * idd));
      } else {
        eta = fma(wave_sum_f64_dpp(tr), idd, rho_t);
      }
      if (lane == 0) { ssc[0] = s; ssc[1] = eta; ssc[2] = s + eta; ssc[3] = kappa; }
      double A2[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) A2[q] = inq[q] ? kappa * G[q] - A1[q] : ((lk + 4 * q) == lr ? 1.0 : 0.0);
      wave_sweep16m(A2, r2, swk, bad);          // -P_z+
#pragma unroll
      for (int q = 0; q < 4; ++q) sPp[(lk + 4 * q) * SR + lr] = inq[q] ? -A2[q] : 0.0;
    } else {
      const int hc = one_tile ? r : 0, ht = one_tile ? 0 : 256;      // where h sits: column r of the tile / column 0 of the second one
      for (int idx = tid - 64; idx < 256; idx += WG - 64) {
        const int q = idx >> 6, l = idx & 63, i = (l >> 4) + 4 * q, c = l & 15;
        const double g0 = (sgp[idx] + sgp[512 + idx]) + sgp[1024 + idx];
        sG[i * SR + c] = (i < r && c < r) ? g0 : 0.0;
        if (c == hc) {
          const double h0 = (sgp[ht + idx] + sgp[512 + ht + idx]) + sgp[1024 + ht + idx];
          sh[i] = i < r ? h0 : 0.0;
        }
      }
    }
    ssm_barrier();
    // ---- phase 7: B = P_z^-1 P_z+; rank-1 updates of C and V (they need N, e, w only) ----
    {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int k = 0; k < SR; k += 2) {
        a0 = fma(sPzi[rk0 * SR + k], sPp[k * SR + rc], a0);
        a1 = fma(sPzi[rk0 * SR + k + 1], sPp[(k + 1) * SR + rc], a1);
      }
      sB[rk0 * SR + rc] = a0 + a1;
      const double wsc = fast_rcp(ssc[2]);
      for (int idx = tid; idx < d * SR; idx += WG) {       // (padding columns: w is zero there)
        const int i = idx >> 4, l = idx & 15;
        sC[idx] = fma(se[i], sw[l] * wsc, sC[idx]);
      }
      if constexpr (ROB) {
        const double phi = fma((sxt[0] + sxt[1]) + sxt[2], wsc, ssc[5]) * ssc[6];
        // w_i w_j first: the same bits at (i, j) and (j, i), so a symmetric V stays symmetric to the bit.  (w_i / N) w_j leaves an
        // antisymmetric part of an ulp per step, which the update never contracts (w w^T is symmetric) while phi and the projections
        // take the symmetric part down by ten orders: 1.3e-8 in V against the d x d model at d = 246, r = 3, lambda = 50 fixed with
        // steps of one observed row.  The instances that are not robust keep their statement (the plain one's code is unchanged).
        sV[rk0 * SR + rc] = (p.alpha * phi) * fma(-(sw[rk0] * sw[rc]), wsc, sV[rk0 * SR + rc]);
        if (tid == 64) ssc[7] = phi;
      } else {
        sV[rk0 * SR + rc] = fma(-sw[rk0] * wsc, sw[rc], sV[rk0 * SR + rc]);
      }
    }
    ssm_barrier();
    // ---- phase 8: W = kappa sym(B G), u = kappa B h ----
    {
      const double kap = ssc[3];
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int k = 0; k < SR; ++k) {
        a0 = fma(sB[rk0 * SR + k], sG[k * SR + rc], a0);
        a1 = fma(sB[rc * SR + k], sG[k * SR + rk0], a1);
      }
      sW[rk0 * SR + rc] = 0.5 * kap * (a0 + a1);
      if (wv == 3 && lane < SR) {
        double b0 = 0.0, b1 = 0.0;
#pragma unroll
        for (int k = 0; k < SR; k += 2) { b0 = fma(sB[lane * SR + k], sh[k], b0); b1 = fma(sB[lane * SR + k + 1], sh[k + 1], b1); }
        su[lane] = kap * (b0 + b1);
      }
    }
    ssm_barrier();
    // ---- phase 9: x = xbar + (Pbar H^T) u; T2 = (Pbar H^T) W ----
    if (wv == 3 && lane < SP) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < SR; c += 2) { a0 = fma(sPH[lane * SLH + c], su[c], a0); a1 = fma(sPH[lane * SLH + c + 1], su[c + 1], a1); }
      const double xn = sxb[lane] + (a0 + a1);
      bad |= !isfinite(xn);
      sx[lane] = xn;                             // (rows >= p of Pbar H^T and of xbar are zero)
    }
    if constexpr (ROB)
      if (wv == 2) {       // (the idle wave of this phase) omega = (lambda + kappa e^T e - kappa^2 h^T P_z+ h) / (lambda + d)
        double b0 = 0.0, b1 = 0.0;
        const int i = lane & 15;
#pragma unroll
        for (int k = 0; k < SR; k += 2) { b0 = fma(sPp[i * SR + k], sh[k], b0); b1 = fma(sPp[i * SR + k + 1], sh[k + 1], b1); }
        const double hph = wave_sum_f64_dpp(lane < SR ? sh[i] * (b0 + b1) : 0.0);
        const double kap = ssc[3];
        const double om = (ssc[5] + kap * (((sxt[0] + sxt[1]) + sxt[2]) - kap * hph)) * ssc[6];
        bad |= !(om > 0.0) || !isfinite(om);
        if (lane == 0) sxt[3] = om;
      }
    if (wv < 2) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < SR; kk += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sPH[(16 * wv + lr) * SLH + kk + lk], sW[(kk + lk) * SR + lr], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) sT[(16 * wv + lk + 4 * q) * SLH + lr] = acc[q];
    }
    ssm_barrier();
    // ---- phase 10: P = Pbar - T2 (Pbar H^T)^T; the step's stores, from LDS ----
    {
      f64x4 acc;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = sPb[(ti + lk + 4 * q) * SLA + tj + lr];
#pragma unroll
      for (int kk = 0; kk < SR; kk += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-sT[(ti + lr) * SLH + kk + lk], sPH[(tj + lr) * SLH + kk + lk], acc, 0, 0, 0);
      if constexpr (ROB) {
        const double bom = p.beta * sxt[3];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] *= bom;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) sP[(ti + lk + 4 * q) * SLA + tj + lr] = acc[q];
    }
    if constexpr (MSK) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (tid + u * WG < d) smk[tid + u * WG] = nm[u];
    }
    if (tid < np) Xg[(size_t)t * np + tid] = sx[tid];
    if (p.Ypred) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * WG;
        if (i < d) p.Ypred[((size_t)rep * n + t) * d + i] = syh[i];
      }
    }
    if constexpr (ROB || MSK) {       // four scalars per step: (s, eta, omega, phi)
      if (p.scal && tid == 64) {
        double* o = p.scal + ((size_t)rep * n + t) * 4;
        o[0] = ssc[0];
        o[1] = ssc[1];
        o[2] = ROB ? sxt[3] : 1.0;
        o[3] = ROB ? ssc[7] : 1.0;
      }
    } else if (p.scal && tid == 64) {
      p.scal[((size_t)rep * n + t) * 2] = ssc[0];
      p.scal[((size_t)rep * n + t) * 2 + 1] = ssc[1];
    }
    if constexpr (ROB)
      if (tid == 64) {
        ssc[4] *= sxt[3];
        ssc[5] = sxt[8];
        ssc[6] = sxt[9];
      }
    ssm_barrier();
  }
  if constexpr (ROB)
    if (tid == 0) { p.rstate[2 * rep] = ssc[5]; p.rstate[2 * rep + 1] = ssc[4]; }
  if (tid == 0) *errflag = 0;
  __syncthreads();
  for (int idx = tid; idx < d * r; idx += WG) { const int i = idx / r, l = idx - i * r; Cg[idx] = sC[i * SR + l]; }
  for (int idx = tid; idx < r * r; idx += WG) { const int i = idx / r, l = idx - i * r; Vg[idx] = sV[i * SR + l]; }
  for (int idx = tid; idx < np * np; idx += WG) { const int i = idx / np, l = idx - i * np; Pg[idx] = sP[i * SLA + l]; }
  if (tid < np) xg[tid] = sx[tid];
  if (bad) *errflag = 1;                     // (benign race: every writer stores 1)
  __syncthreads();
  if (tid == 0) p.err[rep] = *errflag;
}

}  // namespace psmf

namespace psmf {
namespace {

// psmf_ssm_run (ex = false: `scalars` is batch x n x 2, no mask, not robust) and psmf_ssm_run_ex (batch x n x 4)
int ssm_run(const EntryFail& fail, bool ex, const psmf_ssm_config_ex* cfg, const double* Y, const uint8_t* mask, double* C, double* V, double* x,
            double* P, const double* A, const double* Q, const double* H, double rho, double* robust_state, double* X, double* Ypred,
            double* scalars, int32_t* status, float* elapsed_ms) {
  if (!cfg || !Y || !C || !V || !x || !P || !A || !Q || !H || !X) return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const bool robust = cfg->robust != 0, masked = mask != nullptr;
  const int d = cfg->d, n = cfg->n, r = cfg->r, np = cfg->p, B = cfg->batch;
  if (d < 1 || d > 2 * WG)
    return fail(PSMF_ERR_ARG, "need 1 <= d <= 512 (one workgroup per replica holds C in LDS; d = " + std::to_string(d) + ")");
  if (r < 1 || r > SR) return fail(PSMF_ERR_ARG, "need 1 <= r <= 16 (r = " + std::to_string(r) + ")");
  if (np > SP) return fail(PSMF_ERR_ARG, "need p <= 32 (p = " + std::to_string(np) + ")");
  if (np < r) return fail(PSMF_ERR_ARG, "need p >= r: the observation map H is r x p (p = " + std::to_string(np) + ", r = " + std::to_string(r) + ")");
  if (n < 1 || B < 1) return fail(PSMF_ERR_ARG, "need n >= 1 and batch >= 1");
  if (cfg->want_pred && !Ypred) return fail(PSMF_ERR_ARG, "want_pred needs Ypred");
  if (!std::isfinite(rho) || rho < 0.0) return fail(PSMF_ERR_ARG, "rho must be finite and >= 0 (R = rho I)");
  if (robust) {
    if (!std::isfinite(cfg->lambda0) || cfg->lambda0 <= 0.0) return fail(PSMF_ERR_ARG, "robust needs a finite lambda0 > 0");
    if (!std::isfinite(cfg->alpha) || cfg->alpha <= 0.0 || !std::isfinite(cfg->beta) || cfg->beta <= 0.0)
      return fail(PSMF_ERR_ARG, "alpha and beta must be finite and > 0");
    if (!robust_state) return fail(PSMF_ERR_ARG, "robust needs robust_state (batch x 2: lambda, Omega)");
    if (!cfg->first_step)
      for (int b = 0; b < B; ++b) {
        const double l = robust_state[2 * b], o = robust_state[2 * b + 1];
        if (!std::isfinite(l) || l <= 0.0 || !std::isfinite(o) || o <= 0.0)
          return fail(PSMF_ERR_ARG, "robust_state needs finite lambda > 0 and Omega > 0 (replica " + std::to_string(b) + ")");
      }
  }
  if (masked)       // every step needs an observed row: eta = 0 and phi = 0 / 0 otherwise
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < n; ++t) {
        const uint8_t* m = mask + ((size_t)b * n + t) * d;
        int cnt = 0;
        for (int i = 0; i < d; ++i) {
          if (m[i] > 1) return fail(PSMF_ERR_ARG, "the mask must hold 0 and 1 only (replica " + std::to_string(b) + ", step " + std::to_string(t) + ")");
          cnt += m[i];
        }
        if (cnt == 0) return fail(PSMF_ERR_ARG, "no observed row in replica " + std::to_string(b) + ", step " + std::to_string(t) + ": every step needs at least one");
      }
  const size_t lds = ssm_lds_bytes(d, masked);
  if (lds > 160 * 1024) return fail(PSMF_ERR_ARG, "the replica's state needs more than 160 KB of LDS");
  {
    // Q: symmetric positive definite (Cholesky on the host, p <= 32)
    double qmax = 0.0;
    for (int i = 0; i < np * np; ++i) {
      if (!std::isfinite(Q[i]) || !std::isfinite(A[i])) return fail(PSMF_ERR_ARG, "A and Q must be finite");
      qmax = std::fmax(qmax, std::fabs(Q[i]));
    }
    for (int i = 0; i < np; ++i)
      for (int j = 0; j < i; ++j)
        if (std::fabs(Q[i * np + j] - Q[j * np + i]) > 1e-12 * qmax) return fail(PSMF_ERR_ARG, "Q must be symmetric");
    std::vector<double> L((size_t)np * np, 0.0);
    for (int i = 0; i < np; ++i)
      for (int j = 0; j <= i; ++j) {
        double a = Q[i * np + j];
        for (int k = 0; k < j; ++k) a -= L[i * np + k] * L[j * np + k];
        if (i == j) {
          if (!(a > 0.0)) return fail(PSMF_ERR_ARG, "Q must be positive definite");
          L[i * np + i] = std::sqrt(a);
        } else {
          L[i * np + j] = a / L[j * np + j];
        }
      }
  }
  PSMF_TRY(open_device(fail, cfg->device));

  const size_t nY = (size_t)B * n * d, nC = (size_t)B * d * r, nV = (size_t)B * r * r, nx = (size_t)B * np, nP = (size_t)B * np * np;
  const size_t pp = (size_t)np * np, rp = (size_t)r * np;
  const bool plain = !robust && !masked;       // the plain instance writes two scalars per step
  const size_t nX = (size_t)B * n * np, nS = (size_t)B * n * (plain ? 2 : 4);
  Dev<double> dY, dC, dV, dx, dP, dA, dQ, dH, dX, dYp, dSc, dRs;
  Dev<unsigned char> dM;
  Dev<int> dErr;
  TimedLaunch timed;
  std::vector<int> herr(B, 0);
  const auto io = std::make_tuple(      // buffer, filled from, read back to, elements
      slot(dY, Y, nullptr, nY), slot(dC, C, C, nC), slot(dV, V, V, nV), slot(dx, x, x, nx), slot(dP, P, P, nP),
      slot(dA, A, nullptr, pp), slot(dQ, Q, nullptr, pp), slot(dH, H, nullptr, rp), slot(dX, nullptr, X, nX), slot(dErr, nullptr, nullptr, B),
      slot(dYp, nullptr, Ypred, cfg->want_pred ? nY : 0), slot(dSc, nullptr, scalars, scalars ? nS : 0));
  PSMF_TRY(alloc_all(fail, io));
  PSMF_TRY(copy_in_all(fail, io));
  if (masked) PSMF_TRY(alloc_copy_in(fail, dM, mask, nY));
  if (robust) {
    PSMF_TRY(alloc_n(fail, dRs, (size_t)B * 2));
    if (!cfg->first_step) PSMF_TRY(copy_in(fail, dRs, robust_state, (size_t)B * 2));
  }
  SsmParamsEx sp;
  sp.d = d; sp.n = n; sp.r = r; sp.p = np; sp.carry_P = cfg->carry_P != 0; sp.first_step = cfg->first_step != 0; sp.rho = rho;
  sp.Y = dY; sp.C = dC; sp.V = dV; sp.x = dx; sp.P = dP; sp.A = dA; sp.Q = dQ; sp.H = dH; sp.X = dX;
  sp.Ypred = cfg->want_pred ? dYp.get() : nullptr; sp.scal = scalars ? dSc.get() : nullptr; sp.err = dErr;
  sp.mask = masked ? dM.get() : nullptr; sp.rstate = robust ? dRs.get() : nullptr;
  sp.lambda0 = cfg->lambda0; sp.alpha = cfg->alpha; sp.beta = cfg->beta; sp.fixed_lambda = cfg->fixed_lambda != 0;
  SsmParams sp0 = sp;       // what the plain instance takes
  const void* const kern = robust ? (masked ? (const void*)psmf_ssm_kernel<true, true> : (const void*)psmf_ssm_kernel<true, false>)
                                  : (masked ? (const void*)psmf_ssm_kernel<false, true> : (const void*)psmf_ssm_kernel<false, false>);
  PSMF_TRY(timed.run(fail, kern, dim3(B), dim3(WG), plain ? (void*)&sp0 : (void*)&sp, lds, elapsed_ms));
  PSMF_TRY(copy_out_all(fail, io));
  if (scalars && ex && plain)       // (s, eta) -> (s, eta, omega = 1, phi = 1), in place from the back
    for (size_t i = (size_t)B * n; i-- > 0;) {
      const double s0 = scalars[2 * i], s1 = scalars[2 * i + 1];
      scalars[4 * i] = s0; scalars[4 * i + 1] = s1; scalars[4 * i + 2] = 1.0; scalars[4 * i + 3] = 1.0;
    }
  if (robust) PSMF_TRY(copy_out(fail, robust_state, dRs, (size_t)B * 2));
  PSMF_TRY(copy_out(fail, herr.data(), dErr, B));
  // Per-replica outcome, as psmf_impute_run; the other replicas are untouched by a bad one (one workgroup each).
  const auto bad = [&](int b) { return herr[b] != 0 || !all_finite(x + (size_t)b * np, np) || !all_finite(C + (size_t)b * d * r, (size_t)d * r); };
  return replica_status(fail, B, status, bad, [](int b) {
    return "the r x r system lost positive definiteness, or the state is not finite, in replica " + std::to_string(b);
  });
}

}  // namespace
}  // namespace psmf

extern "C" int psmf_ssm_run(const psmf_ssm_config* cfg, const double* Y, double* C, double* V, double* x, double* P, const double* A,
                            const double* Q, const double* H, double rho, double* X, double* Ypred, double* scalars, int32_t* status,
                            float* elapsed_ms) {
  psmf_ssm_config_ex c{};
  if (cfg) {
    c.abi_version = cfg->abi_version; c.d = cfg->d; c.n = cfg->n; c.r = cfg->r; c.p = cfg->p; c.batch = cfg->batch; c.device = cfg->device;
    c.carry_P = cfg->carry_P; c.first_step = cfg->first_step; c.want_pred = cfg->want_pred;
  }
  return psmf::ssm_run(EntryFail{"psmf_ssm_run"}, false, cfg ? &c : nullptr, Y, nullptr, C, V, x, P, A, Q, H, rho, nullptr, X, Ypred, scalars, status, elapsed_ms);
}

extern "C" int psmf_ssm_run_ex(const psmf_ssm_config_ex* cfg, const double* Y, const uint8_t* mask, double* C, double* V, double* x,
                               double* P, const double* A, const double* Q, const double* H, double rho, double* robust_state, double* X,
                               double* Ypred, double* scalars, int32_t* status, float* elapsed_ms) {
  return psmf::ssm_run(EntryFail{"psmf_ssm_run_ex"}, true, cfg, Y, mask, C, V, x, P, A, Q, H, rho, robust_state, X, Ypred, scalars, status, elapsed_ms);
}
