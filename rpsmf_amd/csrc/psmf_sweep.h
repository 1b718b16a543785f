// Sweeps, solves and reductions that the per-step engine shares with the blocked engine's kernels and the masked small-shape engine:
// the symmetric sweep inversion, the fixed-order strided sum, the column / block reductions through LDS.
// Defines no kernel (the per-step engine's are in psmf_kernels.hip), so any translation unit may include it.
#pragma once
#include "psmf_device.h"

namespace psmf {

// fixed-order sum of base[w * ps] for w = first, first + step, ... < n, 16 independent loads in flight.
// The loads are UNCONDITIONAL (index clamped, value masked afterwards): a load under a runtime
// predicate makes hipcc branch around it and wait for it alone -- 16 dependent L2 round trips.
__device__ __forceinline__ double strided_sum(const double* base, int first, int step, int n, int ps) {
  double acc = 0.0;
  for (int w0 = first; w0 < n; w0 += 16 * step) {
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = base[(size_t)min(w0 + q * step, n - 1) * ps];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (w0 + q * step < n) ? v[q] : 0.0;
    acc += (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) +
           (((v[8] + v[9]) + (v[10] + v[11])) + ((v[12] + v[13]) + (v[14] + v[15])));
  }
  return acc;
}

// ------------------------------------------------------------------------------------------
// r x r solve block:  Pplus = (Pbar^-1 + kappa G)^-1  -- the reference's own formulation
// (inv(P_bar), then inv(Pi + C^T Ri C): pypsmf/psmf/psmf.py:147-149, ExperimentImpute/PSMF.py:34-36)
// as two symmetric SWEEP passes in float64.  Sweeping pivot k of a symmetric matrix A,
//     a_ij <- a_ij - a_ik a_kj / a_kk   (i, j != k),   a_ik = a_ki <- a_ik / a_kk,   a_kk <- -1 / a_kk,
// for all k turns A into -A^-1; for SPD A every pivot is positive, no pivot search is needed and
// the matrix stays (bitwise) symmetric, so one pivot ROW per step is all the waves exchange:
// matrix in registers (thread = column c, rows rg + m * RG), pivot row through a ping-pong LDS
// line, one barrier per pivot.  A non-positive pivot raises the numeric-error flag (the
// reference raises LinAlgError from np.linalg.inv in the same situation).
// ------------------------------------------------------------------------------------------
// LDS_ONLY: the barriers order LDS traffic only (s_waitcnt lgkmcnt(0); s_barrier) instead of __syncthreads(), which also
// drains vmcnt -- for callers that keep global loads / stores in flight across the solve (psmf_impute.hip)
template <bool LDS_ONLY>
__device__ __forceinline__ void solve_barrier() {
  if (LDS_ONLY) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else __syncthreads();
}

template <int RPAD, bool LDS_ONLY = false>
__device__ __forceinline__ void sweep_all(double (&A)[(RPAD * RPAD) / WG > 0 ? (RPAD * RPAD) / WG : 1], const int r2,
                                          const int c, const int rg, double* rowbuf, int* errflag) {
  // (a 512-thread workgroup may run two independent sweeps in lockstep, one per 256-thread half, each
  //  with its own rowbuf: the wave id is taken modulo 4 and the barriers are shared)
  constexpr int RG = WG / RPAD;                 // row groups; wave w holds row groups [w*RGW, (w+1)*RGW)
  constexpr int RGW = RG / 4 > 0 ? RG / 4 : 1;  // (RPAD = 64: one row group per wave)
  constexpr int M = (RPAD * RPAD) / WG > 0 ? (RPAD * RPAD) / WG : 1;
  // Measured on MI355X (tools/solve_prof.hip): one LDS publish -> barrier -> LDS read exchange costs
  // ~450 cycles whatever is exchanged, the arithmetic of a pivot ~250.  So pivots are taken as 2 x 2
  // SPD blocks: two pivot rows per exchange, the 2 x 2 inverse recomputed by every thread.
  //   K = [[a, b], [b, e]] = rows/cols (k, k+1);  Ki = K^-1 = [[p, q], [q, s]]
  //   a_ic <- a_ic - [u_i w_i] Ki [u_c w_c]^T            (i, c outside the block; u = row k, w = row k+1)
  //   rows k, k+1 <- Ki [u_c; w_c]    columns k, k+1 <- the same by symmetry    block <- -Ki
  // r2 = r rounded up to even (the caller pads with an identity row/column).
  const int wv = (threadIdx.x >> 6) & 3;
  const bool con = c < r2;
  const int cc = con ? c : r2 - 1;
  int ic[M];
#pragma unroll
  for (int m = 0; m < M; ++m) ic[m] = min(rg + m * RG, r2 - 1);
  // rows 0 and 1 live in slot m = 0 of row groups 0 and 1 (RG >= 4)
  if (rg < 2 && con) rowbuf[rg * RM + c] = A[0];
  solve_barrier<LDS_ONLY>();
  bool bad = false;
  for (int k = 0; k < r2; k += 2) {
    const double* rb0 = rowbuf + ((k >> 1) & 1) * 2 * RM;
    const double* rb1 = rb0 + RM;
    double* rn0 = rowbuf + (((k >> 1) + 1) & 1) * 2 * RM;
    double* rn1 = rn0 + RM;
    const double ka = rb0[k], kb = rb0[k + 1], ke = rb1[k + 1];
    const double uc = rb0[cc], wc = rb1[cc];
    double ui[M], wi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      ui[m] = rb0[ic[m]];
      wi[m] = rb1[ic[m]];
    }
    const double det = ka * ke - kb * kb;
    bad |= !(ka > 0.0) | !(det > 0.0);
    const double dinv = fast_rcp(det);
    const double kp = ke * dinv, kq = -kb * dinv, ks = ka * dinv;
    const bool c0 = (c == k), c1 = (c == k + 1);
    // coefficients of this thread's column: generic  t = Ki [u_c; w_c];  pivot columns: -row of Ki, no a_ic term
    double t1 = kp * uc + kq * wc;
    double t2 = kq * uc + ks * wc;
    const double keep = (c0 | c1) ? 0.0 : 1.0;
    const double g1 = c0 ? -kp : (c1 ? -kq : t1);
    const double g2 = c0 ? -kq : (c1 ? -ks : t2);
#pragma unroll
    for (int m = 0; m < M; ++m) A[m] = fma(-wi[m], g2, fma(-ui[m], g1, keep * A[m]));
    // pivot rows: a_kc <- t1, a_(k+1)c <- t2; inside the block <- -Ki   (only in the waves that hold them)
    if (((k % RG) / RGW) == wv || (((k + 1) % RG) / RGW) == wv) {
      const double r0v = c0 ? -kp : (c1 ? -kq : t1);
      const double r1v = c0 ? -kq : (c1 ? -ks : t2);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int i = rg + m * RG;
        A[m] = (i == k) ? r0v : ((i == k + 1) ? r1v : A[m]);
      }
    }
    // next two pivot rows -> LDS
    if (k + 2 < r2) {
      if ((((k + 2) % RG) / RGW) == wv || (((k + 3) % RG) / RGW) == wv) {
        double nx = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int i = rg + m * RG;
          nx = (i == k + 2 || i == k + 3) ? A[m] : nx;
        }
        if (con && ((k + 2) % RG) == rg) rn0[c] = nx;
        if (con && ((k + 3) % RG) == rg) rn1[c] = nx;
      }
    }
    solve_barrier<LDS_ONLY>();
  }
  if (bad && (threadIdx.x & (WG - 1)) == 0) *errflag = 1;
}

// A (in): symmetric Pbar elements of this thread, identity-padded to r2;  Gk (in): kappa * G elements
// (0 in the padding).  A (out): elements of (Pbar^-1 + kappa G)^-1.  rowbuf: 4 * RM doubles of LDS.
template <int RPAD, bool LDS_ONLY = false>
__device__ __forceinline__ void spd_update_solve(double (&A)[(RPAD * RPAD) / WG > 0 ? (RPAD * RPAD) / WG : 1],
                                                 const double (&Gk)[(RPAD * RPAD) / WG > 0 ? (RPAD * RPAD) / WG : 1],
                                                 const int r2, const int c, const int rg, double* rowbuf, int* errflag) {
  constexpr int M = (RPAD * RPAD) / WG > 0 ? (RPAD * RPAD) / WG : 1;
  sweep_all<RPAD, LDS_ONLY>(A, r2, c, rg, rowbuf, errflag);       // A = -Pbar^-1
#pragma unroll
  for (int m = 0; m < M; ++m) A[m] = Gk[m] - A[m];
  sweep_all<RPAD, LDS_ONLY>(A, r2, c, rg, rowbuf, errflag);       // A = -(Pbar^-1 + kappa G)^-1
#pragma unroll
  for (int m = 0; m < M; ++m) A[m] = -A[m];
}

template <int RPAD, int NWK = WG>
__device__ __forceinline__ void col_reduce(double partial, double* s_red, double* s_out) {
  constexpr int RG = NWK / RPAD;
  const int tid = threadIdx.x;
  s_red[tid] = partial;  // index = (tid / RPAD) * RPAD + tid % RPAD
  __syncthreads();
  if (tid < RPAD) {
    double a = 0.0;
#pragma unroll
    for (int gI = 0; gI < RG; ++gI) a += s_red[gI * RPAD + tid];
    s_out[tid] = a;
  }
  __syncthreads();
}

template <int NWK = WG>
__device__ __forceinline__ double block_sum(double x, double* s4) {   // worker waves only
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = x;
  __syncthreads();
  double a = 0.0;
#pragma unroll
  for (int g = 0; g < NWK / 64; g += 4) a += (s4[g] + s4[g + 1]) + (s4[g + 2] + s4[g + 3]);      // fixed order
  return a;
}

}  // namespace psmf
