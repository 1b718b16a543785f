// Batched Bayesian probabilistic matrix factorisation (the BPMF baseline of the imputation experiment, ExperimentImpute/BPMF.py:121-302:
// a Gibbs sampler over the factors and their Gaussian-Wishart hyper-parameters), float64 throughout, for a batch of independent
// replicas.  The recursion is written out at psmf_bpmf_run in include/psmf_hip.h.
//
// The host hands over every random number of the sampler, drawn up front in the reference's order -- no draw depends on the data:
// per epoch two standard Bartlett factors and two r-vectors of normals for the hyper-parameters, and per sweep n x r and d x r
// normals -- and the warm-start factors.  The device does all the arithmetic.  Within a sweep the columns are conditionally
// independent given P and the rows given W, so the reference's serial loops are parallel as they stand.  Per epoch, launches on the
// null stream (the dependencies between the phases are whole-grid ones, and launches express them):
//
//   psmf_bpmf_wsum_kernel    grid = (workgroups per replica, replicas): the column sums of W over the workgroup's columns.
//   psmf_bpmf_wcov_kernel    same grid: the mean of W from those partial sums, added in workgroup order, then the centred Gram
//       sum_j (w_j - xbar)(w_j - xbar)^T of the workgroup's columns on v_mfma_f64_16x16x4_f64 (np.cov is two passes).
//   psmf_bpmf_hyper_kernel   grid = replicas, one workgroup: for W (N = n, from the partials) and then for P (N = d, directly) the
//       r x r hyper step.  T = I + N S + N b0 / (b0 + N) xbar xbar^T is factored T = U U^T from the last row upwards (U upper
//       triangular), so that U^-T IS the lower Cholesky factor of T^-1: alpha = X X^T with U^T X = A, A the Bartlett factor;
//       (b0 + N) alpha = V V^T the same way and mu = V^-1 z + N xbar / (b0 + N).  Written out: alpha and alpha mu, zero-padded to 16
//       with a unit diagonal in the padding.
//   then twice (the two Gibbs sweeps of an epoch):
//   psmf_bpmf_col_kernel     grid = (workgroups per replica, replicas); a workgroup owns a range of columns and holds P (zero-padded to
//       16 features) in LDS; a wave takes four columns at a time.  Per column the masked Gram sum_i m_ij p_i p_i^T and the right-hand
//       side sum_i m_ij (v_ij - mbar) p_i run on the matrix core (A operand: element (row lr, k-slot lk); B operand (k-slot lk,
//       column lr); result rows lk + 4 q of column lr; lr = lane & 15, lk = lane >> 4): the contracted index is the row i, four rows
//       a product, and the masked P is the A operand where the plain P is the B operand.  Lambda = alpha + beta Gram goes to a
//       wave-private LDS image, 16 x 17 with b = beta rhs + alpha mu in the 17th column, from which the 16 lanes of row g of the wave
//       read the system of column j0 + g, a lane a matrix row.  bpmf_factor_sample then factors Lambda = U U^T from the last row
//       upwards, in registers with lane reads, and returns U^-1 z + U^-T U^-1 b, which is cholesky(inv Lambda).T z + inv(Lambda) b.
//   psmf_bpmf_row_part_kernel   same grid: per row i the Gram sum_j m_ij w_j w_j^T and right-hand side over the workgroup's columns
//       (the new W), a wave a row, four columns a product; one 16 x 17 partial per workgroup and row.
//   psmf_bpmf_row_kernel     grid = (ceil(d / 16), replicas): adds the partials of a row in workgroup order, then the same
//       bpmf_factor_sample, 16 lanes a row.
//   psmf_bpmf_metric_kernel  grid = replicas, once in front of the first epoch (the prediction of the warm start opens the running
//       average) and once per epoch: the prediction at the probe entries, the running average, the squared error of the average.
//
// No atomics and no flags.  Every sum has a fixed order, so a call gives the same bits twice, a replica the same bits alone as inside
// a batch, and the chunking moves no bit (the workgroups of a replica depend on n and PSMF_BPMF_COLS alone).  A non-positive pivot
// sets the replica's flag (a plain store of 1) and the replica goes on in NaNs; nothing of its neighbours reads it.
// Limits: 2 <= d <= 512, 2 <= r <= 16, n >= 2.
#include "psmf_host.h"        // Switches
#include "psmf_batch.h"       // EntryFail, open_device, plan_chunk, per-item slots, TimedLaunch, cols_per_workgroup, all_finite, replica_status
#include "psmf_wave.h"        // f64x4, row_sum_f64_dpp

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace psmf {

constexpr int BPMF_MAX_D = 512, BPMF_MAX_R = 16;
constexpr int BPMF_S = 17;                 // row stride of every 16-wide LDS or global image: 16 features and the right-hand side
constexpr int BPMF_IMG = 16 * BPMF_S;      // a 16 x 16 system with its right-hand side
constexpr int BPMF_WG = 256;               // every kernel
constexpr int BPMF_MAX_REPLICAS = 65535;   // grid.y
constexpr double BPMF_B0 = 2.0;            // b0_u = b0_m of BPMF.py:152-158

struct BpmfParams {
  int d, n, r, cols, nwg, epochs, epoch, sweep, count, last;
  double beta;
  const double* Yt;            // n x d, time-major, shared by the replicas
  const uint8_t* M;            // replicas x n x d, nonzero = training entry
  const uint8_t* miss;         // replicas x n x d, nonzero = probe entry
  const double* mu;            // replicas
  const double* mbar;          // replicas
  const double* bart;          // replicas x epochs x 2 x r x r
  const double* hz;            // replicas x epochs x 2 x r
  const double* Z;             // replicas x epochs x 2 x (n + d) x r
  double* W;                   // replicas x n x r
  double* P;                   // replicas x d x r
  double* psum;                // replicas x nwg x 16
  double* pcov;                // replicas x nwg x 256
  double* hyp;                 // replicas x 2 x BPMF_IMG: alpha, and alpha mu in the 17th column (0: of W, 1: of P)
  double* part;                // replicas x nwg x d x BPMF_IMG
  double* avg;                 // replicas x n x d: the running average of the prediction at the probe entries
  double* efull;               // replicas x epochs
  double* yrec;                // replicas x n x d or null
  int* bad;                    // replicas
};

// the wave's own LDS stores are complete and visible to its lanes (LDS operations of a wave complete in program order)
__device__ __forceinline__ void bpmf_wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Lane lr of a 16-lane row holds row lr of the symmetric positive definite A (a[0 .. 15]; rows beyond r: the unit matrix), b_lr and
// z_lr.  Factors A = U U^T from the last row upwards -- afterwards a[k] = U[lr][k] -- and returns component lr of
// U^-1 z + U^-T U^-1 b.  `bad` is set where a pivot is not positive.
__device__ __forceinline__ double bpmf_factor_sample(double (&a)[16], const double b, const double z, const int lr, bool& bad) {
  double dg[16];
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const double piv = __shfl(a[k], k, 16);
    bad = bad || !(piv > 0.0);
    const double ukk = sqrt(piv);
    dg[k] = ukk;
    const double u = lr < k ? a[k] / ukk : (lr == k ? ukk : 0.0);
    a[k] = u;
#pragma unroll
    for (int j = 0; j < k; ++j) a[j] = fma(-u, __shfl(u, j, 16), a[j]);
  }
  // U y = b and U t = z, from the last component upwards
  double yb = b, yz = z;
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const double tb = __shfl(yb, k, 16) / dg[k], tz = __shfl(yz, k, 16) / dg[k];
    if (lr == k) { yb = tb; yz = tz; }
    else if (lr < k) { yb = fma(-a[k], tb, yb); yz = fma(-a[k], tz, yz); }
  }
  // U^T x = y: x_i = (y_i - sum over k < i of U[k][i] x_k) / U[i][i]; lane k holds U[k][i] in a[i]
  double x = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const double s = row_sum_f64_dpp(lr < i ? a[i] * x : 0.0);
    if (lr == i) x = (yb - s) / dg[i];
  }
  return yz + x;
}

__device__ __forceinline__ const double* bpmf_normals(const BpmfParams& p, int rep) {      // of this sweep: n x r for W, then d x r for P
  return p.Z + (((size_t)rep * p.epochs + p.epoch) * 2 + p.sweep) * ((size_t)p.n + p.d) * p.r;
}

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_wsum_kernel(BpmfParams p) {
  __shared__ double s[BPMF_WG];
  const int r = p.r, tid = threadIdx.x, k = tid & 15, sub = tid >> 4, rep = blockIdx.y, wg = blockIdx.x;
  const int c0 = wg * p.cols, c1 = min(p.n, c0 + p.cols);
  const double* Wg = p.W + (size_t)rep * p.n * r;
  double acc = 0.0;
  if (k < r)
    for (int j = c0 + sub; j < c1; j += 16) acc += Wg[(size_t)j * r + k];
  s[tid] = acc;
  __syncthreads();
  for (int h = 8; h > 0; h >>= 1) {
    if (sub < h) s[tid] += s[tid + 16 * h];
    __syncthreads();
  }
  if (tid < 16) p.psum[((size_t)rep * p.nwg + wg) * 16 + tid] = s[tid];
}

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_wcov_kernel(BpmfParams p) {
  __shared__ double sC[256];
  const int r = p.r, n = p.n, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4, rep = blockIdx.y, wg = blockIdx.x;
  const int c0 = wg * p.cols, c1 = min(n, c0 + p.cols);
  const double* Wg = p.W + (size_t)rep * n * r;
  const double* ps = p.psum + (size_t)rep * p.nwg * 16;
  double xbar = 0.0;
  for (int w = 0; w < p.nwg; ++w) xbar += ps[w * 16 + lr];      // in the order of the workgroups
  xbar /= (double)n;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = c0 + 4 * wv; j0 < c1; j0 += 16) {
    const int j = j0 + lk;
    const double v = (j < c1 && lr < r) ? Wg[(size_t)j * r + lr] - xbar : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
  }
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int slot = (lk + 4 * q) * 16 + lr;
        sC[slot] = w == 0 ? acc[q] : sC[slot] + acc[q];
      }
    }
    __syncthreads();
  }
  p.pcov[((size_t)rep * p.nwg + wg) * 256 + tid] = sC[tid];
}

// T (16 x BPMF_S in LDS, its leading r x r block symmetric) = U U^T from the last row upwards; U[i][k], i <= k, replaces T[i][k]
__device__ void bpmf_hyper_factor(double* T, const int r, const int tid, bool& bad) {
  const int i = tid >> 4, j = tid & 15;
  for (int k = r - 1; k >= 0; --k) {
    __syncthreads();
    const double piv = T[k * BPMF_S + k];
    bad = bad || !(piv > 0.0);
    const double ukk = sqrt(piv);
    __syncthreads();
    if (tid < k) T[tid * BPMF_S + k] = T[tid * BPMF_S + k] / ukk;
    else if (tid == k) T[k * BPMF_S + k] = ukk;
    __syncthreads();
    if (i < k && j < k) T[i * BPMF_S + j] = fma(-T[i * BPMF_S + k], T[j * BPMF_S + k], T[i * BPMF_S + j]);
  }
  __syncthreads();
}

// One side of the hyper step.  sG: the centred Gram (16 x 16, stride 16), sX: xbar; the other LDS buffers are scratch.
__device__ void bpmf_hyper_side(const int r, const double N, const double* sG, const double* sX, const double* bart, const double* z, double* sT, double* sA,
                                double* sAl, double* sMu, double* out, const int tid, bool& bad) {
  const int f = tid >> 4, g = tid & 15;
  const double b0 = BPMF_B0;
  if (f < r && g < r) {
    const double S = sG[f * 16 + g] * (1.0 / (N - 1.0));                                   // np.cov: the Gram times 1 / (N - 1)
    sT[f * BPMF_S + g] = ((f == g ? 1.0 : 0.0) + N * S) + (((N * b0) * sX[f]) * sX[g]) / (b0 + N);
    sA[f * BPMF_S + g] = bart[f * r + g];
  }
  bpmf_hyper_factor(sT, r, tid, bad);
  // U^T X = A, a thread a column of X (in the place of A)
  if (tid < r) {
    for (int i = 0; i < r; ++i) {
      double s = sA[i * BPMF_S + tid];
      for (int k = 0; k < i; ++k) s = fma(-sT[k * BPMF_S + i], sA[k * BPMF_S + tid], s);
      sA[i * BPMF_S + tid] = s / sT[i * BPMF_S + i];
    }
  }
  __syncthreads();
  double al = f == g ? 1.0 : 0.0;      // the padding: a unit diagonal
  if (f < r && g < r) {
    al = 0.0;
    for (int c = 0; c < r; ++c) al = fma(sA[f * BPMF_S + c], sA[g * BPMF_S + c], al);
    sT[f * BPMF_S + g] = (b0 + N) * al;
  }
  sAl[f * 16 + g] = al;
  __syncthreads();
  bpmf_hyper_factor(sT, r, tid, bad);
  if (tid == 0) {                      // V t = z from the last component upwards, then mu = t + N xbar / (b0 + N)
    for (int k = r - 1; k >= 0; --k) {
      double s = z[k];
      for (int j = k + 1; j < r; ++j) s = fma(-sT[k * BPMF_S + j], sMu[j], s);
      sMu[k] = s / sT[k * BPMF_S + k];
    }
    for (int k = 0; k < 16; ++k) sMu[k] = k < r ? sMu[k] + (N * sX[k]) / (b0 + N) : 0.0;
  }
  __syncthreads();
  out[f * BPMF_S + g] = al;
  if (g == 0) {
    double h = 0.0;
    for (int c = 0; c < r; ++c) h = fma(sAl[f * 16 + c], sMu[c], h);
    out[f * BPMF_S + 16] = f < r ? h : 0.0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_hyper_kernel(BpmfParams p) {
  __shared__ double sG[256], sX[16], sT[BPMF_IMG], sA[BPMF_IMG], sAl[256], sMu[16];
  const int d = p.d, n = p.n, r = p.r, tid = threadIdx.x, f = tid >> 4, g = tid & 15, rep = blockIdx.x;
  const double* bart = p.bart + ((size_t)rep * p.epochs + p.epoch) * 2 * r * r;
  const double* hz = p.hz + ((size_t)rep * p.epochs + p.epoch) * 2 * r;
  double* hyp = p.hyp + (size_t)rep * 2 * BPMF_IMG;
  bool bad = false;
  // W: the partial sums and partial Grams of the workgroups, in their order
  {
    const double* ps = p.psum + (size_t)rep * p.nwg * 16;
    const double* pc = p.pcov + (size_t)rep * p.nwg * 256;
    double s = 0.0, c = 0.0;
    for (int w = 0; w < p.nwg; ++w) {
      if (tid < 16) s += ps[w * 16 + tid];
      c += pc[(size_t)w * 256 + tid];
    }
    if (tid < 16) sX[tid] = s / (double)n;
    sG[tid] = c;
  }
  __syncthreads();
  bpmf_hyper_side(r, (double)n, sG, sX, bart, hz, sT, sA, sAl, sMu, hyp, tid, bad);
  // P: d <= 512 rows, two passes
  const double* Pg = p.P + (size_t)rep * d * r;
  if (tid < 16) {
    double s = 0.0;
    if (tid < r)
      for (int i = 0; i < d; ++i) s += Pg[i * r + tid];
    sX[tid] = s / (double)d;
  }
  __syncthreads();
  {
    double c = 0.0;
    if (f < r && g < r)
      for (int i = 0; i < d; ++i) c = fma(Pg[i * r + f] - sX[f], Pg[i * r + g] - sX[g], c);
    sG[tid] = c;
  }
  __syncthreads();
  bpmf_hyper_side(r, (double)d, sG, sX, bart + r * r, hz + r, sT, sA, sAl, sMu, hyp + BPMF_IMG, tid, bad);
  if (bad && tid == 0) p.bad[rep] = 1;
}

// LDS of the column kernel in doubles: P padded to a multiple of 4 rows, alpha with alpha mu, four images per wave
__host__ __device__ constexpr size_t bpmf_col_lds_doubles(int d) { return (size_t)((d + 3) / 4 * 4) * BPMF_S + BPMF_IMG + (BPMF_WG / 64) * 4 * BPMF_IMG; }

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_col_kernel(BpmfParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int d = p.d, n = p.n, r = p.r, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int rep = blockIdx.y, wg = blockIdx.x, dpad = (d + 3) / 4 * 4;
  double* sP = reinterpret_cast<double*>(smem_raw);      // dpad x BPMF_S
  double* sA = sP + dpad * BPMF_S;                       // alpha | alpha mu
  double* sS = sA + BPMF_IMG + wv * 4 * BPMF_IMG;        // the wave's four systems
  const double* Pg = p.P + (size_t)rep * d * r;
  for (int idx = tid; idx < dpad * 16; idx += BPMF_WG) {
    const int i = idx >> 4, k = idx & 15;
    sP[i * BPMF_S + k] = (i < d && k < r) ? Pg[i * r + k] : 0.0;
  }
  const double* hyp = p.hyp + (size_t)rep * 2 * BPMF_IMG;
  for (int idx = tid; idx < BPMF_IMG; idx += BPMF_WG) sA[idx] = hyp[idx];
  __syncthreads();
  const int c0 = wg * p.cols, c1 = min(n, c0 + p.cols);
  const double mu = p.mu[rep], mbar = p.mbar[rep], beta = p.beta;
  const uint8_t* Mg = p.M + (size_t)rep * n * d;
  const double* Zg = bpmf_normals(p, rep);
  double* Wg = p.W + (size_t)rep * n * r;
  bool bad = false;
  for (int j0 = c0 + 4 * wv; j0 < c1; j0 += BPMF_WG / 16) {
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      const int j = j0 + g;      // (uniform)
      double* S = sS + g * BPMF_IMG;
      if (j < c1) {
        const uint8_t* mj = Mg + (size_t)j * d;
        const double* yj = p.Yt + (size_t)j * d;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0}, rhs = {0.0, 0.0, 0.0, 0.0};
        for (int i0 = 0; i0 < dpad; i0 += 4) {
          const int i = i0 + lk;
          const bool m = i < d && mj[i] != 0;
          const double pv = sP[i * BPMF_S + lr];
          const double e = (m && lr == 0) ? (yj[i] - mu) / mu - mbar : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(m ? pv : 0.0, pv, acc, 0, 0, 0);
          rhs = __builtin_amdgcn_mfma_f64_16x16x4f64(pv, e, rhs, 0, 0, 0);      // column 0: sum_i m_ij (v_ij - mbar) p_i
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = lk + 4 * q;
          S[row * BPMF_S + lr] = fma(beta, acc[q], sA[row * BPMF_S + lr]);
          if (lr == 0) S[row * BPMF_S + 16] = fma(beta, rhs[q], sA[row * BPMF_S + 16]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = lk + 4 * q;
          S[row * BPMF_S + lr] = row == lr ? 1.0 : 0.0;
          if (lr == 0) S[row * BPMF_S + 16] = 0.0;
        }
      }
    }
    bpmf_wave_lds_sync();
    const int j = j0 + lk;      // the 16 lanes of row lk: column j, a lane a row of its system
    const bool live = j < c1;
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = sS[lk * BPMF_IMG + lr * BPMF_S + c];
    const double b = sS[lk * BPMF_IMG + lr * BPMF_S + 16];
    const double z = (live && lr < r) ? Zg[(size_t)j * r + lr] : 0.0;
    bool bad_here = false;
    const double w = bpmf_factor_sample(a, b, z, lr, bad_here);
    bad = bad || (live && bad_here);
    if (live && lr < r) Wg[(size_t)j * r + lr] = w;
    bpmf_wave_lds_sync();       // every lane has read its system before the next four overwrite the images
  }
  if (bad) p.bad[rep] = 1;
}

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_row_part_kernel(BpmfParams p) {
  const int d = p.d, n = p.n, r = p.r, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int rep = blockIdx.y, wg = blockIdx.x;
  const int c0 = wg * p.cols, c1 = min(n, c0 + p.cols);
  const double mu = p.mu[rep], mbar = p.mbar[rep];
  const uint8_t* Mg = p.M + (size_t)rep * n * d;
  const double* Wg = p.W + (size_t)rep * n * r;
  double* part = p.part + ((size_t)rep * p.nwg + wg) * d * BPMF_IMG;
  for (int i = wv; i < d; i += BPMF_WG / 64) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0}, rhs = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = c0; j0 < c1; j0 += 4) {
      const int j = j0 + lk;
      const bool in = j < c1;
      const bool m = in && Mg[(size_t)j * d + i] != 0;
      const double wv_ = (in && lr < r) ? Wg[(size_t)j * r + lr] : 0.0;
      const double e = (m && lr == 0) ? (p.Yt[(size_t)j * d + i] - mu) / mu - mbar : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(m ? wv_ : 0.0, wv_, acc, 0, 0, 0);
      rhs = __builtin_amdgcn_mfma_f64_16x16x4f64(wv_, e, rhs, 0, 0, 0);
    }
    double* out = part + (size_t)i * BPMF_IMG;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = lk + 4 * q;
      out[row * BPMF_S + lr] = acc[q];
      if (lr == 0) out[row * BPMF_S + 16] = rhs[q];
    }
  }
}

__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_row_kernel(BpmfParams p) {
  const int d = p.d, r = p.r, tid = threadIdx.x, lr = tid & 15, rep = blockIdx.y;
  const int i = blockIdx.x * (BPMF_WG / 16) + (tid >> 4);      // 16 lanes a row of P, a lane a row of its system
  const bool live = i < d;
  const double* al = p.hyp + ((size_t)rep * 2 + 1) * BPMF_IMG + lr * BPMF_S;
  double a[16], b = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) a[c] = c == lr ? 1.0 : 0.0;
  if (live) {
    double s[BPMF_S];
#pragma unroll
    for (int c = 0; c < BPMF_S; ++c) s[c] = 0.0;
    const double* part = p.part + (size_t)rep * p.nwg * d * BPMF_IMG + (size_t)i * BPMF_IMG + lr * BPMF_S;
    for (int w = 0; w < p.nwg; ++w) {      // in the order of the workgroups
      const double* pw = part + (size_t)w * d * BPMF_IMG;
#pragma unroll
      for (int c = 0; c < BPMF_S; ++c) s[c] += pw[c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = fma(p.beta, s[c], al[c]);
    b = fma(p.beta, s[16], al[16]);
  }
  const double* Zg = bpmf_normals(p, rep) + (size_t)p.n * r;
  const double z = (live && lr < r) ? Zg[(size_t)i * r + lr] : 0.0;
  bool bad = false;
  const double x = bpmf_factor_sample(a, b, z, lr, bad);
  if (live && lr < r) p.P[(size_t)rep * d * r + (size_t)i * r + lr] = x;
  if (live && bad) p.bad[rep] = 1;
}

// count = 0: the prediction of the warm start opens the running average; count = c > 0: avg = (c avg + pred) / (c + 1), the error
// of the average against the data at the probe entries, and with the last epoch the reconstruction
__global__ __launch_bounds__(BPMF_WG) void psmf_bpmf_metric_kernel(BpmfParams p) {
  __shared__ double ssum[BPMF_WG];
  __shared__ long long scnt[BPMF_WG];
  const int d = p.d, r = p.r, rep = blockIdx.x, tid = threadIdx.x;
  const size_t total = (size_t)p.n * d;
  const uint8_t* miss = p.miss + (size_t)rep * total;
  const double* Wg = p.W + (size_t)rep * p.n * r;
  const double* Pg = p.P + (size_t)rep * d * r;
  double* avg = p.avg + (size_t)rep * total;
  const double mu = p.mu[rep], mbar = p.mbar[rep], c = (double)p.count;
  double* yrec = (p.yrec && p.last) ? p.yrec + (size_t)rep * total : nullptr;
  double acc = 0.0;
  long long cnt = 0;
  for (size_t e = tid; e < total; e += BPMF_WG) {
    if (miss[e] == 0) continue;
    const size_t j = e / d;
    const int i = (int)(e - j * d);
    double dot = 0.0;
    for (int k = 0; k < r; ++k) dot = fma(Wg[j * r + k], Pg[i * r + k], dot);
    const double pred = dot + mbar;
    if (p.count == 0) { avg[e] = pred; continue; }
    const double av = (c * avg[e] + pred) / (c + 1.0);
    avg[e] = av;
    const double yhat = av * mu + mu;
    const double df = yhat - p.Yt[e];
    acc = fma(df, df, acc);
    ++cnt;
    if (yrec) yrec[e] = yhat;
  }
  if (p.count == 0) return;      // (uniform)
  ssum[tid] = acc;
  scnt[tid] = cnt;
  __syncthreads();
  for (int s = BPMF_WG / 2; s > 0; s >>= 1) {
    if (tid < s) { ssum[tid] += ssum[tid + s]; scnt[tid] += scnt[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) p.efull[(size_t)rep * p.epochs + p.epoch] = sqrt((1.0 / (double)scnt[0]) * ssum[0]);
}

namespace {

int bpmf_run(const psmf_bpmf_config* cfg, const double* Y, const uint8_t* M, const uint8_t* Mmiss, const double* mean, const double* mean_rating,
             const double* bartlett, const double* hyper_normals, const double* normals, double* P, double* W, double* Efull, double* Yrec,
             int32_t* status, float* elapsed_ms) {
  const EntryFail fail{"psmf_bpmf_run"};
  const Switches sw;      // no handle here: read at entry, on every call
  if (!cfg || !Y || !M || !Mmiss || !mean || !mean_rating || !bartlett || !hyper_normals || !normals || !P || !W || !Efull) return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const int d = cfg->d, n = cfg->n, r = cfg->r, B = cfg->batch, epochs = cfg->epochs;
  if (d < 2 || d > BPMF_MAX_D) return fail(PSMF_ERR_ARG, "need 2 <= d <= 512 (the covariance of P needs two rows, and P lives in the LDS of one workgroup; d = " + std::to_string(d) + ")");
  if (r < 2 || r > BPMF_MAX_R) return fail(PSMF_ERR_ARG, "need 2 <= r <= 16 (one matrix-core tile of features; the reference fails at r = 1; r = " + std::to_string(r) + ")");
  if (n < 2 || B < 1 || epochs < 1) return fail(PSMF_ERR_ARG, "need n >= 2 (the covariance of W needs two rows), batch >= 1 and epochs >= 1");
  if (cfg->want_rec && !Yrec) return fail(PSMF_ERR_ARG, "want_rec needs Yrec");
  if (sw.bpmf_cols < 0 || sw.bpmf_chunk < 0) return fail(PSMF_ERR_ARG, "PSMF_BPMF_COLS and PSMF_BPMF_CHUNK must be >= 0 (0 = chosen by the library)");
  for (int b = 0; b < B; ++b)
    if (mean[b] == 0.0 || !std::isfinite(mean[b])) return fail(PSMF_ERR_ARG, "the mean of the training entries is 0 or not finite in replica " + std::to_string(b) + " (the data is divided by it)");
  const bool wantRec = cfg->want_rec != 0;
  PSMF_TRY(open_device(fail, cfg->device));

  // columns per workgroup: a multiple of the four columns a wave takes at a time (PSMF_BPMF_COLS)
  const auto [cols, nwg] = cols_per_workgroup(n, sw.bpmf_cols, 64, 4);

  const size_t nYd = (size_t)n * d, nW = (size_t)n * r, nP = (size_t)d * r, nZ = (size_t)epochs * 2 * (nW + nP), nBart = (size_t)epochs * 2 * r * r,
               nHz = (size_t)epochs * 2 * r, nPart = (size_t)nwg * d * BPMF_IMG, nSum = (size_t)nwg * 16, nCov = (size_t)nwg * 256;
  const size_t per_rep = 2 * nYd * sizeof(uint8_t) + sizeof(int) +
                         (nZ + nBart + nHz + nW + nP + nPart + nSum + nCov + 2 * BPMF_IMG + nYd + (wantRec ? nYd : 0) + epochs + 2) * sizeof(double);
  int chunk = 0;      // replicas per chunk (PSMF_BPMF_CHUNK: smaller chunks than memory asks for)
  PSMF_TRY(plan_chunk(fail, B, nYd * sizeof(double), per_rep, BPMF_MAX_REPLICAS, sw.bpmf_chunk, "replica", &chunk));

  Dev<double> dY, dMu, dMbar, dBart, dHz, dZ, dW, dP, dSum, dCov, dHyp, dPart, dAvg, dE, dRec;
  Dev<uint8_t> dM, dMiss;
  Dev<int> dBad;
  TimedLaunch timed;
  std::vector<int> bad((size_t)B, 0);
  const size_t nE = epochs, nHyp = 2 * BPMF_IMG;
  const auto items = std::make_tuple(      // buffer, filled from, read back to, elements per replica, cleared for every chunk
      item_slot(dM, M, nullptr, nYd), item_slot(dMiss, Mmiss, nullptr, nYd), item_slot(dMu, mean, nullptr, 1), item_slot(dMbar, mean_rating, nullptr, 1),
      item_slot(dBart, bartlett, nullptr, nBart), item_slot(dHz, hyper_normals, nullptr, nHz), item_slot(dZ, normals, nullptr, nZ),
      item_slot(dW, W, W, nW), item_slot(dP, P, P, nP), item_slot(dSum, nullptr, nullptr, nSum), item_slot(dCov, nullptr, nullptr, nCov),
      item_slot(dHyp, nullptr, nullptr, nHyp), item_slot(dPart, nullptr, nullptr, nPart), item_slot(dAvg, nullptr, nullptr, nYd),
      item_slot(dE, nullptr, Efull, nE), item_slot(dRec, nullptr, Yrec, wantRec ? nYd : 0, true), item_slot(dBad, nullptr, bad.data(), 1, true));
  const auto shared = std::make_tuple(slot(dY, Y, nullptr, nYd));      // what every chunk shares, filled once
  PSMF_TRY(alloc_all(fail, shared));
  PSMF_TRY(alloc_items(fail, items, chunk));
  PSMF_TRY(copy_in_all(fail, shared));
  PSMF_TRY(timed.create(fail));
  const size_t col_lds = bpmf_col_lds_doubles(d) * sizeof(double);
  PSMF_TRY(lds_opt_in(fail, (const void*)psmf_bpmf_col_kernel, col_lds));

  BpmfParams pp;
  pp.d = d; pp.n = n; pp.r = r; pp.cols = cols; pp.nwg = nwg; pp.epochs = epochs; pp.epoch = 0; pp.sweep = 0; pp.count = 0; pp.last = 0;
  pp.beta = cfg->beta;
  pp.Yt = dY; pp.M = dM; pp.miss = dMiss; pp.mu = dMu; pp.mbar = dMbar; pp.bart = dBart; pp.hz = dHz; pp.Z = dZ; pp.W = dW; pp.P = dP;
  pp.psum = dSum; pp.pcov = dCov; pp.hyp = dHyp; pp.part = dPart; pp.avg = dAvg; pp.efull = dE; pp.yrec = wantRec ? dRec.get() : nullptr;
  pp.bad = dBad;

  float total_ms = 0.0f;
  for (int s0 = 0; s0 < B; s0 += chunk) {      // s0: the chunk's first replica = its element offset in the host arrays, per replica
    const size_t ns = std::min(chunk, B - s0);
    const dim3 wide((unsigned)nwg, (unsigned)ns), one((unsigned)ns), block(BPMF_WG);
    PSMF_TRY(fill_items(fail, items, s0, ns));
    PSMF_TRY(timed.start(fail));
    pp.count = 0; pp.last = 0; pp.epoch = 0;
    PSMF_TRY(launch(fail, (const void*)psmf_bpmf_metric_kernel, one, block, &pp, 0));
    for (int e = 0; e < epochs; ++e) {
      pp.epoch = e;
      pp.count = e + 1;
      pp.last = e == epochs - 1;
      PSMF_TRY(launch(fail, (const void*)psmf_bpmf_wsum_kernel, wide, block, &pp, 0));
      PSMF_TRY(launch(fail, (const void*)psmf_bpmf_wcov_kernel, wide, block, &pp, 0));
      PSMF_TRY(launch(fail, (const void*)psmf_bpmf_hyper_kernel, one, block, &pp, 0));
      for (int s = 0; s < 2; ++s) {
        pp.sweep = s;
        PSMF_TRY(launch(fail, (const void*)psmf_bpmf_col_kernel, wide, block, &pp, col_lds));
        PSMF_TRY(launch(fail, (const void*)psmf_bpmf_row_part_kernel, wide, block, &pp, 0));
        PSMF_TRY(launch(fail, (const void*)psmf_bpmf_row_kernel, dim3((unsigned)((d + 15) / 16), (unsigned)ns), block, &pp, 0));
      }
      PSMF_TRY(launch(fail, (const void*)psmf_bpmf_metric_kernel, one, block, &pp, 0));
    }
    float ms = 0.0f;
    PSMF_TRY(timed.finish(fail, &ms));
    total_ms += ms;
    PSMF_TRY(read_items(fail, items, s0, ns));
  }
  if (elapsed_ms) *elapsed_ms = total_ms;
  // Per-replica outcome, as psmf_pmf_run: a replica with a pivot that was not positive, or whose factors or errors left the finite
  // range; the others are untouched by it.
  return replica_status(fail, B, status,
                        [&](int b) { return bad[b] != 0 || !(all_finite(W + b * nW, nW) && all_finite(P + b * nP, nP) && all_finite(Efull + b * nE, nE)); },
                        [](int b) { return "a precision matrix of replica " + std::to_string(b) + " is not positive definite (numpy.linalg.LinAlgError upstream)"; });
}

}  // namespace
}  // namespace psmf

extern "C" int psmf_bpmf_run(const psmf_bpmf_config* cfg, const double* Y, const uint8_t* M, const uint8_t* Mmiss, const double* mean,
                             const double* mean_rating, const double* bartlett, const double* hyper_normals, const double* normals, double* P,
                             double* W, double* Efull, double* Yrec, int32_t* status, float* elapsed_ms) {
  return psmf::bpmf_run(cfg, Y, M, Mmiss, mean, mean_rating, bartlett, hyper_normals, normals, P, W, Efull, Yrec, status, elapsed_ms);
}
