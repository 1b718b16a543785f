// Batched probabilistic matrix factorisation (the PMF baseline of the imputation experiment, ExperimentImpute/PMF.py:43-159: mini-batch
// gradient descent with momentum on the observed entries), float64 throughout, for a batch of independent replicas.  The recursion is
// written out at psmf_pmf_run in include/psmf_hip.h.
//
// The host hands over, per replica and epoch, a BATCH MAP: n x d bytes, time-major, the batch index of a training entry and 255
// elsewhere.  The order of the entries inside a batch only orders sums, so the map says everything the device needs.  Per batch b two
// launches on the null stream, and per epoch a third:
//
//   psmf_pmf_batch_kernel<NT, WAVES, LDSACC>   grid = (workgroups per replica, replicas).  A workgroup owns `cols` consecutive columns
//       of its replica and holds P (d x r, zero-padded to 16 NT x 16) in LDS; a wave takes the 16-column tiles wv, wv + WAVES, ...  The
//       three products of a tile run on v_mfma_f64_16x16x4_f64 (A operand: element (row lr, k-slot lk), B operand (k-slot lk, column lr),
//       result rows lk + 4 q of column lr; lr = lane & 15, lk = lane >> 4), row tile by row tile (16 rows i0 .. i0 + 15 of P):
//         S^T = P_tile W_tile^T   (K = r padded to a multiple of 4): the lane holds column j0 + lr, rows i0 + lk + 4 q
//         G   = map == b ? 2 (S - (v - mbar)) : 0,  v = (y - mu) / mu
//         dW_tile += G P_tile     (K = 16 rows): G as it stands IS the A operand -- slot lk of slice q is row i0 + 4 q + lk
//         S   = W_tile P_tile^T   the same operands the other way round: the lane holds row i0 + lr, columns j0 + lk + 4 q
//         dP_tile += G^T W_tile   (K = 16 columns): again G as it stands is the A operand
//       S is formed twice because dW contracts over rows and dP over columns: the matrix core contracts over the k-slot, so each product
//       wants G with ITS contracted index there, and two products of K <= 16 are cheaper than a transpose through LDS.  The tile of W and
//       incW is then updated in place by the wave (it has read all it needs of them; the number of batch entries of a column comes
//       from the lanes' hit counts).  The dP accumulators of a wave, 4 doubles a lane and row tile, are registers up to d = 256; at
//       d <= 512 (32 row tiles) they live in LDS and the workgroup is one wave.  At the end the waves add their dP into one LDS buffer
//       one after the other, in the order of their index, and the workgroup writes its partial sum to global memory.
//   psmf_pmf_p_kernel    grid = replicas: adds the partials of a replica's workgroups in the order of their index, then updates P and incP.
//   psmf_pmf_metric_kernel   grid = replicas, once per epoch: the squared error over the probe entries, every thread over a fixed set of
//       entries and a tree over the threads; with the last epoch, if asked for, the reconstruction at the probe entries.
//
// No atomics and no flags: the dependency between the batches is a whole-grid one, and launches express it.  Every sum has a fixed
// order, so a call gives the same bits twice, and a replica the same bits alone as inside a batch (the workgroups of a replica depend
// on n and PSMF_PMF_COLS alone).  Limits: d <= 512, r <= 16, num_batches <= 254; n is unlimited.  A batch whose buffers do not fit
// the device is processed in chunks of replicas (plan_chunk in psmf_batch.h).
#include "psmf_host.h"        // Switches
#include "psmf_batch.h"       // EntryFail, open_device, plan_chunk, per-item slots, TimedLaunch, cols_per_workgroup, all_finite, replica_status
#include "psmf_wave.h"        // f64x4

#include <algorithm>
#include <cmath>
#include <string>

namespace psmf {

constexpr int PMF_MAX_D = 512, PMF_MAX_R = 16, PMF_MAX_NB = 254;
constexpr int PMF_SP = 17;            // LDS row stride of P in doubles: 16 features and one of padding (the operand reads walk down rows)
constexpr int PMF_SMALL_WG = 256;     // the P and metric kernels
constexpr int PMF_MAX_REPLICAS = 65535;      // grid.y

struct PmfParams {
  int d, n, r, cols, nwg, nb, epochs, b, epoch, last;
  double lmd, momentum, epsilon;
  const double* Yt;            // n x d, time-major, shared by the replicas
  const uint8_t* map;          // replicas x epochs x n x d
  const uint8_t* miss;         // replicas x n x d
  const int* nbsize;           // replicas x nb: entries of a batch
  const int* rowcnt;           // replicas x epochs x nb x d: entries of a batch by row
  const double* mu;            // replicas
  const double* mbar;          // replicas
  double* W;                   // replicas x n x r
  double* incW;
  double* P;                   // replicas x d x r
  double* incP;
  double* part;                // replicas x nwg x d x r
  double* efull;               // replicas x epochs
  double* yrec;                // replicas x n x d or null
};

// LDS of the batch kernel in doubles: P, then either the dP accumulators of the one wave (4 a lane and row tile) or the buffer the
// waves add their dP into
__host__ __device__ constexpr size_t pmf_lds_doubles(int NT) { return (size_t)NT * 16 * PMF_SP + (size_t)NT * 256; }

template <int NT, int WAVES, bool LDSACC>
__global__ __launch_bounds__(WAVES * 64) void psmf_pmf_batch_kernel(PmfParams p) {
  static_assert(!LDSACC || WAVES == 1, "accumulators in LDS: one wave per workgroup");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sP = reinterpret_cast<double*>(smem_raw);      // (16 NT) x PMF_SP
  double* sAcc = sP + NT * 16 * PMF_SP;                  // LDSACC: [row tile][q][lane]; else [row][16 features], the waves' sum
  const int d = p.d, n = p.n, r = p.r, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int rep = blockIdx.y, wg = blockIdx.x;
  const int nk = (r + 3) >> 2;                           // k-slices of the products over the features
  const double* Pg = p.P + (size_t)rep * d * r;
  for (int idx = tid; idx < NT * 256; idx += WAVES * 64) {
    const int i = idx >> 4, k = idx & 15;
    sP[i * PMF_SP + k] = (i < d && k < r) ? Pg[i * r + k] : 0.0;
  }
  if constexpr (LDSACC)
    for (int idx = lane; idx < NT * 256; idx += 64) sAcc[idx] = 0.0;
  __syncthreads();
  const int c0 = wg * p.cols, c1 = min(n, c0 + p.cols), ntile = (c1 - c0 + 15) >> 4;
  const uint8_t bb = (uint8_t)p.b;
  const double mu = p.mu[rep], mbar = p.mbar[rep], lmd = p.lmd, mom = p.momentum, eps = p.epsilon;
  const double Nb = (double)p.nbsize[(size_t)rep * p.nb + p.b];
  const uint8_t* mapg = p.map + ((size_t)rep * p.epochs + p.epoch) * n * d;
  const double* Yt = p.Yt;
  double* Wg = p.W + (size_t)rep * n * r;
  double* Ig = p.incW + (size_t)rep * n * r;
  f64x4 dP[LDSACC ? 1 : NT];
  if constexpr (!LDSACC) {
#pragma unroll
    for (int it = 0; it < NT; ++it) dP[it] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  for (int tile = wv; tile < ntile; tile += WAVES) {
    const int j0 = c0 + 16 * tile, ja = j0 + lr;
    double wa[4], wb[4];      // W[ja][4 kq + lk] (operand of both S); W[j0 + 4 q + lk][lr] (operand of dP, and what the update reads)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = 4 * q + lk, j = j0 + 4 * q + lk;
      wa[q] = (ja < c1 && k < r) ? Wg[(size_t)ja * r + k] : 0.0;
      wb[q] = (j < c1 && lr < r) ? Wg[(size_t)j * r + lr] : 0.0;
    }
    f64x4 dW = {0.0, 0.0, 0.0, 0.0};
    int cnt = 0;              // batch entries of column ja in this lane's rows
#pragma unroll
    for (int it = 0; it < NT; ++it) {
      const int i0 = 16 * it;
      if (i0 < d) {           // (uniform)
        double pa[4];         // P[i0 + lr][4 kq + lk]
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) pa[kq] = sP[(i0 + lr) * PMF_SP + 4 * kq + lk];
        // S^T: this lane holds column ja, rows i0 + lk + 4 q
        f64x4 st = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kq = 0; kq < 4; ++kq)
          if (kq < nk) st = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kq], wa[kq], st, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + lk + 4 * q;
          double g = 0.0;
          if (ja < c1 && i < d && mapg[(size_t)ja * d + i] == bb) {
            const double v = (Yt[(size_t)ja * d + i] - mu) / mu;
            g = 2.0 * (st[q] - (v - mbar));
            ++cnt;
          }
          dW = __builtin_amdgcn_mfma_f64_16x16x4f64(g, sP[(i0 + 4 * q + lk) * PMF_SP + lr], dW, 0, 0, 0);
        }
        // S: this lane holds row i0 + lr, columns j0 + lk + 4 q
        f64x4 s2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kq = 0; kq < 4; ++kq)
          if (kq < nk) s2 = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[kq], pa[kq], s2, 0, 0, 0);
        f64x4 acc;
        if constexpr (LDSACC) {
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] = sAcc[(it * 4 + q) * 64 + lane];
        } else {
          acc = dP[it];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + lr, j = j0 + lk + 4 * q;
          double g = 0.0;
          if (j < c1 && i < d && mapg[(size_t)j * d + i] == bb) {
            const double v = (Yt[(size_t)j * d + i] - mu) / mu;
            g = 2.0 * (s2[q] - (v - mbar));
          }
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(g, wb[q], acc, 0, 0, 0);
        }
        if constexpr (LDSACC) {
#pragma unroll
          for (int q = 0; q < 4; ++q) sAcc[(it * 4 + q) * 64 + lane] = acc[q];
        } else {
          dP[it] = acc;
        }
      }
    }
    cnt += __shfl_xor(cnt, 16, 64);
    cnt += __shfl_xor(cnt, 32, 64);      // every lane of column ja: its batch entries over all rows
    // dW[q] = dW of column j0 + lk + 4 q, feature lr
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + lk + 4 * q;
      const int c = __shfl(cnt, lk + 4 * q, 64);
      if (j < c1 && lr < r) {
        const size_t idx = (size_t)j * r + lr;
        const double w = wb[q];
        const double dw = dW[q] + (lmd * (double)c) * w;
        const double inc = mom * Ig[idx] + (eps * dw) / Nb;
        Ig[idx] = inc;
        Wg[idx] = w - inc;
      }
    }
  }
  // the workgroup's dP: element (row 16 it + lk + 4 q, feature lr) of a wave's accumulators
  double* part = p.part + ((size_t)rep * p.nwg + wg) * d * r;
  if constexpr (LDSACC) {
#pragma unroll 4
    for (int it = 0; it < NT; ++it)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * it + lk + 4 * q;
        if (i < d && lr < r) part[i * r + lr] = sAcc[(it * 4 + q) * 64 + lane];
      }
  } else {
    for (int w = 0; w < WAVES; ++w) {
      if (wv == w) {
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int slot = (16 * it + lk + 4 * q) * 16 + lr;
            sAcc[slot] = w == 0 ? dP[it][q] : sAcc[slot] + dP[it][q];
          }
      }
      __syncthreads();
    }
    for (int idx = tid; idx < d * r; idx += WAVES * 64) {
      const int i = idx / r, k = idx - i * r;
      part[idx] = sAcc[i * 16 + k];
    }
  }
}

__global__ __launch_bounds__(PMF_SMALL_WG) void psmf_pmf_p_kernel(PmfParams p) {
  const int d = p.d, r = p.r, rep = blockIdx.x;
  const double Nb = (double)p.nbsize[(size_t)rep * p.nb + p.b];
  const int* rowcnt = p.rowcnt + (((size_t)rep * p.epochs + p.epoch) * p.nb + p.b) * d;
  const double* part = p.part + (size_t)rep * p.nwg * d * r;
  double* Pg = p.P + (size_t)rep * d * r;
  double* Ig = p.incP + (size_t)rep * d * r;
  for (int idx = threadIdx.x; idx < d * r; idx += PMF_SMALL_WG) {
    double s = 0.0;
    for (int w = 0; w < p.nwg; ++w) s += part[(size_t)w * d * r + idx];      // in the order of the workgroups
    const double pv = Pg[idx];
    const double dp = s + (p.lmd * (double)rowcnt[idx / r]) * pv;
    const double inc = p.momentum * Ig[idx] + (p.epsilon * dp) / Nb;
    Ig[idx] = inc;
    Pg[idx] = pv - inc;
  }
}

__global__ __launch_bounds__(PMF_SMALL_WG) void psmf_pmf_metric_kernel(PmfParams p) {
  __shared__ double ssum[PMF_SMALL_WG];
  __shared__ long long scnt[PMF_SMALL_WG];
  const int d = p.d, r = p.r, rep = blockIdx.x, tid = threadIdx.x;
  const size_t total = (size_t)p.n * d;
  const uint8_t* miss = p.miss + (size_t)rep * total;
  const double* Wg = p.W + (size_t)rep * p.n * r;
  const double* Pg = p.P + (size_t)rep * d * r;
  const double mu = p.mu[rep], mbar = p.mbar[rep];
  double* yrec = (p.yrec && p.last) ? p.yrec + (size_t)rep * total : nullptr;
  double acc = 0.0;
  long long cnt = 0;
  for (size_t e = tid; e < total; e += PMF_SMALL_WG) {
    if (miss[e] == 0) continue;
    const size_t j = e / d;
    const int i = (int)(e - j * d);
    double dot = 0.0;
    for (int k = 0; k < r; ++k) dot = fma(Wg[j * r + k], Pg[i * r + k], dot);
    const double yhat = (dot + mbar) * mu + mu;
    const double df = yhat - p.Yt[e];
    acc = fma(df, df, acc);
    ++cnt;
    if (yrec) yrec[e] = yhat;
  }
  ssum[tid] = acc;
  scnt[tid] = cnt;
  __syncthreads();
  for (int s = PMF_SMALL_WG / 2; s > 0; s >>= 1) {
    if (tid < s) { ssum[tid] += ssum[tid + s]; scnt[tid] += scnt[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) p.efull[(size_t)rep * p.epochs + p.epoch] = sqrt((1.0 / (double)scnt[0]) * ssum[0]);
}

namespace {

// row tiles of the instance that takes d, and its waves: accumulators in registers up to 16 row tiles
constexpr int pmf_row_tiles(int d) { return d <= 32 ? 2 : d <= 128 ? 8 : d <= 256 ? 16 : 32; }
constexpr int pmf_waves(int NT) { return NT <= 16 ? 4 : 1; }

template <int NT>
int pmf_launch_batch(const EntryFail& fail, const PmfParams& pp, int nrep) {
  constexpr int WAVES = pmf_waves(NT);
  constexpr size_t lds = pmf_lds_doubles(NT) * sizeof(double);
  static_assert(lds <= 160 * 1024, "P and the accumulators fit the LDS");
  const void* kern = (const void*)psmf_pmf_batch_kernel<NT, WAVES, (NT > 16)>;
  PSMF_TRY(lds_opt_in(fail, kern, lds));
  PmfParams q = pp;
  return launch(fail, kern, dim3((unsigned)pp.nwg, (unsigned)nrep), dim3(WAVES * 64), &q, lds);
}

int pmf_launch_batch_for(const EntryFail& fail, const PmfParams& pp, int nrep) {
  switch (pmf_row_tiles(pp.d)) {
    case 2: return pmf_launch_batch<2>(fail, pp, nrep);
    case 8: return pmf_launch_batch<8>(fail, pp, nrep);
    case 16: return pmf_launch_batch<16>(fail, pp, nrep);
    default: return pmf_launch_batch<32>(fail, pp, nrep);
  }
}

int pmf_run(const psmf_pmf_config* cfg, const double* Y, const uint8_t* maps, const uint8_t* Mmiss, const int32_t* batch_sizes,
            const int32_t* row_counts, const double* mean, const double* mean_rating, double* P, double* W, double* Efull, double* Yrec,
            int32_t* status, float* elapsed_ms) {
  const EntryFail fail{"psmf_pmf_run"};
  const Switches sw;      // no handle here: read at entry, on every call
  if (!cfg || !Y || !maps || !Mmiss || !batch_sizes || !row_counts || !mean || !mean_rating || !P || !W || !Efull) return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const int d = cfg->d, n = cfg->n, r = cfg->r, B = cfg->batch, epochs = cfg->epochs, nb = cfg->num_batches;
  if (d < 1 || d > PMF_MAX_D) return fail(PSMF_ERR_ARG, "need 1 <= d <= 512 (P lives in the LDS of one workgroup; d = " + std::to_string(d) + ")");
  if (r < 1 || r > PMF_MAX_R) return fail(PSMF_ERR_ARG, "need 1 <= r <= 16 (one matrix-core tile of features; r = " + std::to_string(r) + ")");
  if (n < 1 || B < 1 || epochs < 1) return fail(PSMF_ERR_ARG, "need n >= 1, batch >= 1 and epochs >= 1");
  if (nb < 1 || nb > PMF_MAX_NB) return fail(PSMF_ERR_ARG, "need 1 <= num_batches <= 254 (the batch map is bytes, 255 = no training entry; num_batches = " + std::to_string(nb) + ")");
  if (cfg->want_rec && !Yrec) return fail(PSMF_ERR_ARG, "want_rec needs Yrec");
  if (sw.pmf_cols < 0 || sw.pmf_chunk < 0) return fail(PSMF_ERR_ARG, "PSMF_PMF_COLS and PSMF_PMF_CHUNK must be >= 0 (0 = chosen by the library)");
  for (size_t i = 0; i < (size_t)B * nb; ++i)
    if (batch_sizes[i] < 1) return fail(PSMF_ERR_ARG, "an empty batch (the reference divides by its size): replica " + std::to_string(i / nb));
  for (int b = 0; b < B; ++b)
    if (mean[b] == 0.0 || !std::isfinite(mean[b])) return fail(PSMF_ERR_ARG, "the mean of the training entries is 0 or not finite in replica " + std::to_string(b) + " (the data is divided by it)");
  const bool wantRec = cfg->want_rec != 0;
  PSMF_TRY(open_device(fail, cfg->device));

  // columns per workgroup: a multiple of the 16-column tile; by default at least 16 tiles a wave (PSMF_PMF_COLS)
  const auto [cols, nwg] = cols_per_workgroup(n, sw.pmf_cols, 64 * pmf_waves(pmf_row_tiles(d)), 16);

  const size_t nYd = (size_t)n * d, nW = (size_t)n * r, nP = (size_t)d * r, nPart = (size_t)nwg * nP, nCnt = (size_t)epochs * nb * d;
  const size_t per_rep = (epochs * nYd + nYd) * sizeof(uint8_t) + (2 * nW + 2 * nP + nPart + (wantRec ? nYd : 0) + epochs + 2) * sizeof(double) +
                         (nCnt + nb) * sizeof(int);
  int chunk = 0;      // replicas per chunk (PSMF_PMF_CHUNK: smaller chunks than memory asks for)
  PSMF_TRY(plan_chunk(fail, B, nYd * sizeof(double), per_rep, PMF_MAX_REPLICAS, sw.pmf_chunk, "replica", &chunk));

  Dev<double> dY, dMu, dMbar, dW, dIncW, dP, dIncP, dPart, dE, dRec;
  Dev<uint8_t> dMap, dMiss;
  Dev<int> dNb, dCnt;
  TimedLaunch timed;
  const size_t nE = epochs, nNb = nb;
  const auto items = std::make_tuple(      // buffer, filled from, read back to, elements per replica, cleared for every chunk
      item_slot(dMap, maps, nullptr, nE * nYd), item_slot(dMiss, Mmiss, nullptr, nYd), item_slot(dNb, batch_sizes, nullptr, nNb),
      item_slot(dCnt, row_counts, nullptr, nCnt), item_slot(dMu, mean, nullptr, 1), item_slot(dMbar, mean_rating, nullptr, 1),
      item_slot(dW, W, W, nW), item_slot(dIncW, nullptr, nullptr, nW, true), item_slot(dP, P, P, nP), item_slot(dIncP, nullptr, nullptr, nP, true),
      item_slot(dPart, nullptr, nullptr, nPart), item_slot(dE, nullptr, Efull, nE), item_slot(dRec, nullptr, Yrec, wantRec ? nYd : 0, true));
  const auto shared = std::make_tuple(slot(dY, Y, nullptr, nYd));      // what every chunk shares, filled once
  PSMF_TRY(alloc_all(fail, shared));
  PSMF_TRY(alloc_items(fail, items, chunk));
  PSMF_TRY(copy_in_all(fail, shared));
  PSMF_TRY(timed.create(fail));

  PmfParams pp;
  pp.d = d; pp.n = n; pp.r = r; pp.cols = cols; pp.nwg = nwg; pp.nb = nb; pp.epochs = epochs; pp.b = 0; pp.epoch = 0; pp.last = 0;
  pp.lmd = cfg->lambda; pp.momentum = cfg->momentum; pp.epsilon = cfg->epsilon;
  pp.Yt = dY; pp.map = dMap; pp.miss = dMiss; pp.nbsize = dNb; pp.rowcnt = dCnt; pp.mu = dMu; pp.mbar = dMbar;
  pp.W = dW; pp.incW = dIncW; pp.P = dP; pp.incP = dIncP; pp.part = dPart; pp.efull = dE; pp.yrec = wantRec ? dRec.get() : nullptr;

  float total_ms = 0.0f;
  for (int s0 = 0; s0 < B; s0 += chunk) {      // s0: the chunk's first replica = its element offset in the host arrays, per replica
    const size_t ns = std::min(chunk, B - s0);
    PSMF_TRY(fill_items(fail, items, s0, ns));
    PSMF_TRY(timed.start(fail));
    for (int e = 0; e < epochs; ++e) {
      pp.epoch = e;
      pp.last = e == epochs - 1;
      for (int b = 0; b < nb; ++b) {
        pp.b = b;
        PSMF_TRY(pmf_launch_batch_for(fail, pp, (int)ns));
        PSMF_TRY(launch(fail, (const void*)psmf_pmf_p_kernel, dim3((unsigned)ns), dim3(PMF_SMALL_WG), &pp, 0));
      }
      PSMF_TRY(launch(fail, (const void*)psmf_pmf_metric_kernel, dim3((unsigned)ns), dim3(PMF_SMALL_WG), &pp, 0));
    }
    float ms = 0.0f;
    PSMF_TRY(timed.finish(fail, &ms));
    total_ms += ms;
    PSMF_TRY(read_items(fail, items, s0, ns));
  }
  if (elapsed_ms) *elapsed_ms = total_ms;
  // Per-replica outcome, as psmf_ssm_run: a replica whose factors or errors left the finite range; the others are untouched by it.
  return replica_status(fail, B, status, [&](int b) { return !(all_finite(W + b * nW, nW) && all_finite(P + b * nP, nP) && all_finite(Efull + b * nE, nE)); },
                        [](int b) { return "the factors or the error of replica " + std::to_string(b) + " are not finite (the gradient steps diverged)"; });
}

}  // namespace
}  // namespace psmf

extern "C" int psmf_pmf_run(const psmf_pmf_config* cfg, const double* Y, const uint8_t* maps, const uint8_t* Mmiss, const int32_t* batch_sizes,
                            const int32_t* row_counts, const double* mean, const double* mean_rating, double* P, double* W, double* Efull,
                            double* Yrec, int32_t* status, float* elapsed_ms) {
  return psmf::pmf_run(cfg, Y, maps, Mmiss, batch_sizes, row_counts, mean, mean_rating, P, W, Efull, Yrec, status, elapsed_ms);
}
