// Device code of the series unit (psmf_series.hip, the only file that includes this one and the only one that launches these kernels):
// what reads or converts rows of the series buffers outside a filter step.
//   psmf_cast_rows          series ring (psmf_series_ring): row conversion on the device.  A ring upload whose element
//                           type differs from the handle's storage type lands in a device staging buffer as it is and is converted here,
//                           on the ring's copy stream; y_hat downloads go the other way.
//   psmf_sq_error_k         sum of squared prediction errors over a range of steps (psmf_sq_error, psmf_predict_sq_error)
//   psmf_masked_metrics_k   the metrics of a masked pass over the held-out entries (psmf_masked_metrics; the filter: psmf_masked.hip)
#pragma once
#include "psmf_device.h"      // StepParams, WG, RM, wave_sum

#include <cstddef>
#include <cstdint>

namespace psmf {

constexpr int CAST_NT = 256;

// dst[i] = (TD)src[i], i < n; float64 -> float32 (round to nearest even, as numpy's astype) or float32 -> float64.  Four elements
// per pass and thread: 16-byte loads and stores (two loads, one store, or one load, two stores).  A row of the ring buffers starts
// at any element, so the first `head` elements are copied one by one and the CALLER places the staging side so that src + head and
// dst + head both sit on a 16-byte boundary (cast_head / cast_shift); the odd remainder is a scalar tail.  Grid-stride.
template <typename TS, typename TD>
__global__ __launch_bounds__(CAST_NT) void psmf_cast_rows(const TS* __restrict__ src, TD* __restrict__ dst, size_t n, int head) {
  static_assert(sizeof(TS) != sizeof(TD) && sizeof(TS) + sizeof(TD) == 12, "float <-> double");
  const size_t tid = (size_t)blockIdx.x * CAST_NT + threadIdx.x, nthr = (size_t)gridDim.x * CAST_NT;
  const size_t h = (size_t)head < n ? (size_t)head : n;
  const size_t nv = (n - h) / 4;
  const TS* __restrict__ s = src + h;
  TD* __restrict__ d = dst + h;
  for (size_t v = tid; v < nv; v += nthr) {
    if constexpr (sizeof(TS) == 8) {
      const double2 a = reinterpret_cast<const double2*>(s)[2 * v], b = reinterpret_cast<const double2*>(s)[2 * v + 1];
      reinterpret_cast<float4*>(d)[v] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
    } else {
      const float4 a = reinterpret_cast<const float4*>(s)[v];
      reinterpret_cast<double2*>(d)[2 * v] = make_double2((double)a.x, (double)a.y);
      reinterpret_cast<double2*>(d)[2 * v + 1] = make_double2((double)a.z, (double)a.w);
    }
  }
  const size_t body_end = h + 4 * nv, nrest = h + (n - body_end);      // head and tail, one element per thread
  for (size_t i = tid; i < nrest; i += nthr) {
    const size_t e = i < h ? i : body_end + (i - h);
    dst[e] = (TD)src[e];
  }
}

// elements of `es` bytes in front of p's next 16-byte boundary (p is a multiple of es)
inline int cast_head(const void* p, size_t es) { return (int)(((16 - ((uintptr_t)p & 15)) & 15) / es); }
// where, in elements of `es` bytes behind a 16-byte boundary, the other side has to start for its element `head` to sit on one too
inline int cast_shift(int head, size_t es) { const int per = (int)(16 / es); return (per - head % per) % per; }

// sum of squared prediction errors over a block of steps (tracking.py:63-76 norms)
template <typename T>
__global__ __launch_bounds__(WG) void psmf_sq_error_k(const T* __restrict__ YP, const T* __restrict__ Y, size_t n,
                                                      double* __restrict__ part) {
  __shared__ double s4[4];
  double a = 0.0;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const double dlt = (double)YP[i] - (double)Y[i];
    a += dlt * dlt;
  }
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// Metrics of a pass over the held-out entries (Mmiss = 1) of this handle's rows, steps t0 .. t0 + nt:
//   part[blk][0] = sum (y_hat - y)^2        (Epred^2 * count, PSMF.py:88)       y_hat = the stored (unmasked) predictions
//   part[blk][1] = sum (c_i . x_t - y)^2    (Efull^2 * count, PSMF.py:86-89)    final C of the pass, x_t = mu_hist[t + 1]
//   part[blk][2] = number of entries strictly inside their band (common.py:87-94)
//   part[blk][3] = number of held-out entries
// grid = (row blocks, time chunks); a thread owns one row (its C row in registers) and walks its chunk of steps.
template <typename T>
__global__ __launch_bounds__(WG) void psmf_masked_metrics_k(StepParams p, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ mmiss,
                                                            const double* __restrict__ sc_hist, long long t0, int nt, int chunk, double sig,
                                                            int robust, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_x = reinterpret_cast<double*>(smem_raw);          // TC x r rows of the mean history
  __shared__ double s_red[4][4];
  const int tid = threadIdx.x, r = p.r, rp = p.rp, d_local = p.d_local;
  const int row = blockIdx.x * WG + tid;
  const bool on = row < d_local;
  const T* __restrict__ C = reinterpret_cast<const T*>(p.C);
  const T* __restrict__ Y = reinterpret_cast<const T*>(p.Y);
  const T* __restrict__ YP = reinterpret_cast<const T*>(p.YP);
  double c[RM];
  for (int l = 0; l < r; ++l) c[l] = on ? (double)C[(size_t)row * rp + l] : 0.0;
  double a_pred = 0.0, a_full = 0.0, a_in = 0.0, a_cnt = 0.0;
  const int tb = blockIdx.y * chunk, te = min(tb + chunk, nt);
  constexpr int TC = 32;
  for (int q0 = tb; q0 < te; q0 += TC) {
    const int nq = min(TC, te - q0);
    __syncthreads();
    for (int idx = tid; idx < nq * r; idx += WG) s_x[idx] = p.mu_hist[(size_t)(t0 + q0 + 1 - p.series_t0) * r + idx];   // row t + 1 = x_t
    __syncthreads();
    if (on) {
      for (int q = 0; q < nq; ++q) {
        const size_t t = (size_t)(t0 + q0 + q - p.series_t0);
        const size_t at = t * d_local + row;
        if (mmiss[(size_t)(q0 + q) * d_local + row]) {
          const double y = (double)Y[at], yh = (double)YP[at];
          double dot = 0.0;
          for (int l = 0; l < r; ++l) dot += c[l] * s_x[q * r + l];
          const double s = sc_hist[2 * t], eta = sc_hist[2 * t + 1];
          const double band = sig * sqrt(robust ? (mask[at] ? s : 0.0) + eta : s + eta);
          a_pred += (yh - y) * (yh - y);
          a_full += (dot - y) * (dot - y);
          a_in += (y < yh + band && yh - band < y) ? 1.0 : 0.0;
          a_cnt += 1.0;
        }
      }
    }
  }
  a_pred = wave_sum(a_pred); a_full = wave_sum(a_full); a_in = wave_sum(a_in); a_cnt = wave_sum(a_cnt);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = a_pred; s_red[tid >> 6][1] = a_full; s_red[tid >> 6][2] = a_in; s_red[tid >> 6][3] = a_cnt; }
  __syncthreads();
  if (tid < 4) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

}  // namespace psmf
