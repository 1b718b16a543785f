// The four small kernels that the C ABI unit (psmf_capi.hip) launches itself: start and end of a run on the handle's DevState, the
// predict roll-out and the copy-bandwidth probe.  Included by that unit alone.
#pragma once
#include "psmf_device.h"

namespace psmf {

// start of a run: step counter.  The numeric-error flag is NOT cleared here: runs may be queued back to back without a
// sync in between, and a failure in an earlier one must still be reported by the next psmf_sync (cleared by psmf_set_state).
__global__ void psmf_prepare_k(DevState* st, long long k) { st->k = k; st->kq = k; st->ticket = 0u; if (st->ns_valid == 7) st->ns_valid = 0; }   // (7: the per-step engine's carried Lbar -- a new run re-derives it)
// end of a run: the numeric-error flag to mapped host memory (system-scope store)
__global__ void psmf_publish_err_k(const DevState* st, int* host_flag) { __hip_atomic_store(host_flag, st->err, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }

// ------------------------------------------------------------------------------------------
// predict roll-out: out[t][row] = C[row] . mu_pred[t]          psmf.py:182-188
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(WG) void psmf_predict_rows(const T* __restrict__ C, int d_local, int r, int rp,
                                                        const double* __restrict__ mu_pred, int n_pred,
                                                        double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_mu = reinterpret_cast<double*>(smem_raw);   // chunk of mu_pred rows
  const int row = blockIdx.x * WG + threadIdx.x;
  double c[RM];
  if (row < d_local)
    for (int l = 0; l < r; ++l) c[l] = (double)C[(size_t)row * rp + l];
  constexpr int TC = 64;
  for (int t0 = 0; t0 < n_pred; t0 += TC) {
    const int nt = min(TC, n_pred - t0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * r; idx += WG) s_mu[idx] = mu_pred[(size_t)t0 * r + idx];
    __syncthreads();
    if (row < d_local) {
      for (int t = 0; t < nt; ++t) {
        double a = 0.0;
        for (int l = 0; l < r; ++l) a += c[l] * s_mu[t * r + l];
        out[(size_t)(t0 + t) * d_local + row] = a;
      }
    }
  }
}

// plain streaming copy (16-byte accesses, grid-stride): the measured HBM bandwidth bench.py quotes beside the nominal peak
__global__ __launch_bounds__(WG) void psmf_copy_k(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16) {
  const size_t stride = (size_t)gridDim.x * WG;
  size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {      // four independent 16-byte loads in flight per thread
    const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) dst[i] = src[i];
}

}  // namespace psmf
