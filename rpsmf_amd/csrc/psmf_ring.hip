// Series ring (psmf_series_ring): row conversion on the device.  A ring upload whose element type differs from the
// handle's storage type lands in a device staging buffer as it is and is converted here, on the ring's copy stream; y_hat downloads
// go the other way.  Launched by psmf_capi.hip only.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace psmf
