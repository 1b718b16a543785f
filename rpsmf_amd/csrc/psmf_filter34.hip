// The filter3 family of the blocked engine (psmf_blk_filter3 / 3s / 4 / 4s / 5) as a translation unit of its own: the headline
// kernel is compiled beside nothing but its siblings, and an edit of it recompiles this unit alone.
#include "psmf_host.h"
#include "psmf_blk34.hip"

// dynamic LDS beyond the default limit, on the handle's device (init_blocked)
int opt_in_lds_filter34(psmf_filter* h) {
  const size_t flds3 = psmf::blk_filter3_lds_bytes();
  const void* const kernels[] = {(const void*)psmf::psmf_blk_filter3, (const void*)psmf::psmf_blk_filter3s, (const void*)psmf::psmf_blk_filter4,
                                 (const void*)psmf::psmf_blk_filter4s, (const void*)psmf::psmf_blk_filter5};
  for (const void* fn : kernels) { const int rc = opt_in_lds(h, fn, flds3); if (rc) return rc; }
  return PSMF_OK;
}

void launch_blk_filter34(FilterKernel fk, const psmf::BlockParams& b, hipStream_t stream) {
  const size_t lds3 = psmf::blk_filter3_lds_bytes();
  switch (fk) {
    case FK_FILTER3: hipLaunchKernelGGL(psmf::psmf_blk_filter3, dim3(1), dim3(psmf::F3_NT), lds3, stream, b); return;
    case FK_FILTER3S: hipLaunchKernelGGL(psmf::psmf_blk_filter3s, dim3(1), dim3(psmf::F3_NT), lds3, stream, b); return;
    case FK_FILTER4: hipLaunchKernelGGL(psmf::psmf_blk_filter4, dim3(1), dim3(psmf::F3_NT), lds3, stream, b); return;
    case FK_FILTER4S: hipLaunchKernelGGL(psmf::psmf_blk_filter4s, dim3(1), dim3(psmf::F3_NT), lds3, stream, b); return;
    case FK_FILTER5: hipLaunchKernelGGL(psmf::psmf_blk_filter5, dim3(1), dim3(psmf::F3_NT), lds3, stream, b); return;
    default: return;      // (the other kernels: launch_blk_filter, psmf_blocked.hip)
  }
}
