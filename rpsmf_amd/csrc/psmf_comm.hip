// The communicator of a sharded handle: RCCL, or host-mediated through a function of the caller's; the one exchange of the sharded
// engines (all_reduce_sum) and the psmf_comm_* entry points.  (psmf_destroy, psmf_capi.hip, destroys the RCCL communicator.)
#include "psmf_host.h"

#include <cstring>
#include <string>

// The one exchange of the sharded engines: in-place sum of `count` float64 on the device over all ranks.  RCCL on the given
// stream, or -- host-mediated communicator -- device -> pinned host -> caller's function -> device, synchronously.
int all_reduce_sum(psmf_filter* h, double* buf, size_t count, hipStream_t s) {
  if (h->host_fn) {
    if (count > psmf_filter::kHostBufElems) return fail(h, PSMF_ERR_ARG, "host all-reduce: message larger than the staging buffer");
    HIP_TRY(h, hipMemcpyAsync(h->host_buf, buf, count * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, spin_stream(s));
    if (h->host_fn(h->host_ctx, h->host_buf, (int64_t)count) != 0) return fail(h, PSMF_ERR_RCCL, "host all-reduce callback reported a failure");
    HIP_TRY(h, hipMemcpyAsync(buf, h->host_buf, count * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, spin_stream(s));        // the staging buffer is reused by the next call
    return PSMF_OK;
  }
  NCCL_TRY(h, ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, h->comm, s));
  return PSMF_OK;
}

extern "C" {

int psmf_comm_unique_id(void* id_out) {
  if (!id_out) return PSMF_ERR_ARG;
  static_assert(sizeof(ncclUniqueId) <= PSMF_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return fail(nullptr, PSMF_ERR_RCCL, "ncclGetUniqueId failed");
  memset(id_out, 0, PSMF_UNIQUE_ID_BYTES);
  memcpy(id_out, &id, sizeof(id));
  return PSMF_OK;
}

int psmf_comm_init(psmf_handle h, int nranks, int rank, const void* unique_id) {
  if (!h || !unique_id || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, PSMF_ERR_ARG, "psmf_comm_init: bad argument");
  if (h->rotU) return fail(h, PSMF_ERR_STATE, "psmf_comm_init: a handle with a noise rotation (non-diagonal R) is one shard by construction");
  int rc = set_device(h);
  if (rc) return rc;
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  NCCL_TRY(h, ncclCommInitRank(&h->comm, nranks, id, rank));
  h->nranks = nranks;
  h->rank = rank;
  {
    // Connect now: the first collective of each message size sets up its channels (seconds on 8 GPUs), and in the pipelined
    // block engine a filter kernel would be polling for its result meanwhile.  Same sizes, same streams as the engines use.
    const size_t xg_elems = (size_t)(psmf::RB + psmf::XGB) * psmf::XGB;
    Dev<double> tmp;
    ALLOC_TRY(h, tmp.alloc(xg_elems * sizeof(double)));
    HIP_TRY(h, hipMemsetAsync(tmp, 0, xg_elems * sizeof(double), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t sizes[4] = {(size_t)h->cfg.r + 1, (size_t)h->cfg.r * h->cfg.r, (size_t)psmf::RB * psmf::RB, xg_elems};
    hipStream_t streams[2] = {h->stream, h->bulk};
    for (int si = 0; si < 2; ++si) {
      if (!streams[si]) continue;
      for (int zi = 0; zi < 4; ++zi) {
        const ncclResult_t e = ncclAllReduce(tmp, tmp, sizes[zi], ncclDouble, ncclSum, h->comm, streams[si]);
        if (e != ncclSuccess) return fail(h, PSMF_ERR_RCCL, std::string("warm-up all-reduce: ") + ncclGetErrorString(e));
      }
      const hipError_t he = hipStreamSynchronize(streams[si]);
      if (he != hipSuccess) return fail(h, PSMF_ERR_HIP, std::string("warm-up all-reduce: ") + hipGetErrorString(he));
    }
  }
  h->use_coll = nranks > 1 || h->sw.force_collective;
  h->sp.external_reduce = (h->use_coll || h->sp.tail_reduce) ? 1 : 0;
  destroy_graph(h);
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_comm_abort(psmf_handle h) {
  if (!h) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  if (h->comm) {
    // ncclCommAbort, not ncclCommDestroy: destroy waits for outstanding work and for its peers, and the caller is here because
    // some peer never joined (or stopped answering)
    const ncclResult_t e = ncclCommAbort(h->comm);
    h->comm = nullptr;
    if (e != ncclSuccess) return fail(h, PSMF_ERR_RCCL, std::string("ncclCommAbort: ") + ncclGetErrorString(e));
  }
  h->nranks = 1; h->rank = 0;
  h->use_coll = false;
  h->sp.external_reduce = h->sp.tail_reduce;
  destroy_graph(h);
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_comm_info(psmf_handle h, int32_t* out4) {
  if (!h || !out4) return PSMF_ERR_ARG;
  out4[0] = h->host_fn ? 2 : (h->comm ? 1 : 0);
  out4[1] = h->nranks; out4[2] = h->rank; out4[3] = h->cfg.device;
  if (h->comm) {          // what RCCL itself says about the communicator the exchanges run on
    int n = -1, rk = -1, dev = -1;
    NCCL_TRY(h, ncclCommCount(h->comm, &n));
    NCCL_TRY(h, ncclCommUserRank(h->comm, &rk));
    NCCL_TRY(h, ncclCommCuDevice(h->comm, &dev));
    out4[1] = n; out4[2] = rk; out4[3] = dev;
  }
  return PSMF_OK;
}

int psmf_comm_init_host(psmf_handle h, int nranks, int rank, psmf_allreduce_fn fn, void* ctx) {
  if (!h || !fn || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, PSMF_ERR_ARG, "psmf_comm_init_host: bad argument");
  if (h->rotU) return fail(h, PSMF_ERR_STATE, "psmf_comm_init_host: a handle with a noise rotation (non-diagonal R) is one shard by construction");
  if (h->comm) return fail(h, PSMF_ERR_STATE, "psmf_comm_init_host: the handle already has an RCCL communicator");
  int rc = set_device(h);
  if (rc) return rc;
  if (!h->host_buf) HIP_TRY(h, hipHostMalloc(h->host_buf.put(), psmf_filter::kHostBufElems * sizeof(double), hipHostMallocDefault));
  h->host_fn = fn;
  h->host_ctx = ctx;
  h->nranks = nranks;
  h->rank = rank;
  h->use_coll = true;               // also with one rank: the exchange path is what this communicator exists to exercise
  h->sp.external_reduce = 1;
  destroy_graph(h);
  h->need_prep = true;
  return PSMF_OK;
}

}  // extern "C"
