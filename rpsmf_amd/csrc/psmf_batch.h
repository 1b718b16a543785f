// Host scaffold of an entry point without a handle (psmf_impute_run*, psmf_ssm_run*, psmf_bocpd_run, psmf_pmf_run, psmf_bpmf_run): the
// failure functor, the device check, typed transfers, the chunk plan and the per-item slots of a call that takes its batch in chunks,
// the timed launch and the closing status loop.  Every function returns PSMF_OK or what `fail` returned, so a call site is
// PSMF_TRY(...).  The byte count of a transfer comes from the buffer's element type and from nowhere else, and a transfer larger
// than the buffer is refused.  What allocates, what moves or clears the bytes and what reports the free memory are parameters (the
// buffer's type, `Copy`, `Zero`, `Query`): tests/native/batch_check.cpp instantiates the same text over memcpy, counting allocators
// and a made-up device.  Needs nothing of psmf_host.h.
#pragma once
#include "../../include/psmf_hip.h"
#include "psmf_own.h"         // Event, Dev<T>, kAllocCall

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <tuple>
#include <type_traits>

extern thread_local std::string g_create_error;      // the message of a failure without a handle (psmf_capi.hip)

#define PSMF_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// Every message starts with "who: ".  The three-argument form is the one HIP_TRY / ALLOC_TRY call.
struct EntryFail {
  const char* who;
  int operator()(int code, const std::string& msg) const { g_create_error = std::string(who) + ": " + msg; return code; }
  int operator()(psmf_handle, int code, const std::string& msg) const { return (*this)(code, msg); }
};

// a HIP call's outcome as a PSMF code; `call` names the HIP function for the message (HIP_OK: the call as it is written)
template <typename F> int hip_ok(const F& fail, const std::string& call, hipError_t e) {
  return e == hipSuccess ? PSMF_OK : fail(PSMF_ERR_HIP, call + ": " + hipGetErrorString(e));
}
#define HIP_OK(fail, expr) hip_ok(fail, #expr, expr)

template <typename F> int open_device(const F& fail, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PSMF_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PSMF_ERR_ARG, "bad device ordinal");
  return HIP_OK(fail, hipSetDevice(device));
}

// ---- typed transfers: `count` is in elements of the buffer's type; B is a Dev<T>, or any Buf with a typed get() ----
template <typename B> using elem_t = std::remove_pointer_t<decltype(std::declval<const B&>().get())>;
using CopyFn = hipError_t (*)(void*, const void*, size_t, hipMemcpyKind);
using ZeroFn = hipError_t (*)(void*, int, size_t);
using MemInfoFn = hipError_t (*)(size_t*, size_t*);

template <typename F, typename B> int alloc_n(const F& fail, B& buf, size_t count) {
  const size_t bytes = count * sizeof(elem_t<B>);
  return hip_ok(fail, std::string(kAllocCall) + " of " + std::to_string(bytes) + " bytes", buf.alloc(bytes));
}
template <typename F, typename B> int fits(const F& fail, const B& buf, size_t count) {
  if (count * sizeof(elem_t<B>) <= buf.bytes()) return PSMF_OK;
  return fail(PSMF_ERR_HIP, "internal error: a transfer of " + std::to_string(count * sizeof(elem_t<B>)) + " bytes on a buffer of " + std::to_string(buf.bytes()));
}
// host[offset .. offset + count) -> the front of the buffer (offset: where the chunk of a batch that the buffer holds begins)
template <CopyFn Copy = hipMemcpy, typename F, typename B> int copy_in(const F& fail, B& buf, const elem_t<B>* host, size_t count, size_t offset = 0) {
  PSMF_TRY(fits(fail, buf, count));
  return hip_ok(fail, "hipMemcpy, host to device", Copy(buf.get(), host + offset, count * sizeof(elem_t<B>), hipMemcpyHostToDevice));
}
template <CopyFn Copy = hipMemcpy, typename F, typename B> int alloc_copy_in(const F& fail, B& buf, const elem_t<B>* host, size_t count) {
  PSMF_TRY(alloc_n(fail, buf, count));
  return copy_in<Copy>(fail, buf, host, count);
}
// the front of the buffer -> host[offset .. offset + count)
template <CopyFn Copy = hipMemcpy, typename F, typename B> int copy_out(const F& fail, elem_t<B>* host, const B& buf, size_t count, size_t offset = 0) {
  PSMF_TRY(fits(fail, buf, count));
  return hip_ok(fail, "hipMemcpy, device to host", Copy(host + offset, buf.get(), count * sizeof(elem_t<B>), hipMemcpyDeviceToHost));
}
template <ZeroFn Zero = hipMemset, typename F, typename B> int zero_n(const F& fail, B& buf, size_t count) {
  PSMF_TRY(fits(fail, buf, count));
  return hip_ok(fail, "hipMemset(buf.get(), 0, count * sizeof(elem_t<B>))", Zero(buf.get(), 0, count * sizeof(elem_t<B>)));
}

// A buffer of a call, stated once: what it is filled from (or null), where it is read back to (or null), its count (0: not part of
// this call).  A tuple of them is allocated, filled and read back in the order it is written.
template <typename B> struct Slot { B& buf; const elem_t<B>* in; elem_t<B>* out; size_t count; };
template <typename B> Slot<B> slot(B& buf, const elem_t<B>* in, elem_t<B>* out, size_t count) { return {buf, in, out, count}; }
template <typename Step, typename... S> int each_slot(const std::tuple<S...>& io, Step step) {      // stops at the first failure
  return std::apply([&](const S&... s) { int rc = PSMF_OK; ((rc = rc ? rc : step(s)), ...); return rc; }, io);
}
template <typename F, typename... S> int alloc_all(const F& fail, const std::tuple<S...>& io) {
  return each_slot(io, [&](const auto& s) { return s.count ? alloc_n(fail, s.buf, s.count) : PSMF_OK; });
}
template <CopyFn Copy = hipMemcpy, typename F, typename... S> int copy_in_all(const F& fail, const std::tuple<S...>& io) {
  return each_slot(io, [&](const auto& s) { return s.count && s.in ? copy_in<Copy>(fail, s.buf, s.in, s.count) : PSMF_OK; });
}
template <CopyFn Copy = hipMemcpy, typename F, typename... S> int copy_out_all(const F& fail, const std::tuple<S...>& io) {
  return each_slot(io, [&](const auto& s) { return s.count && s.out ? copy_out<Copy>(fail, s.out, s.buf, s.count) : PSMF_OK; });
}

// ---- a batch in chunks: when the buffers of all B items may not fit the device, the call takes `chunk` items at a time ----
// Items per chunk.  The budget is half of the free device memory, at most 16 GiB; the buffers every chunk shares and those of one item
// have to fit it (the call fails otherwise: "one <noun> needs ..."); then as many items as fit, at most B and max_items (a grid
// dimension; kNoItemCap: none).  A switch > 0 lowers the result and never raises it.
constexpr int kNoItemCap = INT_MAX;
template <MemInfoFn Query = hipMemGetInfo, typename F>
int plan_chunk(const F& fail, int B, size_t shared_bytes, size_t per_item_bytes, int max_items, int switch_value, const char* noun, int* chunk) {
  size_t free_b = 0, total_b = 0;
  PSMF_TRY(hip_ok(fail, "hipMemGetInfo(&free_b, &total_b)", Query(&free_b, &total_b)));
  const size_t budget = std::min(free_b / 2, (size_t)16 << 30);
  if (shared_bytes + per_item_bytes > budget)
    return fail(PSMF_ERR_HIP, std::string("one ") + noun + " needs " + std::to_string(shared_bytes + per_item_bytes) + " bytes of device memory, more than is free");
  *chunk = (int)std::min({(size_t)B, (size_t)max_items, (budget - shared_bytes) / per_item_bytes});
  if (switch_value > 0) *chunk = std::min(*chunk, switch_value);
  return PSMF_OK;
}

// A per-item buffer of such a call, stated once: the host array a chunk's items are filled from (or null) and the one they are read
// back to (or null), both indexed by item over the whole batch; the elements per item (0: not part of this call); whether the
// chunk's part is cleared before its kernels; and `extra` elements behind the items', allocated and cleared with them (a buffer
// that has to exist where an item has none).  A tuple of them is allocated for `chunk` items; a chunk is its first item s0 and its
// ns <= chunk items, which lie at the front of the buffer and at host + s0 * per.
template <typename B> struct ItemSlot { B& buf; const elem_t<B>* in; elem_t<B>* out; size_t per; bool zero; size_t extra; };
template <typename B> ItemSlot<B> item_slot(B& buf, const elem_t<B>* in, elem_t<B>* out, size_t per, bool zero = false, size_t extra = 0) {
  return {buf, in, out, per, zero, extra};
}
template <typename F, typename... S> int alloc_items(const F& fail, const std::tuple<S...>& io, size_t chunk) {
  return each_slot(io, [&](const auto& s) { return s.per + s.extra ? alloc_n(fail, s.buf, chunk * s.per + s.extra) : PSMF_OK; });
}
template <CopyFn Copy = hipMemcpy, ZeroFn Zero = hipMemset, typename F, typename... S>
int fill_items(const F& fail, const std::tuple<S...>& io, size_t s0, size_t ns) {      // every copy, then every clearing
  PSMF_TRY(each_slot(io, [&](const auto& s) { return s.per && s.in ? copy_in<Copy>(fail, s.buf, s.in, ns * s.per, s0 * s.per) : PSMF_OK; }));
  return each_slot(io, [&](const auto& s) { return s.zero && s.per + s.extra ? zero_n<Zero>(fail, s.buf, ns * s.per + s.extra) : PSMF_OK; });
}
template <CopyFn Copy = hipMemcpy, typename F, typename... S> int read_items(const F& fail, const std::tuple<S...>& io, size_t s0, size_t ns) {
  return each_slot(io, [&](const auto& s) { return s.per && s.out ? copy_out<Copy>(fail, s.out, s.buf, ns * s.per, s0 * s.per) : PSMF_OK; });
}

// ---- launch: a kernel that takes one parameter struct, on the null stream; above 48 KB its dynamic LDS has to be asked for first ----
template <typename F> int lds_opt_in(const F& fail, const void* kern, size_t lds) {
  return lds > 48 * 1024 ? HIP_OK(fail, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) : PSMF_OK;
}
template <typename F> int launch(const F& fail, const void* kern, dim3 grid, dim3 block, void* params, size_t lds) {
  void* args[] = {params};
  return HIP_OK(fail, hipLaunchKernel(kern, grid, block, args, lds, 0));
}

// Columns of a replica per workgroup, and workgroups per replica, of a kernel whose grid is (workgroups, replicas): the switch's
// value or, by default, at most 64 workgroups a replica and at least `floor` columns each; rounded up to the granule (the columns a
// wave takes at a time) and capped at n rounded up.
struct ColsPlan { int cols, nwg; };
inline ColsPlan cols_per_workgroup(int n, int switch_value, int floor, int granule) {
  const auto up = [granule](long long v) { return (v + granule - 1) / granule * granule; };
  const long long cols = std::min(up(switch_value > 0 ? switch_value : std::max(floor, (n + 63) / 64)), up(n));
  return {(int)cols, (int)((n + cols - 1) / cols)};
}

// The event pair around the kernels of a call.  run() is the whole of it for one kernel: LDS opt-in, events, launch, wait.  An entry
// point with several kernels between one pair (psmf_bocpd_run, per chunk) calls create() once, then start(), its launches, finish().
struct TimedLaunch {
  Event e0, e1;
  template <typename F> int create(const F& fail) {
    PSMF_TRY(HIP_OK(fail, hipEventCreate(e0.put())));
    return HIP_OK(fail, hipEventCreate(e1.put()));
  }
  template <typename F> int start(const F& fail) { return HIP_OK(fail, hipEventRecord(e0, 0)); }
  template <typename F> int finish(const F& fail, float* ms) {      // waits for the kernels; *ms (may be null) = the time since start()
    PSMF_TRY(HIP_OK(fail, hipGetLastError()));
    PSMF_TRY(HIP_OK(fail, hipEventRecord(e1, 0)));
    PSMF_TRY(HIP_OK(fail, hipEventSynchronize(e1)));
    return ms ? HIP_OK(fail, hipEventElapsedTime(ms, e0, e1)) : PSMF_OK;
  }
  template <typename F> int run(const F& fail, const void* kern, dim3 grid, dim3 block, void* params, size_t lds, float* ms) {
    PSMF_TRY(lds_opt_in(fail, kern, lds));
    PSMF_TRY(create(fail));
    PSMF_TRY(start(fail));
    PSMF_TRY(launch(fail, kern, grid, block, params, lds));
    return finish(fail, ms);
  }
};

inline bool all_finite(const double* v, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// The closing loop: status[b] = PSMF_ERR_NUMERIC where bad(b), PSMF_OK elsewhere; without a status array the first bad replica fails
// the call with message(b).
template <typename F, typename Bad, typename Msg> int replica_status(const F& fail, int B, int32_t* status, Bad bad, Msg message) {
  for (int b = 0; b < B; ++b) {
    const bool is_bad = bad(b);
    if (status) status[b] = is_bad ? PSMF_ERR_NUMERIC : PSMF_OK;
    if (is_bad && !status) return fail(PSMF_ERR_NUMERIC, message(b));
  }
  return PSMF_OK;
}
