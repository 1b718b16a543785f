// C ABI of libpsmf_hip.so (include/psmf_hip.h): host-side orchestration of the large-d engine.
// One handle = one HIP stream, one device-resident filter (or row shard), one hipGraph of
// per-step launches replayed over the series.  No torch, no hipBLAS: plain HIP + RCCL.
// The batched entry points without a handle (psmf_impute_*, psmf_ssm_*, psmf_bocpd_run) live in the units of their engines.
#include "psmf_host.h"
#include "psmf_kernels.hip"
#include "psmf_masked.hip"
#include "psmf_rotate.hip"
#include "psmf_wave16.hip"     // solve_block_wave: the per-step engine's solve block

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

thread_local std::string g_create_error;

namespace {

#ifndef PSMF_SWEEP_UNROLL
#define PSMF_SWEEP_UNROLL 4
#endif
constexpr int kUnroll = PSMF_SWEEP_UNROLL;      // row passes (16-byte loads per lane) in flight in the sweep
constexpr int kGramWG = 128;

}  // namespace

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

namespace {

int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// A kernel whose dynamic LDS may need the opt-in (hipFuncAttributeMaxDynamicSharedMemorySize): psmf_create sets it for the
// kernels the handle can launch (opt_in_lds), on the handle's device; the launchers only launch.
template <typename Fn>
struct LdsKernel { Fn fn; int threads; size_t lds; };

typedef void (*sweep_fn_t)(StepParams);
typedef void (*serial_fn_t)(StepParams, int);

// loads in flight per lane of the row sweep.  The 256-thread instances of r > 32 (GS lanes x VEC elements > 32 columns) run ONE wave
// per SIMD -- their solve block keeps 3 x 3 / 4 x 4 tile arrays in a wave's 512 registers, and a kernel has one register allocation --
// so the row workgroups make up in depth what they lack in occupancy: 16 passes in flight instead of 4 (rows alone at d = 2e4, r = 40:
// 17.5 us -> see docs/MEASUREMENTS.md).
template <typename T, int GS, int NT>
constexpr int sweep_unroll() { return (NT == 256 && GS * (int)(16 / sizeof(T)) > 32) ? 16 : kUnroll; }

template <typename T, int NT>
sweep_fn_t sweep_for_gs(int gs) {
  switch (gs) {
    case 1: return psmf::psmf_sweep_solve<T, 1, kUnroll, NT>;
    case 2: return psmf::psmf_sweep_solve<T, 2, kUnroll, NT>;
    case 4: return psmf::psmf_sweep_solve<T, 4, kUnroll, NT>;
    case 8: return psmf::psmf_sweep_solve<T, 8, kUnroll, NT>;
    case 16: return psmf::psmf_sweep_solve<T, 16, sweep_unroll<T, 16, NT>(), NT>;
    case 32: return psmf::psmf_sweep_solve<T, 32, sweep_unroll<T, 32, NT>(), NT>;
  }
  return nullptr;
}

// threads per sweep workgroup (tuning knob PSMF_SWEEP_THREADS=256|512): 512 halves the number of
// per-workgroup partial rows the serial stage has to read at the same number of waves per CU
sweep_fn_t sweep_kernel(const psmf_filter* h) {
  const int gs = h->geo.gs;
  return by_storage(h, [&](auto t) { return h->geo.nt == 512 ? sweep_for_gs<decltype(t), 512>(gs) : sweep_for_gs<decltype(t), 256>(gs); });
}

bool serial_wide(const psmf_filter* h) { return h->geo.rpad >= 64 && h->sw.serial_wide; }

serial_fn_t serial_kernel(const psmf_filter* h) {
  switch (h->geo.rpad) {
    case 8: return psmf::psmf_serial<8>;
    case 16: return psmf::psmf_serial<16>;
    case 32: return psmf::psmf_serial<32>;
    default: return serial_wide(h) ? psmf::psmf_serial_wide : psmf::psmf_serial<64>;
  }
}

void launch_sweep(psmf_filter* h) {
  const int grid = h->geo.n_sweep_wg + (h->cfg.coef_update ? 1 : 0);
  hipLaunchKernelGGL(sweep_kernel(h), dim3(grid), dim3(h->geo.nt), h->geo.sweep_lds, h->stream, h->sp);
}

void launch_serial(psmf_filter* h, int first) {
  hipLaunchKernelGGL(serial_kernel(h), dim3(1), dim3(serial_wide(h) ? psmf::SERIAL_WIDE_NT : psmf::serial_threads(h->geo.rpad)), 0, h->stream, h->sp, first);
}

// one filter step on the stream (captured into the graph or launched eagerly)
int enqueue_weighted_gram(psmf_filter* h);

int enqueue_serial_mgram(psmf_filter* h, int first);

int enqueue_step(psmf_filter* h) {
  // non-uniform diagonal R: this step's weighted Gram, before the sweep rewrites C.  On a masked handle it is the masked weighted
  // Gram of step k (mask row st->k, s_k from the serial stage of step k - 1): the sweep's block 0 solves with it, and the serial
  // stage of step k then runs beside the UNWEIGHTED masked Gram of step k + 1 as on every masked handle
  if (h->sp.rho_rows && h->cfg.coef_update) {
    const int rc = enqueue_weighted_gram(h);
    if (rc) return rc;
  }
  launch_sweep(h);
  if (h->use_coll) {
    if (!h->sp.tail_reduce) hipLaunchKernelGGL(psmf::psmf_reduce_partials, dim3(1), dim3(psmf::WG), 0, h->stream, h->sp);
    const int rc = all_reduce_sum(h, h->st->red, h->geo.ps, h->stream);
    if (rc) return rc;
  }
  if (h->cfg.masked) return enqueue_serial_mgram(h, 0);      // serial stage of this step beside the masked Gram of the next (psmf_masked.hip)
  launch_serial(h, 0);
  return PSMF_OK;
}

}  // namespace

// Can the handle's next run go through the persistent per-step kernel?  (one rank, uniform diagonal R, random walk or cos-phase
// dynamics, r <= 32, rows that fit the row workgroups' registers, unmasked or the masked PSMF / rPSMF filter; everything else keeps
// the two -- masked: three -- launches per timestep)
bool pstep_usable(const psmf_filter* h) {
  return h->engine == 1 && h->ps_ok && h->sw.step_persistent && !h->use_coll && !h->host_fn && !h->sp.rho_rows &&
         (h->cfg.masked == 0 || (h->cfg.masked == 1 && h->have_mask)) &&        // masked PSMF / rPSMF; MLE-SMF and TMF keep the two launches
         !h->cfg.nonuniform_R && h->cfg.dyn_kind <= PSMF_DYN_COS_PHASE && !h->sp.solve_lds && !h->sp.q_mat;
}

namespace {

int enqueue_gram_into(psmf_filter* h, double* Gout, const DevState* wst, const double* rho_rows) {
  const int r = h->cfg.r;
  const int rows = (h->cfg.d_local + kGramWG - 1) / kGramWG;
  by_storage(h, [&](auto t) {
    hipLaunchKernelGGL(psmf::psmf_gram_partial<decltype(t)>, dim3(kGramWG), dim3(psmf::WG), 0, h->stream,
                       h->C.as<const decltype(t)>(), h->cfg.d_local, r, h->geo.rp, rows, h->gpart, wst, rho_rows);
  });
  hipLaunchKernelGGL(psmf::psmf_gram_reduce, dim3((r * r + 255) / 256), dim3(256), 0, h->stream,
                     (const double*)h->gpart, kGramWG, r * r, Gout);
  if (h->use_coll) { const int rc = all_reduce_sum(h, Gout, (size_t)r * r, h->stream); if (rc) return rc; }
  return PSMF_OK;
}
constexpr int kMGramWG = 256;      // workgroups of the masked Gram (one partial each)

// psmf_serial_mgram: block 0 = the serial stage, blocks 1 .. kMGramWG = the masked Gram of the next step (psmf_masked.hip)
typedef LdsKernel<void (*)(StepParams, int, double*)> serial_mgram_t;
template <int RPAD, typename T, int NT, int NW>
serial_mgram_t serial_mgram_inst() { return {psmf::psmf_serial_mgram<RPAD, T, NT, NW>, NW * 64, (size_t)psmf::mgram_lds_doubles(NT, NW) * sizeof(double)}; }

template <typename T>
serial_mgram_t serial_mgram_for(int rpad, int r) {
  if (rpad == 8) return serial_mgram_inst<8, T, 1, 16>();
  if (rpad == 16) return serial_mgram_inst<16, T, 1, 16>();
  if (rpad == 32) return serial_mgram_inst<32, T, 2, 8>();
  return r <= 48 ? serial_mgram_inst<64, T, 3, 4>() : serial_mgram_inst<64, T, 4, 4>();
}
serial_mgram_t serial_mgram_kernel(const psmf_filter* h) { return by_storage(h, [&](auto t) { return serial_mgram_for<decltype(t)>(h->geo.rpad, h->cfg.r); }); }

// serial stage of the step + masked Gram of the next, then the Gram's fixed-order reduction (and its all-reduce over the shards)
int enqueue_serial_mgram(psmf_filter* h, int first) {
  const serial_mgram_t k = serial_mgram_kernel(h);
  hipLaunchKernelGGL(k.fn, dim3(1 + kMGramWG), dim3(k.threads), k.lds, h->stream, h->sp, first, h->gpart);
  const int ne = h->cfg.r * h->cfg.r + 1;
  // the shares of <G_m, Pbar> for the next sweep's eta: by the reduction itself, or -- row shards -- behind the all-reduce of the Gram
  const int ntr = (ne + 63) / 64;
  double* tpart = h->mg + ne + 1;
  hipLaunchKernelGGL(psmf::psmf_mgram_reduce, dim3(ntr), dim3(512), 0, h->stream, (const double*)h->gpart, (int)kMGramWG, ne, h->mg,
                     h->use_coll ? (const double*)nullptr : (const double*)h->st->Pbar, h->cfg.r, tpart);
  if (h->use_coll) {
    const int rc2 = all_reduce_sum(h, h->mg, (size_t)ne, h->stream);
    if (rc2) return rc2;
    hipLaunchKernelGGL(psmf::psmf_mgram_trace, dim3(ntr), dim3(64), 0, h->stream, (const double*)h->mg, (const double*)h->st->Pbar, h->cfg.r, tpart);
  }
  return PSMF_OK;
}

int enqueue_gram(psmf_filter* h) { return enqueue_gram_into(h, h->st->G, nullptr, nullptr); }

// the weighted Gram of the current step (non-uniform diagonal R) on the matrix cores: psmf_wgram_mfma -- on a masked handle
// psmf_mwgram_mfma, the masked weighted Gram -- + the masked Gram's reduction
typedef LdsKernel<void (*)(StepParams, double*)> wgram_t;
template <typename T, int NT>
wgram_t wgram_inst(bool masked) {
  return {masked ? psmf::psmf_mwgram_mfma<T, NT, 8> : psmf::psmf_wgram_mfma<T, NT, 8>, 8 * 64, (size_t)psmf::mgram_lds_doubles(NT, 8) * sizeof(double)};
}

template <typename T>
wgram_t wgram_for(int rpad, int r, bool masked) {
  if (rpad <= 16) return wgram_inst<T, 1>(masked);
  if (rpad == 32) return wgram_inst<T, 2>(masked);
  return r <= 48 ? wgram_inst<T, 3>(masked) : wgram_inst<T, 4>(masked);
}
wgram_t wgram_kernel(const psmf_filter* h) { return by_storage(h, [&](auto t) { return wgram_for<decltype(t)>(h->geo.rpad, h->cfg.r, h->cfg.masked != 0); }); }

int enqueue_weighted_gram(psmf_filter* h) {
  // PSMF_WGRAM_MFMA=0: the vector-unit Gram (it knows no mask: psmf_create refuses the switch on a masked handle)
  if (!h->sw.wgram_mfma) return enqueue_gram_into(h, h->st->GR, h->st, h->sp.rho_rows);
  const int r = h->cfg.r;
  const wgram_t k = wgram_kernel(h);
  hipLaunchKernelGGL(k.fn, dim3(kMGramWG), dim3(k.threads), k.lds, h->stream, h->sp, h->gpart);
  hipLaunchKernelGGL(psmf::psmf_mgram_reduce, dim3((r * r + 63) / 64), dim3(512), 0, h->stream, (const double*)h->gpart, (int)kMGramWG, r * r,
                     h->st->GR, (const double*)nullptr, r, (double*)nullptr);
  if (h->use_coll) { const int rc2 = all_reduce_sum(h, h->st->GR, (size_t)r * r, h->stream); if (rc2) return rc2; }
  return PSMF_OK;
}

int build_graph(psmf_filter* h, int chunk) {
  destroy_graph(h);
  HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  int rc = PSMF_OK;
  for (int i = 0; i < chunk && rc == PSMF_OK; ++i) rc = enqueue_step(h);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(h->stream, &g);
  if (rc != PSMF_OK) { if (g) hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) return fail(h, PSMF_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  h->graph = g;
  HIP_TRY(h, hipGraphInstantiate(&h->gexec, h->graph, nullptr, nullptr, 0));
  h->chunk = chunk;
  return PSMF_OK;
}

// O[M x N] = A[M x K] B[K x N] on the handle's stream (psmf_rotate.hip); the caller synchronises
template <typename TA, typename TB, typename TO>
int rot_gemm(psmf_filter* h, const TA* A, long long a_i, long long a_k, const TB* B, long long b_k, long long b_j, TO* O, long long o_i,
             long long M, long long N, long long K) {
  if (M <= 0 || N <= 0 || K <= 0) return PSMF_OK;
  if (!A || !B || !O || (M + psmf::ROT_T - 1) / psmf::ROT_T > 65535) return fail(h, PSMF_ERR_ARG, "rotation: bad operand");
  dim3 grid((unsigned)((N + psmf::ROT_T - 1) / psmf::ROT_T), (unsigned)((M + psmf::ROT_T - 1) / psmf::ROT_T));
  hipLaunchKernelGGL((psmf::psmf_rot_gemm<TA, TB, TO>), grid, dim3(256), 0, h->stream, A, a_i, a_k, B, b_k, b_j, O, o_i, (int)M, (int)N, (int)K);
  HIP_TRY(h, hipGetLastError());
  return PSMF_OK;
}

// the dictionary (d x rp, storage type): dst = U^T src (fwd) or U src (back)
int rot_dict(psmf_filter* h, const void* src, void* dst, bool fwd) {
  const long long d = h->cfg.d_local, rp = h->geo.rp, r = h->cfg.r;
  const long long ai = fwd ? 1 : d, ak = fwd ? d : 1;
  return by_storage(h, [&](auto t) { return rot_gemm(h, (const double*)h->rotU, ai, ak, (const decltype(t)*)src, rp, 1LL, (decltype(t)*)dst, rp, d, r, d); });
}

}  // namespace

// what the series unit (psmf_series.hip) calls besides run_steps: the captured graph holds buffer addresses, the scratch and
// rotation buffers belong to the handle, and the rotation kernel is launched here
void destroy_graph(psmf_filter* h) {
  if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
  if (h->graph) { hipGraphDestroy(h->graph); h->graph = nullptr; }
  h->chunk = 0;
}

int ensure_scratch(psmf_filter* h, size_t bytes) {
  ALLOC_TRY(h, h->scratch.reserve(bytes));
  return PSMF_OK;
}

int ensure_rot_tmp(psmf_filter* h, size_t bytes) {
  ALLOC_TRY(h, h->rot_tmp.reserve(bytes));
  return PSMF_OK;
}

// rows of X (n x d, storage type, row stride d) times U (fwd: into rotated coordinates) or U^T (back), out of place: src -> dst
int rot_rows(psmf_filter* h, const void* src, void* dst, long long n, bool fwd) {
  const long long d = h->cfg.d_local;
  const long long bk = fwd ? d : 1, bj = fwd ? 1 : d;
  return by_storage(h, [&](auto t) { return rot_gemm(h, (const decltype(t)*)src, d, 1LL, (const double*)h->rotU, bk, bj, (decltype(t)*)dst, d, n, d, d); });
}

namespace {

void compute_geometry(const psmf_config& c, Geometry& g, const int sweep_nt = 512) {
  g.vec = c.storage == PSMF_F64 ? 2 : 4;
  g.nv = (c.r + g.vec - 1) / g.vec;
  g.rp = g.nv * g.vec;
  g.gs = next_pow2(g.nv);
  g.nt = c.r > 32 ? 256 : sweep_nt;      // r > 32: the solve block (3 x 3 / 4 x 4 tiles of 16 x 16 in ONE wave's registers) needs a 256-thread kernel's register budget
  g.rpp = g.nt / g.gs;
  g.rpad = next_pow2(c.r < 8 ? 8 : c.r);
  const size_t solve_lds = c.coef_update ? (size_t)(4 * psmf::RM + 2) * 8 : 0;
  const size_t red_lds = (size_t)(g.nt / 64) * (g.gs * g.vec + 1) * 8;
  g.sweep_lds = ((solve_lds > red_lds ? solve_lds : red_lds) + 15) & ~(size_t)15;
  // (r > 32: one 256-thread workgroup per CU -- one wave per SIMD, see sweep_unroll -- so ONE round of workgroups, a few CUs left to the solve block)
  int target = c.n_workgroups > 0 ? c.n_workgroups : (c.r > 32 ? 248 : (g.nt == 512 ? 256 : 512));
  int rows = (c.d_local + target - 1) / target;
  rows = ((rows + g.rpp - 1) / g.rpp) * g.rpp;
  if (rows < g.rpp) rows = g.rpp;
  g.rows_per_wg = rows;
  g.n_sweep_wg = (c.d_local + rows - 1) / rows;
  g.ps = c.nonuniform_R ? 2 * (c.r + 1) : c.r + 1;      // partial row: h, ee (+ the weighted b, q)
}

// StepParams.solve_dual: can the per-step solve block run its two inversions side by side?  (random walk, Q = q I as last uploaded,
// full filter, uniform R, wave-local solve, no Q_k schedule: q of the next step is q -- or omega q -- of this one)
void update_solve_dual(psmf_filter* h) {
  const psmf_config& c = h->cfg;
  // Lbar' = (I / q - W / q^2) / omega loses log10((p + q) / q) digits to cancellation (p: the scale of P): with float64 storage, whose
  // results are otherwise good to 1e-11, the side-by-side form is left where that is more than five (q = 1e-8 against P0 = I: 3e-8
  // measured, 3e-11 with the inversions one after the other -- tools/probe_step_tinyq.py); float32 storage has its 1e-7 anyway
  const bool cancels = c.storage == PSMF_F64 && h->q_last > 0.0 && h->p_diag_max > 1e5 * h->q_last;
  const int v = (h->sw.step_dual && h->engine == 1 && h->q_iso && c.masked < 2 && c.dyn_kind == PSMF_DYN_RANDOM_WALK && c.coef_update && c.pbar_predict && !c.nonuniform_R &&
                 !h->sp.solve_lds && !h->sp.q_sched && !h->sp.q_mat && !cancels) ? 1 : 0;
  if (v != h->sp.solve_dual) {
    h->sp.solve_dual = v;
    destroy_graph(h);        // the captured launches carry the old parameter block
  }
}

// Persistent kernels spin on device flags: two of them resident at once (two handles of one process on one device) could each
// hold compute units the other needs.  They are serialised per device with an event chain.
std::mutex g_ps_mutex;
hipEvent_t g_ps_event[64] = {};      // raw on purpose, never destroyed: an owning static would call into a runtime that is already torn down at exit

int launch_pstep(psmf_filter* h, int64_t k_begin, int64_t n) {
  while (n > 0) {
    const int64_t chunk = n > (int64_t)1 << 30 ? (int64_t)1 << 30 : n;
    psmf::PstepParams q;
    memset(&q, 0, sizeof(q));
    q.sp = h->sp;
    q.k_begin = k_begin;
    q.n_steps = (int)chunk;
    q.n_row_wg = h->ps_plan.n_row_wg;
    q.rows_per_wg = h->ps_plan.rows_per_wg;
    q.np = h->ps_plan.np;
    q.ncol2 = h->ps_plan.ncol2;
    q.flags = h->ps_comm.as<unsigned>();
    q.pkt = reinterpret_cast<unsigned long long*>(h->ps_comm.as<char>() + h->ps_plan.off_pkt);
    q.part = reinterpret_cast<double*>(h->ps_comm.as<char>() + h->ps_plan.off_part);
    if (h->cfg.masked) {
      char* base = h->ps_comm.as<char>();
      q.masked = 1;
      q.nge = h->ps_plan.nge;
      q.slice_len = h->ps_plan.slice_len;
      q.gflags = reinterpret_cast<unsigned*>(base + h->ps_plan.off_gflags);
      q.sflags = reinterpret_cast<unsigned*>(base + h->ps_plan.off_sflags);
      q.gpart = reinterpret_cast<double*>(base + h->ps_plan.off_gpart);
      q.gslice = reinterpret_cast<double*>(base + h->ps_plan.off_gslice);
      q.mg_out = h->mg;
      q.mg_ntr = h->sp.mg_ntr;
    }
    q.prof = h->ps_prof;
    h->ps_prof_steps = chunk;
    std::lock_guard<std::mutex> lock(g_ps_mutex);
    const int dev = h->cfg.device & 63;
    if (!g_ps_event[dev]) HIP_TRY(h, hipEventCreateWithFlags(&g_ps_event[dev], hipEventDisableTiming));
    else HIP_TRY(h, hipStreamWaitEvent(h->stream, g_ps_event[dev], 0));
    HIP_TRY(h, hipMemsetAsync(h->ps_comm, 0, h->ps_plan.zero_bytes, h->stream));      // every polled word, before every launch
    HIP_TRY(h, psmf::pstep_launch(q, h->cfg.storage == PSMF_F64, h->stream));
    HIP_TRY(h, hipEventRecord(g_ps_event[dev], h->stream));
    ++h->ps_launches;
    k_begin += chunk;
    n -= chunk;
  }
  return PSMF_OK;
}

// Give-up policy of filter3's Newton-Schulz starts (docs/MEASUREMENTS.md round 5).  A start whose residual exceeds
// `far` is abandoned for the pivot-exact LDS sweep (15 us) and the next `skip` steps sweep unasked.  Where Lbar' = (I / q - W / q^2) / omega
// cancels -- eigenvalues of Pbar far above q: the adversarial Q = 1e-8 -- every early step that iterates instead of sweeping costs
// accuracy, so the conservative 0.3 / 3 stays; everywhere else (max diag P / q <= 1e3: at most three digits cancel) 0.9 / 1 takes
// config E's cold pass from 36.5 to 35.5 ms with unchanged errors (full-size and adversarial suites under it: profiles/r5_ns_far_policy.txt).
// PSMF_NS_FAR / PSMF_NS_SKIP override both.
void update_ns_policy(psmf_filter* h) {
  const bool benign = h->q_iso && h->q_last > 0.0 && h->p_diag_max <= 1e3 * h->q_last;
  if (!h->sw.ns_far_set) { const double f = benign ? 0.9 : 0.3; h->sp.ns_far2 = f * f; }
  if (!h->sw.ns_skip_set) h->sp.ns_skip_n = benign ? 1 : 3;
}

template <typename T>
void pack_rows(const double* src, T* dst, int d_local, int r, int rp) {
  for (int i = 0; i < d_local; ++i) {
    for (int c = 0; c < r; ++c) dst[(size_t)i * rp + c] = (T)src[(size_t)i * r + c];
    for (int c = r; c < rp; ++c) dst[(size_t)i * rp + c] = (T)0;
  }
}

// start-of-run preparation: step counter, exact Gram, then everything the first sweep needs
int prepare(psmf_filter* h, int64_t k_begin) {
  // step counter and error flag by a one-thread kernel (its arguments travel with the launch): no host buffer to keep
  // alive, so no synchronisation here -- consecutive passes over the series queue up back to back
  hipLaunchKernelGGL(psmf::psmf_prepare_k, dim3(1), dim3(1), 0, h->stream, h->st, (long long)k_begin);
  if (h->flags) clear_block_abort_flag(h);
  if (h->sp.mu_hist)   // (the handle's buffer, or the slot's share of it on a ring handle)
    HIP_TRY(h, hipMemcpyAsync(h->sp.mu_hist + (size_t)(k_begin - h->sp.series_t0) * h->cfg.r, h->st->mu, h->cfg.r * sizeof(double),
                              hipMemcpyDeviceToDevice, h->stream));
  if (h->engine == 2) {   // the blocked engine derives everything it needs from the block Gram
    h->need_prep = false;
    h->k_done = k_begin;
    return PSMF_OK;
  }
  if (h->sp.track_g) {
    int rc = enqueue_gram(h);
    if (rc != PSMF_OK) return rc;
  }
  if (h->cfg.masked) {      // + the masked Gram of the run's first step (psmf_prepare_k set kq = k_begin)
    const int rc = enqueue_serial_mgram(h, 1);
    if (rc) return rc;
  } else {
    launch_serial(h, 1);
  }
  HIP_TRY(h, hipGetLastError());
  h->need_prep = false;
  h->k_done = k_begin;
  return PSMF_OK;
}

// f(theta, x, t) on the host, for the predict roll-out (psmf.py:182-188); same term structure as psmf_dyn.hip
void dyn_f_host(const psmf_config& c, const double* th, const double* x, double t, double* out) {
  const int r = c.r, kind = c.dyn_kind, flags = c.dyn_flags, N = c.dyn_terms;
  if (kind == PSMF_DYN_RANDOM_WALK) { for (int i = 0; i < r; ++i) out[i] = x[i]; return; }
  if (kind == PSMF_DYN_SCALED_WALK) {
    for (int i = 0; i < r; ++i) {
      double a = (flags & 1) ? th[r * r + i] : 0.0;
      for (int j = 0; j < r; ++j) a += th[i * r + j] * x[j];
      out[i] = a;
    }
    return;
  }
  for (int i = 0; i < r; ++i) out[i] = 0.0;
  std::vector<double> val(r);
  const int nt = psmf::dyn_n_terms(kind, N);
  for (int tI = 0; tI < nt; ++tI) {
    const psmf::DynTerm d = psmf::dyn_term(kind, flags, N, r, tI);
    for (int j = 0; j < r; ++j) {
      const double arg = 2.0 * M_PI * th[d.b_off + j] * t + (d.c_off >= 0 ? th[d.c_off + j] : 1.0) * x[j];
      val[j] = d.is_cos ? cos(arg) : sin(arg);
    }
    for (int i = 0; i < r; ++i) {
      if (d.m_off >= 0) { double a = 0.0; for (int j = 0; j < r; ++j) a += th[d.m_off + i * r + j] * val[j]; out[i] += a; }
      else out[i] += val[i];
    }
  }
}

// psmf_create in stages, in the order it calls them.  The argument checks: the message of the first one that fails, or null
const char* check_config(const psmf_config* cfg) {
  if (cfg->abi_version != PSMF_ABI_VERSION) return "psmf_create: ABI version mismatch";
  if (cfg->r < 1 || cfg->r > PSMF_RMAX) return "psmf_create: need 1 <= r <= 64";
  if (cfg->d < 1 || cfg->d_local < 1 || cfg->row0 < 0 || cfg->row0 + cfg->d_local > cfg->d) return "psmf_create: bad d / row0 / d_local";
  if (cfg->storage != PSMF_F32 && cfg->storage != PSMF_F64) return "psmf_create: storage must be f32 or f64";
  if (cfg->dyn_kind < PSMF_DYN_RANDOM_WALK || cfg->dyn_kind > PSMF_DYN_HOST) return "psmf_create: unknown dyn_kind";
  if (cfg->dyn_kind == PSMF_DYN_FOURIER && (cfg->dyn_terms < 1 || 2 * cfg->dyn_terms > psmf::DYN_MAX_TERMS)) return "psmf_create: Fourier dynamics need 1 <= dyn_terms <= 4";
  if (cfg->n_theta != psmf::dyn_n_theta(cfg->dyn_kind, cfg->dyn_flags, cfg->dyn_terms, cfg->r)) return "psmf_create: n_theta does not match dyn_kind / dyn_flags / dyn_terms (see psmf_dyn_kind)";
  if (cfg->dyn_kind == PSMF_DYN_HOST && cfg->recursive) return "psmf_create: host-stepped dynamics keep theta (and its optimiser) on the host";
  if (cfg->recursive && cfg->update_every < 1) return "psmf_create: update_every must be >= 1";
  if (cfg->recursive < 0 || cfg->recursive > 2) return "psmf_create: recursive must be 0, 1 (in-loop Adam) or 2 (in-loop SGD)";
  if (cfg->masked < 0 || cfg->masked > PSMF_MASKED_DYNAMICS) return "psmf_create: masked must be 0 .. 4";
  if ((cfg->masked == 2 || cfg->masked == 3) && (cfg->robust || cfg->dyn_kind != PSMF_DYN_RANDOM_WALK))
    return "psmf_create: masked = 2 (MLE-SMF) / 3 (TMF) are random-walk, non-robust filters";
  if (cfg->masked) {
    // masked = 1 is the ExperimentImpute filter, a random walk by definition; masked = 4 (PSMF_MASKED_DYNAMICS) is the same step with
    // every device-evaluated f_theta (cos-phase, scaled walk, sinusoid, Fourier basis), theta learned between epochs or in the loop:
    // the gradient is that of the masked incremental likelihood (serial_body, psmf_kernels.hip)
    if (cfg->masked == 1 && cfg->dyn_kind != PSMF_DYN_RANDOM_WALK)
      return "psmf_create: masked = 1 handles are random-walk filters (ExperimentImpute/PSMF.py:65-66: Pbar = P + Q); masked = 4 runs f_theta";
    if (cfg->dyn_kind == PSMF_DYN_HOST)
      return "psmf_create: masked handles evaluate f_theta on the device: not with PSMF_DYN_HOST (the host would need the masked gradient g_f)";
    if (cfg->nonuniform_R && cfg->n_theta > 0)
      return "psmf_create: masked handles with nonuniform_R = 1 do not learn theta (the Gram's count slot carries sum m_i rho_i, not n_obs): n_theta must be 0";
    if (!cfg->coef_update || !cfg->eta_full || !cfg->pbar_predict || cfg->engine == 2 || !cfg->store_y_pred)
      return "psmf_create: masked handles need the full filter (coef_update, eta_full, pbar_predict), store_y_pred = 1 and the per-step engine";
    if (cfg->masked == 3 && cfg->nonuniform_R) return "psmf_create: masked = 3 (TMF) ignores R (TMF.py:47-66): not with nonuniform_R = 1";
  }
  return nullptr;
}

int choose_engine(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  const bool can_block = cfg->r <= psmf::RM / 2 && cfg->dyn_kind != PSMF_DYN_HOST && !cfg->nonuniform_R && !cfg->masked;
  if (cfg->engine == 2 && !can_block) return fail(h, PSMF_ERR_ARG, "psmf_create: the blocked engine needs r <= 32, device-evaluated dynamics and a uniform diagonal R");
  if (cfg->engine < 0 || cfg->engine > 2) return fail(h, PSMF_ERR_ARG, "psmf_create: engine must be 0 (auto), 1 (per-step) or 2 (blocked)");
  // auto: blocked whenever it applies -- it is exact and removes the per-step launches and row sweeps
  h->engine = cfg->engine == 0 ? (can_block ? 2 : 1) : cfg->engine;
  { const int v = h->sw.engine_env; if (v == 1 || (v == 2 && can_block)) h->engine = v; }
  // (scaled-walk / sinusoid / Fourier dynamics on the per-step engine -- r > 32, a non-uniform R, engine = 1: the launched form's
  //  serial stage evaluates them through psmf_dyn.hip like the blocked engine's general kernel)
  return PSMF_OK;
}

// the device, the handle's stream and events, and the buffers of every engine
int alloc_common(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  HIP_TRY(h, hipSetDevice(cfg->device));
  HIP_TRY(h, hipStreamCreateWithFlags(h->stream.put(), hipStreamNonBlocking));
  HIP_TRY(h, hipEventCreate(h->ev0.put()));
  HIP_TRY(h, hipEventCreate(h->ev1.put()));
  HIP_TRY(h, hipHostMalloc(h->err_host.put(), sizeof(int), hipHostMallocMapped));
  HIP_TRY(h, hipHostGetDevicePointer((void**)&h->err_host_dev, h->err_host.get(), 0));
  ALLOC_TRY(h, h->st.alloc(sizeof(DevState)));
  HIP_TRY(h, hipMemset(h->st, 0, sizeof(DevState)));
  ALLOC_TRY(h, h->C.alloc((size_t)cfg->d_local * h->geo.rp * h->elem()));
  ALLOC_TRY(h, h->partials.alloc((size_t)h->geo.n_sweep_wg * h->geo.ps * sizeof(double)));
  ALLOC_TRY(h, h->gpart.alloc((size_t)((cfg->masked || cfg->nonuniform_R) ? 256 : kGramWG) * (cfg->r * cfg->r + 1) * sizeof(double)));
  if (cfg->masked) ALLOC_TRY(h, h->mg.alloc((size_t)(cfg->r * cfg->r + 2 + (cfg->r * cfg->r + 64) / 64 + 1) * sizeof(double)));     // Gram, count | trace shares
  h->th_cap = (size_t)(cfg->n_theta > psmf::RM ? cfg->n_theta : psmf::RM);
  ALLOC_TRY(h, h->thbuf.alloc(4 * h->th_cap * sizeof(double)));
  HIP_TRY(h, hipMemset(h->thbuf, 0, 4 * h->th_cap * sizeof(double)));
  return PSMF_OK;
}

// persistent per-step engine (psmf_pstep.hip): the plan of a launch and its communication block, where the kernel applies
int init_pstep(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  if (h->engine == 1 && h->sw.step_persistent && (cfg->r <= 32 || (h->sw.pstep_big && cfg->r <= 48 && cfg->masked == 0)) && cfg->masked <= 1 && !cfg->nonuniform_R &&
      cfg->dyn_kind <= PSMF_DYN_COS_PHASE) {
    hipDeviceProp_t prop;
    HIP_TRY(h, hipGetDeviceProperties(&prop, cfg->device));
    if (psmf::pstep_plan(cfg->d_local, cfg->r, prop.multiProcessorCount, cfg->storage == PSMF_F64, cfg->masked == 1, &h->ps_plan)) {
      HIP_TRY(h, psmf::pstep_init());
      ALLOC_TRY(h, h->ps_comm.alloc(h->ps_plan.total_bytes));
      HIP_TRY(h, hipMemset(h->ps_comm, 0, h->ps_plan.total_bytes));
      if (h->sw.pstep_prof) { ALLOC_TRY(h, h->ps_prof.alloc(64 * sizeof(long long))); HIP_TRY(h, hipMemset(h->ps_prof, 0, 64 * sizeof(long long))); }
      h->ps_ok = true;
    }
  }
  return PSMF_OK;
}

void fill_step_params(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  StepParams& sp = h->sp;
  memset(&sp, 0, sizeof(sp));
  sp.st = h->st;
  sp.C = h->C;
  sp.partials = h->partials;
  sp.d = cfg->d; sp.d_local = cfg->d_local; sp.r = cfg->r; sp.rp = h->geo.rp; sp.nv = h->geo.nv;
  sp.n_sweep_wg = h->geo.n_sweep_wg; sp.rows_per_wg = h->geo.rows_per_wg; sp.ps = h->geo.ps;
  sp.robust = cfg->robust; sp.coef_update = cfg->coef_update; sp.eta_full = cfg->eta_full;
  sp.pbar_predict = cfg->pbar_predict; sp.fixed_lambda = cfg->fixed_lambda;
  sp.dyn_kind = cfg->dyn_kind; sp.n_theta = cfg->n_theta; sp.store_yp = 0;
  sp.dyn_flags = cfg->dyn_flags; sp.dyn_terms = cfg->dyn_terms;
  sp.theta = h->thbuf; sp.gradsum = h->thbuf + h->th_cap; sp.adam_m = h->thbuf + 2 * h->th_cap; sp.adam_v = h->thbuf + 3 * h->th_cap;
  sp.rho_sched = nullptr; sp.q_sched = nullptr; sp.q_mat = nullptr;
  sp.rho_rows = nullptr; sp.rho_mean = 1.0;
  sp.recursive = cfg->recursive; sp.update_every = cfg->update_every > 0 ? cfg->update_every : 1;
  sp.track_g = ((cfg->eta_full || cfg->coef_update) && !cfg->masked) ? 1 : 0;     // masked: G is this step's masked Gram, recomputed every step
  sp.mask = nullptr; sp.mg = nullptr; sp.mg_tr = nullptr; sp.mg_ntr = 0; sp.sc_hist = nullptr; sp.mask_rows = 0;
  sp.masked_method = cfg->masked >= 2 ? cfg->masked : 0;
  sp.solve_lds = (!h->sw.wave_solve || (cfg->r > 32 && !h->sw.wave_big)) ? 1 : 0;
  {
    // The last row workgroup of a sweep sums the partial rows (tail_reduce_partials) where the solve block outlasts the row blocks
    // by more than that tail -- r > 32 at moderate d_local, small shards: 31.6 -> 30.0 us per timestep at r = 40, d = 2e4, 50.3 ->
    // 47.4 at r = 64 -- and the serial stage does where the rows are the longer part (d = 1e5, r = 32: 19.5 against 21.2 with the
    // tail; tools/probe_tail.py).  PSMF_TAIL_REDUCE=1 / 0 forces it on / off.
    const double rows_us = 2.0 * (double)cfg->d_local * h->geo.rp * (double)h->elem() / 3.0e6;
    const double solve_us = cfg->r <= 32 ? 0.3 * cfg->r : (cfg->r <= 48 ? 13.0 : 24.0);
    sp.tail_reduce = (h->engine == 1 && h->sw.tail_reduce != 0 && (h->sw.tail_reduce == 1 || (cfg->coef_update && rows_us + 3.0 < solve_us))) ? 1 : 0;
  }
  sp.external_reduce = sp.tail_reduce;
  sp.use_ns = h->sw.ns ? 1 : 0;
  sp.ns_predict = h->sw.ns_predict;
  // Newton-Schulz acceptance: ||I - M X||_F below the tolerance BEFORE the last update (which squares it).  float64
  // storage: 3e-7 (-> 1e-13).  float32 storage: 3e-4 (-> ~1e-7, of the order of the rounding of C and y to float32; errors
  // against the float64 oracle measured at 1e-4 / 3e-4 / 1e-3 in DESIGN section 5: unchanged up to 3e-4).  PSMF_NS_TOL overrides.
  const double ns_tol = h->sw.ns_tol_set ? h->sw.ns_tol : (cfg->storage == PSMF_F64 ? 3e-7 : 3e-4);
  sp.ns_tol2 = ns_tol * ns_tol;
  // A start with ||I - M X0||_F >= 0.3 is given up for the direct sweep, and the next three steps sweep unasked (PSMF_NS_FAR,
  // PSMF_NS_SKIP).  Below 1 the iteration would converge -- from 0.9 in seven iterations of 0.9 us against a 15 us sweep -- and
  // 0.9 / 0 takes config E's cold pass from 36.4 to 35.5 ms (111 -> 10 sweeps in its first 480 timesteps, tools/probe_cold.py);
  // NOT taken: the iteration stops at a residual (1e-7), the sweep is pivot-exact, and where Lbar' = (I / q - W / q^2) / omega
  // cancels (q = 1e-8, tests/adversarial_cases.py:tiny_Q) every early step iterated instead of swept costs accuracy -- y_hat error
  // 6.4e-7 (0.3 / 3), 4.0e-6 (0.3 / 0), 9.2e-6 (0.6 / 1), 1.26e-5 (0.6 / 0) against the 1e-5 bar (profiles/r4_adversarial_ns_far.txt).
  sp.ns_far2 = h->sw.ns_far * h->sw.ns_far;      // (unset: psmf_set_state picks 0.9 / 1 where nothing cancels, update_ns_policy)
  sp.ns_skip_n = h->sw.ns_skip;
  sp.alpha = cfg->alpha; sp.beta = cfg->beta;
  sp.lr = cfg->adam_lr; sp.lr_end = cfg->adam_lr_end; sp.lr_steps = cfg->adam_lr_steps;
  sp.b1 = cfg->adam_b1; sp.b2 = cfg->adam_b2;
}

// PSMF_PSTEP_PROF=1 with a -DPSTEP_PROF build: the per-phase clock sums of the last launch, at psmf_destroy
void print_pstep_prof(psmf_filter* h) {
  long long pf[64];
  if (!h->ps_prof || hipMemcpy(pf, h->ps_prof, sizeof(pf), hipMemcpyDeviceToHost) != hipSuccess || h->ps_prof_steps <= 0) return;
  fprintf(stderr, "[pstep prof] cycles per timestep over the last launch (%lld steps), d_local %d r %d:\n", h->ps_prof_steps, h->cfg.d_local, h->cfg.r);
  const char* grp[3] = {"hub workers", "solve wave ", "row wg 0   "};
  const int base[3] = {0, 16, 24}, cnt[3] = {11, 3, 8};
  for (int g = 0; g < 3; ++g) {
    fprintf(stderr, "  %s:", grp[g]);
    for (int i = 0; i < cnt[g]; ++i) fprintf(stderr, " %7.0f", (double)pf[base[g] + i] / (double)h->ps_prof_steps);
    fprintf(stderr, "\n");
  }
}

}  // namespace

extern "C" {

int psmf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* psmf_last_error(psmf_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int psmf_create(psmf_handle* out, const psmf_config* cfg_in) {
  if (!out || !cfg_in) return fail(nullptr, PSMF_ERR_ARG, "psmf_create: null argument");
  *out = nullptr;
  if (const char* msg = check_config(cfg_in)) return fail(nullptr, PSMF_ERR_ARG, msg);
  // masked = 4 is masked = 1 with f_theta allowed (check_config): one masked PSMF / rPSMF filter from here on
  psmf_config cfg_norm = *cfg_in;
  if (cfg_norm.masked == PSMF_MASKED_DYNAMICS) cfg_norm.masked = 1;
  const psmf_config* cfg = &cfg_norm;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, PSMF_ERR_NO_DEVICE, "psmf_create: no HIP device visible (the MI355X path has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, PSMF_ERR_ARG, "psmf_create: bad device ordinal");

  psmf_filter* h = new psmf_filter();
  h->cfg = *cfg;
  compute_geometry(h->cfg, h->geo, h->sw.sweep_threads);
  auto bail = [&](int code) { g_create_error = h->err; psmf_destroy(h); return code; };
  int rc = choose_engine(h);
  if (!rc && cfg->masked && cfg->nonuniform_R && !h->sw.wgram_mfma)
    rc = fail(h, PSMF_ERR_ARG, "psmf_create: PSMF_WGRAM_MFMA=0 selects the vector-unit weighted Gram, which has no masked form: "
                               "not on a masked handle with nonuniform_R = 1");
  if (!rc) rc = alloc_common(h);
  if (!rc && h->engine == 2) rc = init_blocked(h);
  // dynamic LDS beyond the default limit: opted in here, per handle and so on the handle's device, for the kernels it can launch
  if (!rc && h->geo.sweep_lds > 48 * 1024) rc = opt_in_lds(h, (const void*)sweep_kernel(h), h->geo.sweep_lds);
  if (!rc && cfg->masked) { const serial_mgram_t k = serial_mgram_kernel(h); rc = opt_in_lds(h, (const void*)k.fn, k.lds); }
  if (!rc && cfg->nonuniform_R) { const wgram_t k = wgram_kernel(h); rc = opt_in_lds(h, (const void*)k.fn, k.lds); }
  if (!rc) rc = init_pstep(h);
  if (rc) return bail(rc);
  fill_step_params(h);
  // the zero-fills above ran on the null stream; the handle's own streams are non-blocking
  if (hipDeviceSynchronize() != hipSuccess) { h->err = "hipDeviceSynchronize at the end of psmf_create failed"; return bail(PSMF_ERR_HIP); }
  *out = h;
  return PSMF_OK;
}

void psmf_destroy(psmf_handle h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  for (hipStream_t s : {h->stream.get(), h->bulk.get(), h->fstream.get(), h->cstream.get()})
    if (s) hipStreamSynchronize(s);
  print_pstep_prof(h);
  destroy_graph(h);
  if (h->comm) ncclCommDestroy(h->comm);
  delete h;      // every buffer, event and stream: the members release themselves
}

int psmf_set_state(psmf_handle h, const double* C, const double* V, const double* P, const double* Q,
                   const double* mu, double rho, double lambda0, const double* theta) {
  if (!h) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int r = h->cfg.r, dl = h->cfg.d_local, rp = h->geo.rp;
  if (C) {
    rc = by_storage(h, [&](auto t) {
      std::vector<decltype(t)> buf((size_t)dl * rp);
      pack_rows(C, buf.data(), dl, r, rp);
      HIP_TRY(h, hipMemcpy(h->C, buf.data(), buf.size() * sizeof(t), hipMemcpyHostToDevice));
      return (int)PSMF_OK;
    });
    if (rc) return rc;
    if (h->rotU) {                       // non-diagonal R: the handle keeps U^T C
      const size_t cb = (size_t)dl * rp * h->elem();
      rc = ensure_rot_tmp(h, cb);
      if (rc) return rc;
      HIP_TRY(h, hipMemcpyAsync(h->rot_tmp, h->C, cb, hipMemcpyDeviceToDevice, h->stream));     // (stream-ordered with the GEMM: a plain D2D hipMemcpy does not wait on the host side)
      rc = rot_dict(h, h->rot_tmp, h->C, true);
      if (rc) return rc;
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  }
  const size_t rr = (size_t)r * r * sizeof(double);
  if (V) HIP_TRY(h, hipMemcpy(h->st->V, V, rr, hipMemcpyHostToDevice));
  if (P) {
    HIP_TRY(h, hipMemcpy(h->st->P, P, rr, hipMemcpyHostToDevice));
    double m = 0.0;
    for (int i = 0; i < r; ++i) m = std::fmax(m, std::fabs(P[(size_t)i * r + i]));
    h->p_diag_max = m;
    if (!Q) update_solve_dual(h);
  }
  if (Q) {
    HIP_TRY(h, hipMemcpy(h->st->Q, Q, rr, hipMemcpyHostToDevice));
    bool iso = Q[0] > 0.0;
    for (int i = 0; i < r && iso; ++i)
      for (int c = 0; c < r; ++c)
        if (Q[i * r + c] != (i == c ? Q[0] : 0.0)) { iso = false; break; }
    h->q_iso = iso;
    h->q_last = Q[0];
    update_solve_dual(h);
  }
  if (mu) HIP_TRY(h, hipMemcpy(h->st->mu, mu, r * sizeof(double), hipMemcpyHostToDevice));
  if (theta && h->cfg.n_theta > 0)
    HIP_TRY(h, hipMemcpy(h->sp.theta, theta, h->cfg.n_theta * sizeof(double), hipMemcpyHostToDevice));
  if (!std::isnan(rho)) HIP_TRY(h, hipMemcpy(&h->st->rho, &rho, sizeof(double), hipMemcpyHostToDevice));
  if (!std::isnan(lambda0)) HIP_TRY(h, hipMemcpy(&h->st->lam, &lambda0, sizeof(double), hipMemcpyHostToDevice));
  { const int zero = 0; HIP_TRY(h, hipMemcpy(&h->st->ns_valid, &zero, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(&h->st->err, &zero, sizeof(int), hipMemcpyHostToDevice)); }   // a new state clears a sticky numeric error
  if (P || Q) update_ns_policy(h);
  if (C && V && P && mu) h->have_state = true;
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_zero_gradsum(psmf_handle h) {
  if (!h) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipMemsetAsync(h->sp.gradsum, 0, sizeof(double) * h->th_cap, h->stream));
  return PSMF_OK;
}

int psmf_set_adam(psmf_handle h, const double* m, const double* v) {
  if (!h) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const size_t nb = (size_t)h->cfg.n_theta * sizeof(double);
  if (m && nb) HIP_TRY(h, hipMemcpy(h->sp.adam_m, m, nb, hipMemcpyHostToDevice));
  if (v && nb) HIP_TRY(h, hipMemcpy(h->sp.adam_v, v, nb, hipMemcpyHostToDevice));
  return PSMF_OK;
}

int psmf_get_state(psmf_handle h, double* C, double* V, double* P, double* Q, double* mu, double* theta,
                   double* gradsum, double* scalars) {
  if (!h) return PSMF_ERR_ARG;
  int rc = psmf_sync(h);
  if (rc) return rc;
  const int r = h->cfg.r, dl = h->cfg.d_local, rp = h->geo.rp;
  if (C) {
    const void* Csrc = h->C;
    if (h->rotU) {                       // non-diagonal R: back to the caller's coordinates, C = U (U^T C)
      const size_t cb = (size_t)dl * rp * h->elem();
      rc = ensure_rot_tmp(h, cb);
      if (rc) return rc;
      HIP_TRY(h, hipMemsetAsync(h->rot_tmp, 0, cb, h->stream));
      rc = rot_dict(h, h->C, h->rot_tmp, false);
      if (rc) return rc;
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      Csrc = h->rot_tmp;
    }
    rc = by_storage(h, [&](auto t) {
      std::vector<decltype(t)> buf((size_t)dl * rp);
      HIP_TRY(h, hipMemcpy(buf.data(), Csrc, buf.size() * sizeof(t), hipMemcpyDeviceToHost));
      for (int i = 0; i < dl; ++i) for (int c = 0; c < r; ++c) C[(size_t)i * r + c] = (double)buf[(size_t)i * rp + c];
      return (int)PSMF_OK;
    });
    if (rc) return rc;
  }
  const size_t rr = (size_t)r * r * sizeof(double);
  if (V) HIP_TRY(h, hipMemcpy(V, h->st->V, rr, hipMemcpyDeviceToHost));
  if (P) HIP_TRY(h, hipMemcpy(P, h->st->P, rr, hipMemcpyDeviceToHost));
  if (Q) HIP_TRY(h, hipMemcpy(Q, h->st->Q, rr, hipMemcpyDeviceToHost));
  if (mu) HIP_TRY(h, hipMemcpy(mu, h->st->mu, r * sizeof(double), hipMemcpyDeviceToHost));
  if (theta && h->cfg.n_theta) HIP_TRY(h, hipMemcpy(theta, h->sp.theta, h->cfg.n_theta * sizeof(double), hipMemcpyDeviceToHost));
  if (gradsum && h->cfg.n_theta) HIP_TRY(h, hipMemcpy(gradsum, h->sp.gradsum, h->cfg.n_theta * sizeof(double), hipMemcpyDeviceToHost));
  if (scalars) {
    DevState* s = h->st;
    double tmp[12];  // rho lam s eta N kappa phi omega ee s_done eta_done N_done
    HIP_TRY(h, hipMemcpy(tmp, &s->rho, sizeof(double) * 12, hipMemcpyDeviceToHost));
    long long k;
    HIP_TRY(h, hipMemcpy(&k, &s->k, sizeof(k), hipMemcpyDeviceToHost));
    scalars[0] = tmp[0]; scalars[1] = tmp[1]; scalars[2] = tmp[9]; scalars[3] = tmp[10];
    scalars[4] = tmp[11]; scalars[5] = tmp[6]; scalars[6] = tmp[7]; scalars[7] = (double)k;
  }
  return PSMF_OK;
}

int psmf_run(psmf_handle h, int64_t k_begin, int64_t k_end) {
  if (!h) return PSMF_ERR_ARG;
  if (!h->have_state) return fail(h, PSMF_ERR_STATE, "psmf_run: set_state (C, V, P, mu) first");
  if (!h->Y) return fail(h, PSMF_ERR_STATE, "psmf_run: upload_series first");
  if (k_begin < 0 || k_end < k_begin || (!h->ring_slots && k_end > h->T_cap)) return fail(h, PSMF_ERR_ARG, "psmf_run: step range outside the uploaded series");
  if (h->cfg.dyn_kind == PSMF_DYN_HOST) return fail(h, PSMF_ERR_STATE, "psmf_run: host-stepped dynamics advance with psmf_step_host");
  if (h->sched && k_end >= h->sched_n) return fail(h, PSMF_ERR_ARG, "psmf_run: step range beyond the R / Q schedules");
  if (h->qmat && k_end >= h->qmat_n) return fail(h, PSMF_ERR_ARG, "psmf_run: step range beyond the Q_k matrix schedule");
  if (h->cfg.nonuniform_R && !h->sp.rho_rows) return fail(h, PSMF_ERR_STATE, "psmf_run: psmf_set_row_noise first (nonuniform_R = 1)");
  if (h->cfg.masked && !h->have_mask) return fail(h, PSMF_ERR_STATE, "psmf_run: psmf_upload_mask first (masked = 1)");
  // the mask buffer is not cleared when it is allocated: a step beyond the uploaded rows would filter with whatever the memory held
  if (h->cfg.masked && !h->ring_slots && k_end > h->mask_hi)
    return fail(h, PSMF_ERR_ARG, "psmf_run: step range beyond the uploaded mask (psmf_upload_mask covers the steps 1 .. " + std::to_string((long long)h->mask_hi) + ")");
  int rc = set_device(h);
  if (rc) return rc;
  return h->ring_slots ? ring_run(h, k_begin, k_end) : run_steps(h, k_begin, k_end);
}

}  // extern "C"

// the steps k_begin + 1 .. k_end of a checked psmf_run, all read at k - sp.series_t0 (a ring handle: one piece of it)
int run_steps(psmf_filter* h, int64_t k_begin, int64_t k_end) {
  int rc = PSMF_OK;
  if (h->need_prep || h->k_done != k_begin) {
    rc = prepare(h, k_begin);
    if (rc) return rc;
  }
  int64_t n = k_end - k_begin;
  if (h->engine == 2) {
    const bool pipe_off = !h->sw.block_pipe;
    if (!pipe_off && k_end - k_begin > h->block_steps) {
      rc = enqueue_blocks_pipelined(h, k_begin, k_end);
      if (rc) return rc;
      h->k_done = k_end;
      return PSMF_OK;
    }
    int64_t k = k_begin;
    while (k < k_end) {
      const int nb = (int)((k_end - k) < h->block_steps ? (k_end - k) : h->block_steps);
      rc = enqueue_block(h, k, nb);
      if (rc) return rc;
      k += nb;
    }
    HIP_TRY(h, hipGetLastError());
    h->k_done = k_end;
    return PSMF_OK;
  }
  const int64_t refresh = h->cfg.gram_refresh > 0 && h->sp.track_g ? h->cfg.gram_refresh : 0;
  while (n > 0) {
    int64_t seg = n;
    if (refresh) {
      const int64_t to_next = refresh - (h->k_done % refresh);
      if (to_next < seg) seg = to_next;
    }
    int64_t left = seg;
    if (pstep_usable(h)) {      // the whole segment in ONE launch: C on chip, hand-offs through device flags (psmf_pstep.hip)
      rc = launch_pstep(h, h->k_done, left);
      if (rc) return rc;
      left = 0;
    }
    if (h->cfg.use_graph && !h->host_fn) {   // (a host-mediated all-reduce cannot be captured)
      const int want = 256;
      if (left >= want && h->chunk != want) {
        rc = build_graph(h, want);
        if (rc) return rc;
      }
      while (h->chunk > 0 && left >= h->chunk) {
        HIP_TRY(h, hipGraphLaunch(h->gexec, h->stream));
        left -= h->chunk;
      }
    }
    for (; left > 0; --left) {
      rc = enqueue_step(h);
      if (rc) return rc;
    }
    HIP_TRY(h, hipGetLastError());
    h->k_done += seg;
    n -= seg;
    if (refresh && n > 0 && h->k_done % refresh == 0) {
      rc = enqueue_gram(h);
      if (rc) return rc;
      launch_serial(h, 1);   // recompute eta / N / kappa of the next step with the exact Gram
    }
  }
  return PSMF_OK;
}

extern "C" {

int psmf_sync(psmf_handle h) {
  if (!h) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  const double t_s0 = h->sw.host_timing ? host_now_ms() : 0.0;
  // (a 4-byte device-to-host hipMemcpy[Async] here now and then took 20-70 ms on this stack -- the copy engine waking
  //  up -- which is half a pass of the headline workload; a store from a kernel to mapped host memory does not)
  hipLaunchKernelGGL(psmf::psmf_publish_err_k, dim3(1), dim3(1), 0, h->stream, (const DevState*)h->st, h->err_host_dev);
  const double t_s1 = h->sw.host_timing ? host_now_ms() : 0.0;
  HIP_TRY(h, spin_stream(h->stream));
  for (int i = 0; i < h->evk_pending; ++i) {         // the chained filter launches that finished: their durations
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->evK0[i], h->evK1[i]) == hipSuccess) { h->kernel_ms_sum += ms; ++h->kernel_launches; }
    else (void)hipGetLastError();
  }
  h->evk_pending = 0;
  if (h->sw.host_timing) { const double t = host_now_ms(); if (t_s1 - t_s0 > 5.0) fprintf(stderr, "[psmf host timing] memcpyAsync call %.1f ms\n", t_s1 - t_s0); if (t - t_s1 > 5.0) fprintf(stderr, "[psmf host timing] spin wait %.1f ms\n", t - t_s1); }
  const int err = *h->err_host;
  if (err == -7) {
    long long fl[8] = {0};
    if (h->flags) (void)hipMemcpy(fl, h->flags, sizeof(fl), hipMemcpyDeviceToHost);
    char msg[320];
    snprintf(msg, sizeof(msg), "pipelined blocks: a device-flag hand-off timed out (PSMF_BLOCK_CHAIN=0: one filter launch per block; "
             "PSMF_BLOCK_FLAGS=0: event hand-off); flags: cross-Gram %lld, filter %lld, next block to enqueue %lld",
             fl[0], fl[1], h->seq_next);
    return fail(h, PSMF_ERR_HIP, msg);
  }
  if (err == -8) return fail(h, PSMF_ERR_HIP, "persistent per-step kernel: a hand-off between the hub and the row workgroups timed out "
                                               "(PSMF_STEP_PERSISTENT=0: two launches per timestep)");
  if (err != 0) {
    char msg[128];
    snprintf(msg, sizeof(msg), "singular r x r system (I + kappa Pbar G) at step %d", err);
    return fail(h, PSMF_ERR_NUMERIC, msg);
  }
  return PSMF_OK;
}

int psmf_run_timed(psmf_handle h, int64_t k_begin, int64_t k_end, float* ms) {
  if (!h || !ms) return PSMF_ERR_ARG;
  int rc = set_device(h);
  if (rc) return rc;
  if (h->have_state && h->Y && !h->ring_slots && (h->need_prep || h->k_done != k_begin)) {
    rc = prepare(h, k_begin);   // keep the one-off preparation outside the timed region
    if (rc) return rc;
  }
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  rc = psmf_run(h, k_begin, k_end);
  if (rc) return rc;
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, spin_event(h->ev1));
  HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
  return psmf_sync(h);
}

// psmf_time_kernel launches a step's kernels at the FIRST steps of the uploaded series whatever the handle has run so far: they
// overwrite the y_hat rows and the posterior means recorded for those steps, which the caller reads after a run
// (psmf_download_y_pred, psmf_sq_error, psmf_download_mu).  These records are saved and restored with the state.
struct StepRecords { Dev<void> yp; Dev<double> mu; };

static int save_step_records(psmf_filter* h, int64_t yp_rows, int64_t mu_rows, StepRecords& s) {
  if (yp_rows > h->T_cap) yp_rows = h->T_cap;
  if (mu_rows > h->T_cap + 1) mu_rows = h->T_cap + 1;
  if (h->YP && yp_rows > 0) {
    ALLOC_TRY(h, s.yp.alloc((size_t)yp_rows * h->cfg.d_local * h->elem()));
    HIP_TRY(h, hipMemcpy(s.yp, h->YP, s.yp.bytes(), hipMemcpyDeviceToDevice));
  }
  if (h->mu_hist && mu_rows > 0) {
    ALLOC_TRY(h, s.mu.alloc((size_t)mu_rows * h->cfg.r * sizeof(double)));
    HIP_TRY(h, hipMemcpy(s.mu, h->mu_hist, s.mu.bytes(), hipMemcpyDeviceToDevice));
  }
  return PSMF_OK;
}

static int restore_step_records(psmf_filter* h, const StepRecords& s) {
  if (s.yp) HIP_TRY(h, hipMemcpy(h->YP, s.yp, s.yp.bytes(), hipMemcpyDeviceToDevice));
  if (s.mu) HIP_TRY(h, hipMemcpy(h->mu_hist, s.mu, s.mu.bytes(), hipMemcpyDeviceToDevice));
  return PSMF_OK;
}

// Everything psmf_time_kernel's launches mutate: C, the DevState, theta with its gradient sums and Adam moments (the filter
// kernels and the serial stage step them too), and the step records above.  The copies are released with the object.
struct TimingSave {
  Dev<void> C; Dev<DevState> st; Dev<double> th;
  StepRecords rec;
  bool complete = false;
};

static int save_for_timing(psmf_filter* h, int64_t yp_rows, int64_t mu_rows, TimingSave& s) {
  ALLOC_TRY(h, s.C.alloc((size_t)h->cfg.d_local * h->geo.rp * h->elem()));
  ALLOC_TRY(h, s.st.alloc(sizeof(DevState)));
  ALLOC_TRY(h, s.th.alloc(4 * h->th_cap * sizeof(double)));
  HIP_TRY(h, hipMemcpy(s.C, h->C, s.C.bytes(), hipMemcpyDeviceToDevice));
  HIP_TRY(h, hipMemcpy(s.st, h->st, sizeof(DevState), hipMemcpyDeviceToDevice));
  HIP_TRY(h, hipMemcpy(s.th, h->thbuf, s.th.bytes(), hipMemcpyDeviceToDevice));
  int rc = save_step_records(h, yp_rows, mu_rows, s.rec);
  if (rc) return rc;
  HIP_TRY(h, hipDeviceSynchronize());      // (device-to-device copies on the null stream are not ordered against the handle's non-blocking stream)
  s.complete = true;
  return PSMF_OK;
}

static int restore_after_timing(psmf_filter* h, const TimingSave& s) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(h->C, s.C, s.C.bytes(), hipMemcpyDeviceToDevice));
  HIP_TRY(h, hipMemcpy(h->st, s.st, sizeof(DevState), hipMemcpyDeviceToDevice));
  HIP_TRY(h, hipMemcpy(h->thbuf, s.th, s.th.bytes(), hipMemcpyDeviceToDevice));
  return restore_step_records(h, s.rec);
}

static int time_step_kernels(psmf_filter* h, int which, int iters, float* avg_us) {
  {  // the sweep reads y_k / writes y_hat_k at the step counter: point it at a valid row of the series
    long long k0 = h->sp.series_t0;
    HIP_TRY(h, hipMemcpy(&h->st->k, &k0, sizeof(k0), hipMemcpyHostToDevice));
  }
  // which = 1 times the full serial stage (first = 0: reduction of the partials left by the last
  // sweep, updates, next-step preparation); the step counter it increments is reset with the state
  for (int i = 0; i < 3; ++i) { if (which == 0) launch_sweep(h); else launch_serial(h, 0); }
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < iters; ++i) { if (which == 0) launch_sweep(h); else launch_serial(h, 0); }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *avg_us = ms * 1000.f / iters;
  return PSMF_OK;
}

int psmf_time_kernel(psmf_handle h, int which, int iters, float* avg_us) {
  if (!h || !avg_us || iters < 1 || which < 0 || which > 2) return PSMF_ERR_ARG;
  if (!h->have_state || !h->Y) return fail(h, PSMF_ERR_STATE, "psmf_time_kernel: needs state and series");
  if (h->ring_slots) return fail(h, PSMF_ERR_STATE, std::string("psmf_time_kernel") + kRingRefused);
  int rc = set_device(h);
  if (rc) return rc;
  const bool blocked = h->engine == 2;
  if (!blocked && h->need_prep) { rc = prepare(h, h->k_done); if (rc) return rc; }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  // Save everything the kernels mutate; from here on there is one way out, which puts it back (the copies go with sv).
  TimingSave sv;
  double* const hist = h->sp.mu_hist;
  const int nb = (int)(h->T_cap < h->block_steps ? h->T_cap : h->block_steps);
  if (blocked) {
    rc = save_for_timing(h, nb, nb + 1, sv);       // the block's y_hat rows (apply) and posterior means (filter)
  } else {
    // the sweep writes y_hat of the series' first step; every launch of the serial stage advances the step counter and records
    // the posterior mean of that step: rows 1 .. iters + 3 of the history (a history shorter than that is not written at all)
    const int64_t serial_launches = (int64_t)iters + 3;
    if (serial_launches > h->T_cap) h->sp.mu_hist = nullptr;
    rc = save_for_timing(h, 1, h->sp.mu_hist ? serial_launches + 1 : 0, sv);
  }
  if (!rc) rc = blocked ? time_block_kernels(h, which, iters, nb, sv.st, avg_us) : time_step_kernels(h, which, iters, avg_us);
  h->sp.mu_hist = hist;
  if (sv.complete) { const int rc2 = restore_after_timing(h, sv); if (!rc) rc = rc2; }     // (a failed measurement too leaves the state as it found it)
  return rc;
}

int psmf_geometry(psmf_handle h, int32_t* out7) {
  if (!h || !out7) return PSMF_ERR_ARG;
  out7[0] = h->geo.n_sweep_wg; out7[1] = h->geo.rows_per_wg; out7[2] = h->geo.rp; out7[3] = h->geo.gs;
  out7[4] = h->chunk; out7[5] = h->engine; out7[6] = h->block_steps;
  return PSMF_OK;
}

int psmf_step_plan(psmf_handle h, int32_t* out5) {
  if (!h || !out5) return PSMF_ERR_ARG;
  if (set_device(h) != PSMF_OK) return PSMF_ERR_HIP;
  int n_cu = 0;
  HIP_TRY(h, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, h->cfg.device));
  out5[0] = pstep_usable(h) ? 1 : 0;
  out5[1] = h->ps_ok ? h->ps_plan.n_row_wg : 0; out5[2] = h->ps_ok ? h->ps_plan.rows_per_wg : 0; out5[3] = h->ps_ok ? h->ps_plan.np : 0;
  out5[4] = n_cu;
  return PSMF_OK;
}

#ifdef F4_DEBUG
// debug builds only (tools/probe_f4d.py): the scratch area the filter4 kernel writes its per-step residuals to
int psmf_debug_read(psmf_handle h, double* out, int n) {
  if (!h || !out) return PSMF_ERR_ARG;
  int rc = psmf_sync(h);
  if (rc) return rc;
  HIP_TRY(h, hipMemcpy(out, h->st->GR, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return PSMF_OK;
}
#endif

int psmf_filter_kernel(psmf_handle h) {
  if (!h) return PSMF_ERR_ARG;
  return (int)select_filter_kernel(h);
}

int psmf_counters(psmf_handle h, int64_t* out8, int reset) {
  if (!h || !out8) return PSMF_ERR_ARG;
  if (set_device(h) != PSMF_OK) return PSMF_ERR_HIP;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  long long c[8], g[8];
  HIP_TRY(h, hipMemcpy(c, h->st->cnt, sizeof(c), hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(g, h->st->dbg, sizeof(g), hipMemcpyDeviceToHost));
  for (int i = 0; i < 8; ++i) out8[i] = c[i];
  out8[6] = g[5];       // kernel launches of psmf_blk_filter3 (cnt[7] counts blocks; cnt[6] is a raw time stamp)
  if (h->sw.dbg_breakdown && c[7] > 0)
    fprintf(stderr, "[psmf] filter3 per launch: hand-off %.2f us, K %.2f, init %.2f, steps %.2f, end %.2f\n", 0.01 * g[0] / c[7], 0.01 * g[1] / c[7],
            0.01 * g[2] / c[7], 0.01 * g[3] / c[7], 0.01 * g[4] / c[7]);
  if (reset) { HIP_TRY(h, hipMemset(h->st->cnt, 0, sizeof(c))); HIP_TRY(h, hipMemset(h->st->dbg, 0, sizeof(g))); HIP_TRY(h, hipDeviceSynchronize()); }   // (before the next run's kernels on the non-blocking stream count)
  return PSMF_OK;
}

int psmf_filter_kernel_time(psmf_handle h, int64_t* launches, double* total_ms, int reset) {
  if (!h || !launches || !total_ms) return PSMF_ERR_ARG;
  int rc = psmf_sync(h);
  if (rc) return rc;
  *launches = h->kernel_launches;
  *total_ms = h->kernel_ms_sum;
  if (reset) { h->kernel_launches = 0; h->kernel_ms_sum = 0.0; }
  return PSMF_OK;
}

int psmf_predict(psmf_handle h, int64_t T, int64_t n_pred, double* out) {
  if (!h || !out || n_pred < 0) return PSMF_ERR_ARG;
  if (n_pred == 0) return PSMF_OK;
  int rc = psmf_sync(h);
  if (rc) return rc;
  if (h->cfg.dyn_kind == PSMF_DYN_HOST) return fail(h, PSMF_ERR_STATE, "psmf_predict: host-stepped dynamics roll mu forward on the host; use psmf_project");
  const int r = h->cfg.r;
  std::vector<double> mu(r), theta((size_t)(h->cfg.n_theta > 0 ? h->cfg.n_theta : 1), 0.0), mup((size_t)n_pred * r), nx(r);
  HIP_TRY(h, hipMemcpy(mu.data(), h->st->mu, r * sizeof(double), hipMemcpyDeviceToHost));
  if (h->cfg.n_theta) HIP_TRY(h, hipMemcpy(theta.data(), h->sp.theta, h->cfg.n_theta * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t q = 0; q < n_pred; ++q) {   // psmf.py:183-187, r-sized: done on the host
    dyn_f_host(h->cfg, theta.data(), mu.data(), (double)(T + q + 1), nx.data());
    mu = nx;
    for (int i = 0; i < r; ++i) mup[(size_t)q * r + i] = mu[i];
  }
  return psmf_project(h, mup.data(), n_pred, out);
}

int psmf_project(psmf_handle h, const double* mu, int64_t n_pred, double* out) {
  if (!h || !mu || !out || n_pred < 0) return PSMF_ERR_ARG;
  if (n_pred == 0) return PSMF_OK;
  int rc = psmf_sync(h);
  if (rc) return rc;
  const int r = h->cfg.r, dl = h->cfg.d_local;
  const size_t nmu = (size_t)n_pred * r;
  const size_t mbytes = nmu * sizeof(double), obytes = (size_t)n_pred * dl * sizeof(double);
  rc = ensure_scratch(h, mbytes + obytes);
  if (rc) return rc;
  double* dmu = h->scratch;
  double* dout = h->scratch + nmu;
  HIP_TRY(h, hipMemcpy(dmu, mu, mbytes, hipMemcpyHostToDevice));
  const int grid = (dl + psmf::WG - 1) / psmf::WG;
  const size_t lds = (size_t)64 * r * sizeof(double);
  by_storage(h, [&](auto t) {
    hipLaunchKernelGGL(psmf::psmf_predict_rows<decltype(t)>, dim3(grid), dim3(psmf::WG), lds, h->stream,
                       h->C.as<const decltype(t)>(), dl, r, h->geo.rp, (const double*)dmu, (int)n_pred, dout);
  });
  HIP_TRY(h, hipGetLastError());
  if (h->rotU) {                         // non-diagonal R: C here is U^T C -- rotate the projections back
    rc = ensure_rot_tmp(h, obytes);
    if (rc) return rc;
    rc = rot_gemm(h, (const double*)dout, (long long)dl, 1LL, (const double*)h->rotU, 1LL, (long long)dl, h->rot_tmp.as<double>(), (long long)dl,
                  (long long)n_pred, (long long)dl, (long long)dl);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, h->rot_tmp, obytes, hipMemcpyDeviceToHost));
    return PSMF_OK;
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(out, dout, obytes, hipMemcpyDeviceToHost));
  return PSMF_OK;
}

int psmf_predict_sq_error(psmf_handle h, int64_t T, int64_t n_pred, const double* Y_true, double* out) {
  if (!h || !Y_true || !out || n_pred < 0) return PSMF_ERR_ARG;
  *out = 0.0;
  if (n_pred == 0) return PSMF_OK;
  const size_t dl = h->cfg.d_local, n = (size_t)n_pred * dl;
  std::vector<double> yp(n);
  int rc = psmf_predict(h, T, n_pred, yp.data());      // leaves the roll-out in the scratch buffer: [mu_pred | y_hat]
  if (rc) return rc;
  const size_t off = (size_t)n_pred * h->cfg.r;
  rc = ensure_scratch(h, (off + 2 * n + kSqErrorParts) * sizeof(double));      // (may move the buffer: upload the roll-out again)
  if (rc) return rc;
  double* dyp = h->scratch + off;
  double* dyt = dyp + n;
  HIP_TRY(h, hipMemcpy(dyp, yp.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(dyt, Y_true, n * sizeof(double), hipMemcpyHostToDevice));
  return sq_error_sum(h, h->stream, PSMF_F64, dyp, dyt, n, dyt + n, out);
}

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

int psmf_set_row_noise(psmf_handle h, const double* rho_rows, double rho_mean) {
  if (!h || !rho_rows || !(rho_mean > 0.0)) return fail(h, PSMF_ERR_ARG, "psmf_set_row_noise: bad argument");
  if (!h->cfg.nonuniform_R) return fail(h, PSMF_ERR_STATE, "psmf_set_row_noise: the handle was created with nonuniform_R = 0");
  for (int i = 0; i < h->cfg.d_local; ++i)
    if (!(rho_rows[i] >= 0.0)) return fail(h, PSMF_ERR_ARG, "psmf_set_row_noise: diag(R) must be non-negative");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  ALLOC_TRY(h, h->rho_rows.reserve((size_t)h->cfg.d_local * sizeof(double)));
  HIP_TRY(h, hipMemcpy(h->rho_rows, rho_rows, (size_t)h->cfg.d_local * sizeof(double), hipMemcpyHostToDevice));
  h->sp.rho_rows = h->rho_rows;
  h->sp.rho_mean = rho_mean;
  destroy_graph(h);
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_set_noise_rotation(psmf_handle h, const double* U, const double* lam) {
  if (!h || !U || !lam) return fail(h, PSMF_ERR_ARG, "psmf_set_noise_rotation: bad argument");
  if (!h->cfg.nonuniform_R) return fail(h, PSMF_ERR_STATE, "psmf_set_noise_rotation: the handle was created with nonuniform_R = 0");
  if (h->cfg.masked) return fail(h, PSMF_ERR_STATE, "psmf_set_noise_rotation: not on a masked handle (the mask selects rows of the ORIGINAL coordinates: it is not equivariant under a rotation)");
  if (h->use_coll || h->cfg.d_local != h->cfg.d)
    return fail(h, PSMF_ERR_STATE, "psmf_set_noise_rotation: a non-diagonal R couples all rows: one shard only (d_local = d, no communicator)");
  if (h->ring_slots) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_noise_rotation") + kRingRefused + ": the rotation of the rows would have to run on the copy stream");
  if (h->Y || h->have_state) return fail(h, PSMF_ERR_STATE, "psmf_set_noise_rotation: call it before psmf_set_state / psmf_upload_series");
  const size_t d = (size_t)h->cfg.d;
  double tr = 0.0;
  for (size_t i = 0; i < d; ++i) {
    if (!(lam[i] >= 0.0)) return fail(h, PSMF_ERR_ARG, "psmf_set_noise_rotation: eigenvalues of R must be non-negative");
    tr += lam[i];
  }
  if (!(tr > 0.0)) return fail(h, PSMF_ERR_ARG, "psmf_set_noise_rotation: tr(R) must be positive");
  if (d > (size_t)PSMF_ROTATION_DMAX)
    return fail(h, PSMF_ERR_ARG, "psmf_set_noise_rotation: a non-diagonal R is supported up to d = 32768 (the handle keeps the d x d eigenvector matrix "
                                 "resident: 8 d^2 bytes); beyond that use a diagonal R or backend=\"numpy\"");
  // orthonormality over ALL of U in O(d^2): U^T (U z) = z for two probe vectors z (+-1 entries from a fixed generator).  A column
  // pair that is not orthonormal shows in (U^T U - I) z unless z lies in that matrix's null space -- two independent sign
  // patterns do not.  (The full check U^T U = I is O(d^3); a C caller with a wrong U used to get a silently wrong filter.)
  {
    std::vector<double> z(d), t(d), u(d);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int probe = 0; probe < 2; ++probe) {
      for (size_t i = 0; i < d; ++i) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; z[i] = (lcg >> 63) ? 1.0 : -1.0; }
      for (size_t i = 0; i < d; ++i) { double a = 0.0; const double* row = U + i * d; for (size_t k = 0; k < d; ++k) a += row[k] * z[k]; t[i] = a; }
      for (size_t k = 0; k < d; ++k) u[k] = 0.0;
      for (size_t i = 0; i < d; ++i) { const double ti = t[i]; const double* row = U + i * d; for (size_t k = 0; k < d; ++k) u[k] += row[k] * ti; }
      double worst = 0.0;
      for (size_t k = 0; k < d; ++k) worst = std::fmax(worst, std::fabs(u[k] - z[k]));
      if (!(worst <= 1e-8 * std::sqrt((double)d) + 1e-10))
        return fail(h, PSMF_ERR_ARG, "psmf_set_noise_rotation: the columns of U are not orthonormal (U^T U z != z)");
    }
  }
  int rc = psmf_set_row_noise(h, lam, tr / (double)d);
  if (rc) return rc;
  ALLOC_TRY(h, h->rotU.reserve(d * d * sizeof(double)));
  HIP_TRY(h, hipMemcpy(h->rotU, U, d * d * sizeof(double), hipMemcpyHostToDevice));
  return PSMF_OK;
}

int psmf_set_schedules(psmf_handle h, const double* rho_k, const double* q_k, int64_t n) {
  if (!h || n < 0) return PSMF_ERR_ARG;
  if (h->cfg.robust && (rho_k || q_k)) return fail(h, PSMF_ERR_ARG, "psmf_set_schedules: rPSMF runs on its own scaled Q, R (rpsmf.py:123,128,141)");
  if (h->cfg.masked && (rho_k || q_k)) return fail(h, PSMF_ERR_ARG, "psmf_set_schedules: masked handles take a constant R = rho I, Q (the ExperimentImpute filters)");
  if (h->ring_slots && (rho_k || q_k) && n > 0) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_schedules") + kRingRefused + ": the schedules are not windowed");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->sched.reset();
  h->sched_n = 0;
  h->sp.rho_sched = h->sp.q_sched = nullptr;
  if ((rho_k || q_k) && n > 0) {
    // n + 1 entries each, the last one repeated: having finished step k the per-step engine's serial stage prepares step
    // k + 1 and reads entry k + 1 -- one past the schedule on the last step of a run (the value is recomputed by the next prepare)
    std::vector<double> buf((size_t)2 * (n + 1), 1.0);
    if (rho_k) { memcpy(buf.data(), rho_k, (size_t)n * sizeof(double)); buf[n] = rho_k[n - 1]; }
    if (q_k) { memcpy(buf.data() + n + 1, q_k, (size_t)n * sizeof(double)); buf[2 * n + 1] = q_k[n - 1]; }
    ALLOC_TRY(h, h->sched.alloc(buf.size() * sizeof(double)));
    HIP_TRY(h, hipMemcpy(h->sched, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
    h->sched_n = n;
    if (rho_k) h->sp.rho_sched = h->sched;
    if (q_k) h->sp.q_sched = h->sched + n + 1;
  }
  update_solve_dual(h);
  destroy_graph(h);      // the graph's kernel nodes carry StepParams by value
  { const int zero = 0; HIP_TRY(h, hipMemcpy(&h->st->ns_valid, &zero, sizeof(int), hipMemcpyHostToDevice)); }   // another filter kernel may run next: no carried register dump
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_set_q_matrix_schedule(psmf_handle h, const double* Q_k, int64_t n) {
  if (!h || n < 0) return PSMF_ERR_ARG;
  if (Q_k && n > 0) {
    if (h->ring_slots) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_q_matrix_schedule") + kRingRefused + ": the schedule is not windowed");
    if (h->cfg.robust) return fail(h, PSMF_ERR_ARG, "psmf_set_q_matrix_schedule: rPSMF runs on its own scaled Q (rpsmf.py:123,128)");
    if (h->cfg.masked) return fail(h, PSMF_ERR_ARG, "psmf_set_q_matrix_schedule: masked handles take a constant Q (the ExperimentImpute filters)");
    if (h->engine != 1) return fail(h, PSMF_ERR_ARG, "psmf_set_q_matrix_schedule: a Q_k that is not a multiple of Q_1 needs the per-step engine (engine = 1)");
    if (h->cfg.dyn_kind == PSMF_DYN_HOST) return fail(h, PSMF_ERR_ARG, "psmf_set_q_matrix_schedule: host-stepped dynamics form P_bar (and add Q_k) on the host");
  }
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->qmat.reset();
  h->qmat_n = 0;
  h->sp.q_mat = nullptr;
  if (Q_k && n > 0) {
    // n + 1 matrices, the last one repeated (as in psmf_set_schedules: the serial stage prepares one step ahead)
    const size_t rr = (size_t)h->cfg.r * h->cfg.r;
    ALLOC_TRY(h, h->qmat.alloc((size_t)(n + 1) * rr * sizeof(double)));
    HIP_TRY(h, hipMemcpy(h->qmat, Q_k, (size_t)n * rr * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->qmat + (size_t)n * rr, Q_k + (size_t)(n - 1) * rr, rr * sizeof(double), hipMemcpyHostToDevice));
    h->qmat_n = n;
    h->sp.q_mat = h->qmat;
  }
  update_solve_dual(h);
  destroy_graph(h);      // the graph's kernel nodes carry StepParams by value
  { const int zero = 0; HIP_TRY(h, hipMemcpy(&h->st->ns_valid, &zero, sizeof(int), hipMemcpyHostToDevice)); }
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_step_host(psmf_handle h, int64_t k, const double* mu_bar, const double* P_bar, double* mu_out, double* gf_out,
                   double* P_out, double* Q_out) {
  if (!h || !mu_bar || !P_bar) return PSMF_ERR_ARG;
  if (h->cfg.dyn_kind != PSMF_DYN_HOST) return fail(h, PSMF_ERR_STATE, "psmf_step_host: the handle was not created with dyn_kind = PSMF_DYN_HOST");
  if (!h->have_state) return fail(h, PSMF_ERR_STATE, "psmf_step_host: set_state (C, V, P, mu) first");
  if (!h->Y) return fail(h, PSMF_ERR_STATE, "psmf_step_host: upload_series first");
  if (k < 0 || k >= h->T_cap) return fail(h, PSMF_ERR_ARG, "psmf_step_host: step outside the uploaded series");
  if (h->sched && k + 1 >= h->sched_n) return fail(h, PSMF_ERR_ARG, "psmf_step_host: step beyond the R / Q schedules");
  int rc = set_device(h);
  if (rc) return rc;
  const int r = h->cfg.r;
  if (h->need_prep || h->k_done != k) {
    hipLaunchKernelGGL(psmf::psmf_prepare_k, dim3(1), dim3(1), 0, h->stream, h->st, (long long)k);
    if (h->mu_hist)
      HIP_TRY(h, hipMemcpyAsync(h->mu_hist + (size_t)(k - h->sp.series_t0) * r, h->st->mu, r * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (h->sp.track_g) { rc = enqueue_gram(h); if (rc) return rc; }
    h->need_prep = false;
    h->k_done = k;
  }
  HIP_TRY(h, hipMemcpyAsync(h->st->mu_bar, mu_bar, r * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->st->Pbar, P_bar, (size_t)r * r * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_serial(h, 1);          // w, s, eta, N, kappa of this step from the uploaded mu_bar, P_bar
  rc = enqueue_step(h);         // row sweep (+ r x r solve), all-reduce, serial stage (stops before the next prediction)
  if (rc) return rc;
  HIP_TRY(h, hipGetLastError());
  h->k_done = k + 1;
  rc = psmf_sync(h);
  if (rc) return rc;
  if (mu_out) HIP_TRY(h, hipMemcpy(mu_out, h->st->mu, r * sizeof(double), hipMemcpyDeviceToHost));
  if (gf_out) HIP_TRY(h, hipMemcpy(gf_out, h->st->gf, r * sizeof(double), hipMemcpyDeviceToHost));
  if (P_out) HIP_TRY(h, hipMemcpy(P_out, h->st->P, (size_t)r * r * sizeof(double), hipMemcpyDeviceToHost));
  if (Q_out) HIP_TRY(h, hipMemcpy(Q_out, h->st->Q, (size_t)r * r * sizeof(double), hipMemcpyDeviceToHost));
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

int psmf_device_pci_bus_id(int device, char* buf, int len) {
  if (!buf || len < 16) return fail(nullptr, PSMF_ERR_ARG, "psmf_device_pci_bus_id: buffer of at least 16 bytes");
  if (hipDeviceGetPCIBusId(buf, len, device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, PSMF_ERR_HIP, "hipDeviceGetPCIBusId failed"); }
  return PSMF_OK;
}

/* ---- masked filter on the large-d handle (psmf_masked.hip) ------------------------------------------------------------- */
int psmf_set_step_size(psmf_handle h, double gam) {
  if (!h || !(gam >= 0.0)) return fail(h, PSMF_ERR_ARG, "psmf_set_step_size: bad argument");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(&h->st->sgd_gamma, &gam, sizeof(double), hipMemcpyHostToDevice));
  return PSMF_OK;
}

int psmf_measure_copy_bandwidth(int device, size_t bytes, int iters, double* gbps) {
  if (!gbps || iters < 1 || bytes < (size_t)1 << 20) return fail(nullptr, PSMF_ERR_ARG, "psmf_measure_copy_bandwidth: bad argument");
  psmf_handle h = nullptr;       // errors go to the create-error slot
  HIP_TRY(h, hipSetDevice(device));
  const size_t n16 = bytes / 16;
  Dev<float4> src, dst;
  Event e0, e1;
  Stream s;
  ALLOC_TRY(h, src.alloc(n16 * 16));
  ALLOC_TRY(h, dst.alloc(n16 * 16));
  HIP_TRY(h, hipMemset(src, 1, n16 * 16));
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipStreamCreateWithFlags(s.put(), hipStreamNonBlocking));
  HIP_TRY(h, hipEventCreate(e0.put()));
  HIP_TRY(h, hipEventCreate(e1.put()));
  // four 16-byte vectors per thread (measured on MI355X, 1 GiB: 4.1 TB/s with 4 workgroups per CU, 5.0 with one workgroup
  // per 16 KiB; 4 GiB: 5.5 TB/s)
  size_t gsz = n16 / ((size_t)psmf::WG * 4);
  if (gsz < 1024) gsz = 1024;
  if (gsz > ((size_t)1 << 20)) gsz = (size_t)1 << 20;
  const int copy_grid = Switches().copy_grid;
  const int grid = copy_grid ? copy_grid : (int)gsz;
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(psmf::psmf_copy_k, dim3(grid), dim3(psmf::WG), 0, s, (const float4*)src, (float4*)dst, n16);
  HIP_TRY(h, hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(psmf::psmf_copy_k, dim3(grid), dim3(psmf::WG), 0, s, (const float4*)src, (float4*)dst, n16);
  HIP_TRY(h, hipEventRecord(e1, s));
  HIP_TRY(h, hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, e0, e1));
  *gbps = 2.0 * (double)(n16 * 16) * iters / (ms * 1e-3) / 1e9;     // read + write
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
