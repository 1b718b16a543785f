// The launched per-step engine of the large-d handle: two -- masked: three -- launches per timestep, captured into a hipGraph and
// replayed over the series (psmf_kernels.hip, psmf_masked.hip, psmf_wave16.hip), and the host driver of the persistent per-step
// kernel (psmf_pstep.hip).  The C ABI unit (psmf_capi.hip) reaches it through init_step, prepare_step, run_step_engine,
// time_step_kernels, pstep_usable, destroy_graph and print_pstep_prof.
#include "psmf_host.h"
#include "psmf_kernels.hip"
#include "psmf_masked.hip"
#include "psmf_wave16.hip"     // solve_block_wave: the per-step engine's solve block

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

namespace {

#ifndef PSMF_SWEEP_UNROLL
#define PSMF_SWEEP_UNROLL 4
#endif
constexpr int kUnroll = PSMF_SWEEP_UNROLL;      // row passes (16-byte loads per lane) in flight in the sweep

// A kernel whose dynamic LDS may need the opt-in (hipFuncAttributeMaxDynamicSharedMemorySize): init_step sets it for the
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

}  // namespace

// the captured graph holds buffer addresses and a copy of StepParams: whoever changes either (psmf_capi.hip, psmf_comm.hip,
// psmf_series.hip) drops it
void destroy_graph(psmf_filter* h) {
  if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
  if (h->graph) { hipGraphDestroy(h->graph); h->graph = nullptr; }
  h->chunk = 0;
}

namespace {

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

}  // namespace

// psmf_create, behind the buffers of every engine and whichever engine the handle runs: the LDS opt-ins of this unit's kernels, then
// the persistent kernel's plan
int init_step(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  int rc = PSMF_OK;
  // dynamic LDS beyond the default limit: opted in here, per handle and so on the handle's device, for the kernels it can launch
  if (!rc && h->geo.sweep_lds > 48 * 1024) rc = opt_in_lds(h, (const void*)sweep_kernel(h), h->geo.sweep_lds);
  if (!rc && cfg->masked) { const serial_mgram_t k = serial_mgram_kernel(h); rc = opt_in_lds(h, (const void*)k.fn, k.lds); }
  if (!rc && cfg->nonuniform_R) { const wgram_t k = wgram_kernel(h); rc = opt_in_lds(h, (const void*)k.fn, k.lds); }
  if (!rc) rc = init_pstep(h);
  return rc;
}

// start-of-run preparation of the per-step engine, behind prepare (psmf_capi.hip): exact Gram, then everything the first sweep needs
int prepare_step(psmf_filter* h, int64_t k_begin) {
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

// the steps k_begin + 1 .. k_end of a prepared run (run_steps, psmf_capi.hip) on the per-step engine
int run_step_engine(psmf_filter* h, int64_t k_begin, int64_t k_end) {
  int rc = PSMF_OK;
  int64_t n = k_end - k_begin;
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

// psmf_time_kernel on the per-step engine: between its save and its restore (psmf_capi.hip)
int time_step_kernels(psmf_filter* h, int which, int iters, float* avg_us) {
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

extern "C" {

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
    launch_prepare_k(h, k);
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

}  // extern "C"
