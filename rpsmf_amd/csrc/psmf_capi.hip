// C ABI of libpsmf_hip.so (include/psmf_hip.h): the glue of the large-d handle.  One handle = one HIP stream and one device-resident
// filter (or row shard); this unit creates and destroys it, moves its state, checks and dispatches a run, and waits.  The engines
// that advance the filter are units of their own -- launched per-step and persistent (psmf_step.hip, psmf_pstep.hip), blocked
// (psmf_blocked.hip) -- as are the series buffers (psmf_series.hip), the communicator (psmf_comm.hip) and the noise rotation
// (psmf_rotation.hip); the only kernels launched here are the four of psmf_handle_kernels.hip.  No torch, no hipBLAS: plain HIP + RCCL.
// The batched entry points without a handle (psmf_impute_*, psmf_ssm_*, psmf_bocpd_run) live in the units of their engines.
#include "psmf_host.h"
#include "psmf_dyn.hip"        // dyn_n_theta, dyn_term: the term structure of f_theta, for check_config and the host roll-out
#include "psmf_handle_kernels.hip"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

thread_local std::string g_create_error;

int ensure_scratch(psmf_filter* h, size_t bytes) {
  ALLOC_TRY(h, h->scratch.reserve(bytes));
  return PSMF_OK;
}

// start of a run: the step counter, by a one-thread kernel on the handle's stream (psmf_step_host, psmf_step.hip, starts its runs with it too)
void launch_prepare_k(psmf_filter* h, int64_t k) {
  hipLaunchKernelGGL(psmf::psmf_prepare_k, dim3(1), dim3(1), 0, h->stream, h->st, (long long)k);
}

namespace {

int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

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
  return prepare_step(h, k_begin);
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
  if (!rc) rc = init_step(h);
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
  return h->engine == 2 ? run_blocks(h, k_begin, k_end) : run_step_engine(h, k_begin, k_end);
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
    rc = rot_rows_back_f64(h, dout, h->rot_tmp.as<double>(), n_pred);
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

}  // extern "C"
