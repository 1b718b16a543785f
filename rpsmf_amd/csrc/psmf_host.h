// Host side of libpsmf_hip.so, shared by its translation units (psmf_capi.hip, psmf_step.hip, psmf_comm.hip, psmf_rotation.hip, psmf_series.hip,
// psmf_blocked.hip, psmf_filter34.hip, psmf_impute.hip, psmf_ssm.hip, psmf_bocpd.hip, psmf_pmf.hip, psmf_bpmf.hip): the handle, the switch table, the error helpers and the few host functions that cross
// unit boundaries.  A kernel is launched -- and its LDS opt-in is made -- only in the unit that defines it (the rule of psmf_pstep.h);
// across units only these functions are called; the entry points without a handle (the last five units) stand on psmf_batch.h.
#pragma once
#include "../../include/psmf_hip.h"
#include "psmf_block.h"       // BlockParams
#include "psmf_own.h"         // Event, Stream, Dev<T>, Pinned<T>: what owns a device resource
#include "psmf_pstep.h"       // persistent per-step engine: its kernels are a translation unit of their own (psmf_pstep.hip)

#include <rccl/rccl.h>

#include <chrono>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

using psmf::DevState;
using psmf::StepParams;

extern thread_local std::string g_create_error;      // the message of a failure without a handle (psmf_capi.hip)

struct Geometry {
  int vec, nv, rp, gs, rpp, rpad, nt;
  int n_sweep_wg, rows_per_wg, ps;
  size_t sweep_lds;
};

// Environment switches: one row each, and this struct is the library's only reader of the environment.  The rows
// are read when a Switches is constructed: ONCE per handle, with the handle at psmf_create -- tests flip them between handles of one
// process, and nothing on the per-block host path looks at the environment; the entry points without a handle (psmf_impute_*,
// psmf_measure_copy_bandwidth, psmf_bocpd_run, psmf_pmf_run, psmf_bpmf_run, psmf_conv_run) construct one at entry, on every call.
struct Switches {
  static bool set(const char* name) { return getenv(name) != nullptr; }                                  // present at all
  static bool on(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }           // set and non-zero
  static bool off(const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; }          // set to zero
  static int as_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
  static double as_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }

  int engine_env = as_int("PSMF_ENGINE", 0);             // 1 | 2: force the per-step / blocked engine (2 only where the blocked engine applies)
  // blocked engine; "=0" puts the older / more general kernel in the place of the role-specialised one
  bool bulk2 = !off("PSMF_BULK2");                       // streaming cross-Gram / apply kernels (psmf_bulk.hip)
  bool filter3 = !off("PSMF_FILTER3"), filter4 = !off("PSMF_FILTER4"), filter6 = !off("PSMF_FILTER6"), filter7 = !off("PSMF_FILTER7");
  bool filter6_dual = !off("PSMF_FILTER6_DUAL"), block_dual = !off("PSMF_BLOCK_DUAL");      // the two inversions side by side
  bool block_pipe = !off("PSMF_BLOCK_PIPE");             // =0: blocks one after the other
  bool block_chain = !off("PSMF_BLOCK_CHAIN");           // =0: one filter launch per block
  bool chain_carry = !off("PSMF_CHAIN_CARRY");           // =0: the blocks of a chained filter3 launch hand the r x r state on through DevState
  bool xg_ahead = !off("PSMF_XG_AHEAD");                 // =0: a carried block loads its cross-Gram behind the hand-off's barrier, not in front of the store drain
  bool block_flags = !off("PSMF_BLOCK_FLAGS");           // =0: event hand-off instead of device flags
  int reserved_cus = as_int("PSMF_RESERVED_CUS", 8);     // CUs that the filter chain's stream owns
  int bulk_wgs_env = as_int("PSMF_BULK_WGS", 0);         // workgroups of the streaming bulk kernels (8..256, rounded down to a multiple of 8 where it is used)
  bool host_comm_flags = on("PSMF_HOST_COMM_FLAGS");     // device-flag hand-off (and chained filter launches) under a host-mediated communicator too
  bool force_collective = set("PSMF_FORCE_COLLECTIVE");  // the RCCL path with one rank
  // per-step engine
  bool step_persistent = !off("PSMF_STEP_PERSISTENT");   // one persistent launch per run (psmf_pstep.hip) where it applies; =0: two launches per timestep
  bool pstep_big = !off("PSMF_PSTEP_BIG");               // =0: the persistent kernel for r <= 32 only
  bool pstep_prof = set("PSMF_PSTEP_PROF");              // diagnostic (-DPSTEP_PROF builds): per-phase clock sums, printed at psmf_destroy
  bool wave_solve = !off("PSMF_STEP_WAVE_SOLVE"), wave_big = !off("PSMF_STEP_WAVE_BIG");      // =0: LDS-and-barrier sweeps in the solve block, for every r / for r > 32
  bool step_dual = !off("PSMF_STEP_DUAL"), serial_wide = !off("PSMF_SERIAL_WIDE"), wgram_mfma = !off("PSMF_WGRAM_MFMA");
  int sweep_threads = as_int("PSMF_SWEEP_THREADS", 512) == 256 ? 256 : 512;
  int tail_reduce = as_int("PSMF_TAIL_REDUCE", -1);      // 0 | 1: the serial stage / the last row workgroup sums the partial rows (unset: by shape)
  // Newton-Schulz starts of the inversions; the *_set ones have defaults that depend on the handle (fill_step_params, update_ns_policy)
  bool ns = !off("PSMF_NS");                             // =0: direct sweeps only
  int ns_predict = as_int("PSMF_NS_PREDICT", 7);         // bits: 1 a / b (phase F), 2 core (wave 7), 4 applied
  bool ns_tol_set = set("PSMF_NS_TOL"); double ns_tol = as_double("PSMF_NS_TOL", 0.0);      // diagnostic: acceptance tolerance
  bool ns_far_set = set("PSMF_NS_FAR"); double ns_far = as_double("PSMF_NS_FAR", 0.3);      // diagnostic: residual at which a start is given up
  bool ns_skip_set = set("PSMF_NS_SKIP"); int ns_skip = as_int("PSMF_NS_SKIP", 3);          // diagnostic: timesteps that then sweep unasked
  double ns_far4 = as_double("PSMF_NS_FAR4", 0.6);       // filter4 / filter4s: their give-up residual (PSMF_NS_FAR, when set, rules both)
  // small-shape masked engine (psmf_impute.hip)
  bool impute_v3 = !off("PSMF_IMPUTE_V3"), impute_par = !off("PSMF_IMPUTE_PAR");      // =0: round 2's loop for the small shapes too; inversions one after the other
  // change-point detection (psmf_bocpd.hip)
  int bocpd_chunk = as_int("PSMF_BOCPD_CHUNK", 0);       // n > 0: at most n series per chunk, still capped by free memory (0, unset: sized from free memory alone)
  // probabilistic matrix factorisation (psmf_pmf.hip)
  int pmf_cols = as_int("PSMF_PMF_COLS", 0);             // n > 0: columns per workgroup, rounded up to a multiple of 16 (0, unset: from n, at most 64 workgroups a replica)
  int pmf_chunk = as_int("PSMF_PMF_CHUNK", 0);           // n > 0: at most n replicas per chunk, still capped by free memory (0, unset: sized from free memory alone)
  // Bayesian probabilistic matrix factorisation (psmf_bpmf.hip)
  int bpmf_cols = as_int("PSMF_BPMF_COLS", 0);           // n > 0: columns per workgroup, rounded up to a multiple of 4 (0, unset: from n, at most 64 workgroups a replica)
  int bpmf_chunk = as_int("PSMF_BPMF_CHUNK", 0);         // n > 0: at most n replicas per chunk, still capped by free memory (0, unset: sized from free memory alone)
  // convergence experiment (psmf_conv.hip)
  int conv_chunk = as_int("PSMF_CONV_CHUNK", 0);         // n > 0: at most n replicas per chunk, still capped by free memory (0, unset: sized from free memory alone)
  int conv_iters = as_int("PSMF_CONV_ITERS", 0);         // k > 0: at most k iterations per launch (0, unset: the most with n k <= 2^20 steps)
  // diagnostics
  bool dbg_breakdown = set("PSMF_DBG_BREAKDOWN");        // psmf_counters prints the in-situ breakdown of a filter3 launch
  bool host_timing = on("PSMF_HOST_TIMING");             // report slow host-side enqueues and waits
  int copy_grid = as_int("PSMF_COPY_GRID", 0);           // grid of the copy-bandwidth probe (0, unset: sized from the buffer)
};

// Every device resource of a handle is a member of an owning type (psmf_own.h) and is released when the handle is deleted.
// psmf_destroy waits for all of the handle's streams first, so the order in which the members release is immaterial.  StepParams /
// BlockParams carry raw copies of the pointers into the kernels: they are set where the buffer is allocated.
struct psmf_filter {
  psmf_config cfg;
  Geometry geo;
  Switches sw;
  Stream stream;
  Dev<DevState> st;
  Dev<void> C, Y, YP;
  Dev<double> partials, gpart;
  Dev<double> thbuf;           // theta | gradsum | adam_m | adam_v, th_cap doubles each
  size_t th_cap = 0;
  Dev<double> rho_rows;        // d_local per-row diag(R) (cfg.nonuniform_R)
  Dev<double> rotU;            // d x d: eigenvectors of a non-diagonal R in its columns (psmf_set_noise_rotation); series, C, y_hat are kept rotated
  Dev<void> rot_tmp;           // staging of a rotation (the GEMM is out of place); grows on demand
  // masked filter (cfg.masked, psmf_masked.hip)
  Dev<uint8_t> mask;           // T_cap x d_local observation mask (psmf_upload_mask)
  Dev<uint8_t> mmiss;          // staging of the held-out mask for psmf_masked_metrics; grows on demand
  Dev<double> mg;              // r*r + 1: masked Gram and observed count of the current step, summed over workgroups (and ranks)
  Dev<double> sc_hist;         // T_cap x 2: (s_k, eta_k) of every step -- the bands are formed from them
  bool have_mask = false;
  int64_t mask_hi = 0;         // resident series: the mask has been uploaded for the series rows [0, mask_hi)
  Dev<double> sched;           // rho_k | q_k schedules, sched_n doubles each (psmf_set_schedules)
  int64_t sched_n = 0;
  Dev<double> qmat;            // Q_k matrices, (qmat_n + 1) x r x r (psmf_set_q_matrix_schedule)
  int64_t qmat_n = 0;
  Dev<double> mu_hist;         // (T_cap + 1) x r
  Stream fstream;                  // blocked engine, pipelined: the filter chain's own stream, pinned to reserved CUs (or empty)
  bool streams_concurrent = false;           // the filter stream's kernels run concurrently with the bulk stream's (probed at creation)
  // HIP-event timing of the chained filter launches (one per run): a ring of event pairs, read out at the next sync
  static constexpr int kTimedRuns = 256;
  Event evK0[kTimedRuns], evK1[kTimedRuns];
  Event evC;                       // end of the chained filter launch: orders the handle's main stream (host reads of DevState) after it
  int evk_pending = 0;
  double kernel_ms_sum = 0.0;
  long long kernel_launches = 0;
  int reserved_cus = 0;
  int bulk_wgs = 256;          // workgroups of the streaming bulk kernels (one per CU of the bulk stream: a 257th would wait for a whole round)
  Dev<double> scratch;         // sq-error partials / predict staging; grows on demand
  // blocked engine
  int engine = 1;              // 1 per-step, 2 blocked
  int block_steps = 0;         // B = RB - r
  bool q_iso = false;          // Q = q I with q > 0 as last uploaded (two-group block filter applies)
  double q_last = 0.0, p_diag_max = 0.0;      // Q[0][0] and max_i P[i][i] as last uploaded: the give-up policy of the Newton-Schulz starts (update_ns_policy)
  Dev<double> Kpart, Kmat;
  Dev<double> Acoef;           // 2 x RB x RM   (ping-pong across pipelined blocks)
  Dev<double> Bcoef;           // 2 x RB x RB
  Dev<double> XGpart;          // BLK_GRAM_WG x (RB + XGB) x XGB
  Dev<double> XG;              // 2 x (RB + XGB) x XGB
  Dev<long long> flags;        // device-flag hand-off of the pipelined blocks (psmf_block.hip): xg_seq, filt_seq, abort
  long long seq_next = 1;      // sequence number of the next block to be enqueued
  Stream bulk;                 // Gram / cross-Gram / apply of the pipelined blocked engine
  Event evF[4], evA[4], evX[4], evS;
  int64_t T_cap = 0;
  // series ring (psmf_series_ring): the series buffers hold ring_slots windows of ring_chunk rows; chunk c of the stream lives in slot
  // c % ring_slots and is run with sp.series_t0 = (c - slot) * ring_chunk.  ring_slots = 0: the whole series is resident.
  struct RingSlot {
    int64_t chunk = -1;          // chunk of the stream the slot holds (-1: none)
    int64_t rows = 0, mrows = 0; // series / mask rows of it uploaded so far
    Event up;                    // the last upload into the slot (copy stream)
    Event run;                   // the last run that touched the slot (compute stream)
    bool up_set = false, run_set = false;
  };
  int64_t ring_chunk = 0;
  int ring_slots = 0;
  int64_t ring_cur = -1;           // the chunk sp.series_t0 (and the histories' slot base) point at
  std::vector<RingSlot> ring;
  Stream cstream;                  // the ring's copy stream: uploads, downloads, row conversion
  Dev<void> ring_stage;            // device staging of one chunk in the caller's element type (psmf_cast_rows converts from / into it)
  bool ring_mg_stale = false;      // masked: the Gram formed one step ahead read a mask row that was not resident yet
  StepParams sp;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int chunk = 0;
  // persistent per-step engine (psmf_pstep.hip): geometry of a launch and its communication block (flags | packet | partial rows)
  psmf::PstepPlan ps_plan = {};
  bool ps_ok = false;
  Dev<void> ps_comm;
  Dev<long long> ps_prof;          // PSMF_PSTEP_PROF=1 with a -DPSTEP_PROF build: per-phase clock sums of the last launch, printed at psmf_destroy
  long long ps_prof_steps = 0;
  long long ps_launches = 0;
  bool have_state = false;
  bool need_prep = true;
  int64_t k_done = 0;
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  bool use_coll = false;   // per-step all-reduce on (nranks > 1, or forced for single-GPU testing)
  // host-mediated collective (psmf_comm_init_host): the sum-all-reduce goes through a caller-supplied function
  psmf_allreduce_fn host_fn = nullptr;
  void* host_ctx = nullptr;
  Pinned<double> host_buf;         // pinned staging buffer, kHostBufElems doubles
  static constexpr size_t kHostBufElems = 8192;
  Event ev0, ev1;
  Pinned<int> err_host;        // pinned, device-mapped: a one-thread kernel publishes the device error flag here
  int* err_host_dev = nullptr; // the device address of err_host
  std::string err;
  size_t elem() const { return cfg.storage == PSMF_F64 ? 8 : 4; }
};

namespace {

int fail(psmf_handle h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

#define HIP_TRY_AS(h, what, expr)                                                          \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(h, PSMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e_));     \
  } while (0)
#define HIP_TRY(h, expr) HIP_TRY_AS(h, #expr, expr)
// alloc / reserve of an owning buffer: the message names the HIP call behind them as well
#define ALLOC_TRY(h, expr) HIP_TRY_AS(h, std::string(kAllocCall) + " in " #expr, expr)

#define NCCL_TRY(h, expr)                                                                  \
  do {                                                                                     \
    ncclResult_t e_ = (expr);                                                              \
    if (e_ != ncclSuccess)                                                                 \
      return fail(h, PSMF_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(e_));  \
  } while (0)

// The one dispatch on the storage type: f(T()) with T = double or float (the argument only carries the type: decltype(t)).
template <typename F>
auto by_storage(const psmf_filter* h, F&& f) { return h->cfg.storage == PSMF_F64 ? f(double()) : f(float()); }

// Completion waits by polling: hipStreamSynchronize / hipEventSynchronize fall back to an interrupt wait that, on this
// stack, now and then returns ~70 ms after the work is done (seen as wall time without matching event time).
hipError_t spin_stream(hipStream_t s) {
  hipError_t e;
  while ((e = hipStreamQuery(s)) == hipErrorNotReady) { __builtin_ia32_pause(); }
  return e;
}
hipError_t spin_event(hipEvent_t ev) {
  hipError_t e;
  while ((e = hipEventQuery(ev)) == hipErrorNotReady) { __builtin_ia32_pause(); }
  return e;
}

double host_now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

int set_device(psmf_handle h) {
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  return PSMF_OK;
}

int opt_in_lds(psmf_filter* h, const void* fn, size_t bytes) {
  HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return PSMF_OK;
}

}  // namespace

// The ONE place that decides which kernel advances the coefficient-space state of a block: launch_blk_filter switches on it
// and psmf_filter_kernel reports it (tests and bench.py quote that name as evidence of what ran).  Values = the codes of
// psmf_filter_kernel in include/psmf_hip.h.
enum FilterKernel { FK_STEP = 0, FK_GENERAL = 1, FK_FILTER2 = 2, FK_FILTER3 = 3, FK_FILTER3S = 4, FK_FILTER4 = 5, FK_FILTER4S = 6,
                    FK_FILTER5 = 7, FK_FILTER6 = 8, FK_FILTER6D = 9, FK_FILTER7 = 10, FK_PSTEP = 11 };

// what the entry points that a ring handle refuses say (psmf_capi.hip) and psmf_series_ring says of what it refuses (psmf_series.hip)
inline constexpr char kRingRefused[] = " is not available on a handle with a series ring (psmf_series_ring)";

constexpr int kSqErrorParts = 1024;      // workgroups of psmf_sq_error_k = partial sums that sq_error_sum reads back
constexpr int kGramWG = 128;             // workgroups of the exact Gram (psmf_step.hip) = partial Grams that alloc_common sizes gpart for

// ---- host functions that cross unit boundaries ----
// psmf_capi.hip: the C ABI
int run_steps(psmf_filter* h, int64_t k_begin, int64_t k_end);      // the steps of a checked psmf_run, read at k - sp.series_t0
int ensure_scratch(psmf_filter* h, size_t bytes);
void launch_prepare_k(psmf_filter* h, int64_t k);      // start of a run: the step counter, on the handle's stream
// psmf_step.hip: the launched per-step engine and the host driver of the persistent kernel
int init_step(psmf_filter* h);                          // psmf_create: LDS opt-ins, the persistent kernel's plan
int prepare_step(psmf_filter* h, int64_t k_begin);      // the per-step engine's part of a run's preparation
int run_step_engine(psmf_filter* h, int64_t k_begin, int64_t k_end);
int time_step_kernels(psmf_filter* h, int which, int iters, float* avg_us);
bool pstep_usable(const psmf_filter* h);
void destroy_graph(psmf_filter* h);
void print_pstep_prof(psmf_filter* h);
// psmf_comm.hip: the communicator
int all_reduce_sum(psmf_filter* h, double* buf, size_t count, hipStream_t s);
// psmf_rotation.hip: the noise rotation
int ensure_rot_tmp(psmf_filter* h, size_t bytes);
int rot_rows(psmf_filter* h, const void* src, void* dst, long long n, bool fwd);
int rot_rows_back_f64(psmf_filter* h, const double* src, double* dst, long long n);
int rot_dict(psmf_filter* h, const void* src, void* dst, bool fwd);
// psmf_series.hip: the series buffers (resident or a ring), their uploads, downloads and reductions
int ring_run(psmf_filter* h, int64_t k_begin, int64_t k_end);      // psmf_run on a ring handle
int sq_error_sum(psmf_filter* h, hipStream_t stream, int storage, const void* yp, const void* y, size_t n, double* part_d, double* acc);
// psmf_blocked.hip: the blocked engine
FilterKernel select_filter_kernel(const psmf_filter* h);
int init_blocked(psmf_filter* h);
void clear_block_abort_flag(psmf_filter* h);      // start of a run, on the handle's stream
int run_blocks(psmf_filter* h, int64_t k_begin, int64_t k_end);
int time_block_kernels(psmf_filter* h, int which, int iters, int nb, const DevState* saved_st, float* avg_us);
// psmf_filter34.hip: the filter3 family (FK_FILTER3, 3S, 4, 4S, 5)
int opt_in_lds_filter34(psmf_filter* h);
void launch_blk_filter34(FilterKernel fk, const psmf::BlockParams& b, hipStream_t stream);
