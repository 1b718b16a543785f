/*
 * psmf_hip.h -- C ABI of the MI355X (gfx950) PSMF / rPSMF filter library  (libpsmf_hip.so)
 *
 * The reference (alan-turing-institute/rPSMF) is pure Python and has no FFI layer; the
 * functions below are what a ctypes binding for its hot path binds instead of executing the
 * Python/numpy bodies cited next to each entry point (paths relative to the reference root).
 * Plain pointers and sizes only; no exceptions cross the boundary; every function returns
 * PSMF_OK (0) or a negative psmf_status, and psmf_last_error() gives the message.
 *
 * Conventions
 *   - the caller owns all host buffers; the library owns all device memory;
 *   - host matrices are row-major float64 unless a dtype argument says otherwise;
 *   - one handle = one filter (or one row-shard of a filter on one GPU); a handle is not
 *     thread-safe, independent handles may be used from different threads;
 *   - calls are asynchronous on the handle's HIP stream unless they return host data.
 */
#ifndef PSMF_HIP_H
#define PSMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSMF_ABI_VERSION 3
#define PSMF_RMAX 64 /* largest supported rank r */
#define PSMF_ROTATION_DMAX 32768 /* largest d of psmf_set_noise_rotation (the d x d eigenvector matrix stays resident) */

typedef enum {
  PSMF_OK = 0,
  PSMF_ERR_ARG = -1,         /* bad argument / shape / unsupported configuration           */
  PSMF_ERR_HIP = -2,         /* HIP runtime error                                          */
  PSMF_ERR_RCCL = -3,        /* RCCL error                                                 */
  PSMF_ERR_NUMERIC = -4,     /* singular r x r system (numpy.linalg.LinAlgError upstream)  */
  PSMF_ERR_STATE = -5,       /* call sequence error (e.g. run before set_state)            */
  PSMF_ERR_NO_DEVICE = -6    /* no HIP device visible                                      */
} psmf_status;

typedef enum { PSMF_F32 = 0, PSMF_F64 = 1 } psmf_dtype;

/* State transition f(theta, x, t); theta packs its blocks in the reference's order (BaseNonLinearity.dims).
 * PSMF_DYN_RANDOM_WALK  f = x                                   pypsmf/psmf/nonlinearities.py:42-56
 * PSMF_DYN_COS_PHASE    f = cos(2 pi theta t + x)               ExperimentSynthetic/synthetic_psmf.py:105-106   theta: [r]
 * PSMF_DYN_SCALED_WALK  f = A x (+ b)                           nonlinearities.py:59-78     theta: A [r*r], b [r] if dyn_flags & 1
 * PSMF_DYN_SINUSOID     f = [A] sin(2 pi b t + [c o] x)         nonlinearities.py:81-114    theta: A [r*r] if dyn_flags & 1 (scaled),
 *                                                                                           b [r], c [r] if dyn_flags & 2 (phased)
 * PSMF_DYN_FOURIER      f = sum_n A_n sin(2 pi b_n t + c_n o x) + D_n cos(2 pi e_n t + f_n o x)   nonlinearities.py:117-150
 *                                                               theta: A_1, D_1, .., A_N, D_N [r*r each], then b_n, c_n, e_n, f_n [r each]
 *                                                               per n; N = dyn_terms <= 4
 * PSMF_DYN_HOST         any callable: the host evaluates mu_bar = f(theta, mu, k) and P_bar = F P F^T + Q (r-sized) and
 *                       advances the device one timestep at a time with psmf_step_host (the d-sized work stays on the device)
 * Kinds 0-4 are evaluated inside the device time loop of either engine, with analytic Jacobians df/dx, df/dtheta (the reference
 * uses autograd, psmf.py:41-44): the blocked engine (r <= 32) or the serial stage of the per-step engine's launched form (r > 32,
 * a non-uniform R, a masked handle, engine = 1; the persistent per-step kernel takes kinds 0, 1).  Kind 5 is the per-step engine's.
 * A masked handle created with masked = PSMF_MASKED_DYNAMICS takes kinds 0-4, each with its own n_theta; kind 5 is refused there, and
 * masked = 1 / 2 / 3 take kind 0 only. */
typedef enum { PSMF_DYN_RANDOM_WALK = 0, PSMF_DYN_COS_PHASE = 1, PSMF_DYN_SCALED_WALK = 2, PSMF_DYN_SINUSOID = 3,
               PSMF_DYN_FOURIER = 4, PSMF_DYN_HOST = 5 } psmf_dyn_kind;

typedef struct psmf_filter* psmf_handle;

/* psmf_config.masked: 1 = the masked PSMF / rPSMF filter of ExperimentImpute (a random walk), 2 = MLE-SMF, 3 = TMF, and */
#define PSMF_MASKED_DYNAMICS 4 /* the masked PSMF / rPSMF filter with any device-evaluated f_theta (see the field) */

/* Mode table: which hook configuration of PSMFIter / rPSMFIter runs fused. */
typedef struct {
  int32_t abi_version;   /* PSMF_ABI_VERSION                                                  */
  int32_t d;             /* global number of rows of C (= len(y_k))                           */
  int32_t r;             /* rank, 1..PSMF_RMAX                                                */
  int32_t row0;          /* first global row held by this handle (row sharding)               */
  int32_t d_local;       /* rows held by this handle (== d when not sharded)                  */
  int32_t robust;        /* 0: PSMFIter  psmf.py:90-180;  1: rPSMFIter  rpsmf.py:116-184      */
  int32_t coef_update;   /* 1: Kalman update of (mu, P) psmf.py:140-165; 0: mu_k = mu_bar,
                            P_k = P_bar  (synthetic_psmf.py:89-98)                            */
  int32_t eta_full;      /* 1: eta = tr(R + C Pbar C^T)/d  psmf.py:121-125; 0: tr(R)/d        */
  int32_t pbar_predict;  /* 1: Pbar = F P F^T + Q  psmf.py:107-115; 0: Pbar = P_{k-1}         */
  int32_t fixed_lambda;  /* rpsmf.py:36-40                                                    */
  int32_t dyn_kind;      /* psmf_dyn_kind                                                     */
  int32_t n_theta;       /* length of theta: 0 random walk / host, r cos-phase, see psmf_dyn_kind       */
  int32_t storage;       /* psmf_dtype of C, y, y_pred in HBM (arithmetic on r x r is f64)    */
  int32_t store_y_pred;  /* keep y_hat_k = C_{k-1} mu_bar_k for every step (psmf.py:93)       */
  int32_t recursive;     /* 1: PSMFRecursive -- Adam step on theta inside the time loop every
                            `update_every` steps (psmf.py:287-304); 2: the same with plain SGD
                            (psmf.py:244-248; learning rate = adam_lr / its schedule).  0, 1 and 2 are accepted on a
                            masked = PSMF_MASKED_DYNAMICS handle too (theta, its gradient sum and the moments are replicated over row shards);
                            refused with PSMF_DYN_HOST, which keeps theta on the host            */
  int32_t update_every;
  int32_t gram_refresh;  /* recompute G = C^T C exactly every this many steps (0 = only at
                            set_state); between refreshes G is updated algebraically           */
  int32_t device;        /* HIP device ordinal                                                */
  int32_t use_graph;     /* 1: replay the per-step launches from a hipGraph                   */
  int32_t n_workgroups;  /* row-sweep workgroups, 0 = auto                                    */
  int32_t engine;        /* 0 = auto, 1 = per-step engine (one row sweep per timestep),
                            2 = exact time-blocked engine (one Gram Z^T Z per block of min(64 - r, 48) steps,
                            the steps in coefficient space; needs r <= 32)                      */
  int32_t dyn_flags;     /* see psmf_dyn_kind                                                  */
  int32_t dyn_terms;     /* PSMF_DYN_FOURIER: N                                                */
  int32_t nonuniform_R;  /* 1: R = rho * diag(rho_rows) with per-row values uploaded by psmf_set_row_noise
                            (psmf.py:140-153 takes any diagonal R); per-step engine, weighted Gram every step.  With masked =
                            1 / 2: the masked filters' diagonal R read row by row (ExperimentImpute/PSMF.py:70-72, rPSMF.py:91-98,
                            MLESMF.py:70-76), weights m_i / (rho rho_i + s) (MLE-SMF: m_i / (rho rho_i)) -- one masked weighted
                            Gram pass more per step; not with masked = 3 (TMF ignores R) */
  int32_t masked;        /* 1: every step has a 0/1 observation mask over the rows (psmf_upload_mask): the masked filter of
                            ExperimentImpute/PSMF.py:59-84, rPSMF.py:75-135 -- e = m o (y - y_hat), rows with m_i = 0 not
                            updated, Gram / innovation covariance over the observed rows only, eta and lambda with d (not the
                            observed count), y_hat stored unmasked.  Per-step engine, one masked Gram pass per step; needs the
                            full filter (coef_update, eta_full, pbar_predict = 1) and store_y_pred = 1; R = rho I, or any
                            diagonal R with nonuniform_R = 1 (masked = 1 / 2; psmf_set_row_noise before the first run).
                            masked = 1 is a random-walk filter (Pbar = P + Q, PSMF.py:65-66) and refuses every other dyn_kind.
                            Dynamics: masked = 4 (PSMF_MASKED_DYNAMICS) is the step of masked = 1 with every device-evaluated
                            f_theta (dyn_kind 0-4: mu_bar = f_theta(mu, k), Pbar = F P F^T + Q inside the time loop), robust = 0
                            or 1 and recursive = 0, 1 or 2, on row shards and on the series ring; psmf_predict rolls out with
                            f_theta; with dyn_kind 0 it is masked = 1, bit for bit, and takes a row noise the same way.  The theta gradient of a masked step is
                            that of the masked incremental likelihood 1/2 sum_i log(s m_i + eta) + 1/2 e^T e / (s + eta)
                            (psmf.py:264-270, rpsmf.py:196-200; the Gaussian form for robust = 1 too):
                            g_f = n_obs w / N - h / N - ee w / N^2 with n_obs = sum_i m_i of the step; a step without any
                            observation adds exactly zero.  Refused, each by name: dynamics with masked = 1; PSMF_DYN_HOST on a masked handle (the host
                            would need the masked g_f); nonuniform_R = 1 together with n_theta > 0 (the Gram's count slot then
                            carries sum m_i rho_i, so n_obs is not on the device); masked = 2 / 3 with any dynamics; R_k / Q_k
                            schedules (psmf_set_schedules, psmf_set_q_matrix_schedule).
                            2 / 3: the baseline filters that share these contractions -- 2 = MLE-SMF (MLESMF.py:57-88: weights m_i / rho,
                            C += gam / eta (m o e) x_p^T, bands -+ sig sqrt(eta)), 3 = TMF (TMF.py:47-66: Pbar = I / nu with Q = I / nu and
                            P = 0 from the caller, kappa = 1, C += gam (m o e) x_p^T); gam from psmf_set_step_size */
  double alpha, beta;    /* rPSMF scaling factors (rpsmf.py:45-51), 1.0 unless use_scaling     */
  double adam_lr, adam_lr_end, adam_lr_steps; /* lr (Constant) or lr_start/lr_end/steps
                            (ExponentialLearningRate, learning_rate.py:20-27; steps = 0 ->
                            constant), used when recursive = 1                                 */
  double adam_b1, adam_b2;
} psmf_config;

/* ---- lifetime -------------------------------------------------------------------------- */
/* replaces PSMFIter.__init__ / rPSMFIter.__init__  (psmf.py:18-46, rpsmf.py:12-51) */
int psmf_create(psmf_handle* out, const psmf_config* cfg);
void psmf_destroy(psmf_handle h);
const char* psmf_last_error(psmf_handle h);
/* SHA-256 (hex) of the sources and compiler flags this library was built from (rpsmf_amd/build.py compares it with the sources on
 * disk: a stale binary is rebuilt, never silently used).  (New: the reference is interpreted Python.) */
const char* psmf_build_id(void); /* h may be NULL: error of the last failed create */
int psmf_device_count(void);

/* ---- state ----------------------------------------------------------------------------- */
/* Any pointer may be NULL = leave that part unchanged.  C: d_local x r;  V, P, Q: r x r;
 * mu: r; theta: n_theta.  rho = diag(R) (uniform), lambda0 = Student-t dof (rPSMF).
 * Pass a NaN for rho / lambda0 to leave them unchanged.
 * replaces step_reset (psmf.py:75-83, rpsmf.py:106-114) and the constructors' state. */
int psmf_set_state(psmf_handle h, const double* C, const double* V, const double* P,
                   const double* Q, const double* mu, double rho, double lambda0,
                   const double* theta);
int psmf_zero_gradsum(psmf_handle h);
/* scalars[8] = { rho_k, lambda_k, s, eta, N, phi, omega, step_counter } of the last step. */
int psmf_get_state(psmf_handle h, double* C, double* V, double* P, double* Q, double* mu,
                   double* theta, double* gradsum, double* scalars);
/* Adam moments for the recursive mode (psmf.py:190-204): m, v of length n_theta. */
int psmf_set_adam(psmf_handle h, const double* m, const double* v);

/* Per-step schedules of PSMFIter's R[k], Q[k] (psmf.py:115,123,141): R_k = rho_k[k] I and Q_k = q_k[k] * Q for the 1-based
 * step k = 1 .. n - 1 (entry 0 unused; steps beyond n - 1 are refused by psmf_run).  NULL = constant (rho / Q of
 * psmf_set_state).  Not with robust = 1 (rPSMF runs on its own omega-scaled Q_{k-1}, R_{k-1}, rpsmf.py:123,128,141). */
int psmf_set_schedules(psmf_handle h, const double* rho_k, const double* q_k, int64_t n);
/* PSMFIter's Q[k] when it is NOT a scalar multiple of Q[1] (psmf.py:115 reads a matrix per step): n matrices of r x r doubles,
 * row-major, matrix k for the 1-based step k (matrix 0 unused; steps beyond n - 1 are refused by psmf_run).  P_bar_k =
 * F P F^T + Q_k is then formed from the uploaded matrix in the serial stage of the per-step engine (launched form; the handle
 * must have been created with engine = 1).  NULL or n = 0 drops the schedule.  Not with robust = 1, masked handles or
 * PSMF_DYN_HOST. */
int psmf_set_q_matrix_schedule(psmf_handle h, const double* Q_k, int64_t n);

/* Non-uniform diagonal R (cfg.nonuniform_R = 1): rho_rows[d_local] = diag(R) of this handle's rows, rho_mean = sum of diag(R)
 * over ALL rows / d (tr(R) / d of psmf.py:121-125; the same value on every shard).  The `rho` of psmf_set_state is then the
 * scalar in front (1 to start with; rPSMF multiplies it by omega_k, rpsmf.py:169).  Masked handles (masked = 1 / 2) take it the
 * same way: eta of a step is then (rho sum_i m_i rho_i + <G_m, Pbar>) / d, the reference's trace(M R M + C_M Pbar C_M^T) / d. */
int psmf_set_row_noise(psmf_handle h, const double* rho_rows, double rho_mean);

/* A NON-DIAGONAL R (the dense d x d branch of psmf.py:150-152, rpsmf.py:150-152), cfg.nonuniform_R = 1, one shard (d_local = d):
 * R = U diag(lam) U^T with U (d x d, row-major, eigenvectors in its COLUMNS, orthonormal) and lam[d] >= 0 from the caller's
 * symmetric eigen-solver (LAPACK dsyevd / numpy.linalg.eigh; O(d^3), once).  The recursion is equivariant under the orthogonal
 * change of observation coordinates y -> U^T y, C -> U^T C (eta and the residual norms are invariant), so the handle keeps the
 * series and the dictionary ROTATED, runs the non-uniform-diagonal step with rho_rows = lam, and rotates at its boundary:
 * psmf_set_state / psmf_upload_series on the way in, psmf_get_state's C, psmf_download_y_pred, psmf_predict, psmf_project on the
 * way out (float64 GEMMs against the resident U on the matrix cores) -- callers see original coordinates everywhere; no d x d
 * inverse is formed and a step stays O(d r^2).  Call it before the first psmf_set_state / psmf_upload_series.  U stays resident:
 * 8 d^2 bytes, d <= PSMF_ROTATION_DMAX (PSMF_ERR_ARG beyond).  Orthonormality of U is checked over the whole matrix in O(d^2)
 * (U^T U z = z for two sign vectors z): PSMF_ERR_ARG if it fails.  Not on a masked handle: the mask selects rows of the original
 * coordinates and is not equivariant under the rotation (PSMF_ERR_STATE). */
int psmf_set_noise_rotation(psmf_handle h, const double* U, const double* lam);

/* ---- series ---------------------------------------------------------------------------- */
/* Y: nt x d_local time-major block holding y_{t0+1} .. y_{t0+nt}; T_total sizes the device
 * buffers on first use (a ring handle, psmf_series_ring below: one chunk per call, T_total ignored).  replaces the dict y[k] of (d,1) arrays passed to step (psmf.py:85-88) */
int psmf_upload_series(psmf_handle h, const void* Y, int dtype, int64_t t0, int64_t nt,
                       int64_t T_total);

/* masked = 1: M: nt x d_local uint8, time-major like Y, 1 = observed, for the steps t0+1 .. t0+nt (after psmf_upload_series, which
 * sizes the buffer).  Where M = 0 the value of Y is never read.  replaces Mk = diag(M[:, t]) of ExperimentImpute/PSMF.py:62.
 * A resident (non-ring) handle takes the mask in order: the rows may arrive in pieces, each piece starting at or before the end
 * of what has been uploaded so far (rows behind a gap do not count), and psmf_run refuses with PSMF_ERR_ARG a step range that ends
 * beyond the rows uploaded so (the buffer is not cleared when it is allocated).  The masked Gram is formed one step ahead; rows
 * uploaded after a run that stopped in front of them are taken up by the next run, which then prepares again. */
int psmf_upload_mask(psmf_handle h, const uint8_t* M, int64_t t0, int64_t nt);

/* ---- series ring: a stream longer than the device buffers (or of unknown length) --------
 * psmf_series_ring makes the series buffers of the handle -- Y, y_hat, the posterior-mean history and, masked handles, the mask
 * and the (s, eta) history -- a ring of n_slots windows of `chunk` rows instead of T_total resident rows.  Call it before the
 * first psmf_upload_series (PSMF_ERR_STATE after one); chunk >= 1, n_slots >= 2.  Row t of the stream (0-based; step k = t + 1)
 * belongs to chunk t / chunk, and a chunk lives in slot (t / chunk) % n_slots at row offset t % chunk: uploading chunk c evicts
 * chunk c - n_slots.  On a ring handle
 *   psmf_upload_series / psmf_upload_mask  take rows of ONE chunk per call (PSMF_ERR_ARG across a chunk boundary; the rows of a
 *       chunk in order; the last chunk of a stream may be short; the mask after the series rows it belongs to); T_total is
 *       ignored.  The copy runs on a copy stream of the handle behind the last run that touched the slot's previous occupant, and
 *       does not synchronise the compute stream: a chunk is uploaded while another one runs.  The call returns when the caller's
 *       array has been read.  An array whose dtype differs from the storage type is converted on the device (psmf_cast_rows),
 *       in a staging buffer of one chunk of float64 that the first such upload or download allocates.
 *   psmf_run  may span chunks; it is cut at the chunk boundaries, waits (on the device) for the uploads of the slots it reads, and
 *       goes on across a boundary exactly as between two psmf_run calls on a resident handle cut at the same steps -- the same
 *       bits.  A step that is not resident is PSMF_ERR_STATE, names the step, and nothing of the call is launched.
 *       Masked handles form the Gram of the NEXT step beside each step: for the same bits across a boundary the first mask row of
 *       the next chunk has to be uploaded before the run that ends the chunk is called (with n_slots >= 3 that still overlaps);
 *       otherwise the run re-prepares at the boundary like a fresh psmf_run.
 *   psmf_download_y_pred, psmf_download_mu, psmf_sq_error, psmf_masked_metrics, psmf_download_step_scalars  take ranges in chunks
 *       that are still resident (PSMF_ERR_STATE: "step k is no longer resident"), wait for the runs of those slots only, and do
 *       not report a numeric failure of the run: psmf_sync does.  Row k of the mean history is kept with the chunk of step k;
 *       the row a chunk starts from is the last row of its predecessor's slot and is rewritten when that slot is run again.
 *       psmf_masked_metrics alone also waits for the compute stream: its second sum reads C, which every queued run rewrites,
 *       so "the present C" is the C behind every run queued before the call, as on a resident handle.
 *   psmf_set_schedules, psmf_set_q_matrix_schedule (indexed by step, not windowed), psmf_set_noise_rotation (its rotation would
 *       have to run on the copy stream), psmf_time_kernel and PSMF_DYN_HOST handles are refused by name, PSMF_ERR_STATE.
 * psmf_predict, psmf_predict_sq_error, psmf_project, psmf_get_state do not read the series and are unchanged.  Without this call a
 * handle behaves as before.  (New: the reference's step() consumes a dict of observations one by one, psmf.py:85-88, and holds
 * nothing on a device.) */
int psmf_series_ring(psmf_handle h, int64_t chunk, int n_slots);
/* Read-only (tests): out[0] = chunk, out[1] = n_slots (both 0 without a ring), out[2 + i] = the chunk slot i holds or -1;
 * out has room for 2 + n_slots values. */
int psmf_series_ring_info(psmf_handle h, int64_t* out);

/* ---- the hot loop ---------------------------------------------------------------------- */
/* for k in k_begin+1 .. k_end: inner(k, y_k)  entirely on the device
 * replaces PSMFIter.step / inner and its ten hooks (psmf.py:85-180), rPSMFIter overrides
 * (rpsmf.py:116-184), PSMFRecursive.inner (psmf.py:287-304). Asynchronous. */
int psmf_run(psmf_handle h, int64_t k_begin, int64_t k_end);
int psmf_sync(psmf_handle h); /* waits, then reports a device-side numeric failure if any */

/* Host-stepped dynamics (dyn_kind = PSMF_DYN_HOST): ONE timestep, k -> k + 1 (k = number of finished steps), with
 * mu_bar = f(theta, mu_k, k + 1) [r] and P_bar = F P_k F^T + Q [r x r] formed by the caller (psmf.py:104-115); the device
 * does everything d-sized of inner() (psmf.py:90-102).  Returns what the caller needs for the next step and for the
 * theta gradient: mu_{k+1} [r], g_f = d(incremental likelihood)/df [r] (gradsum += J_theta^T g_f, psmf.py:167-177),
 * P_{k+1}, Q_{k+1} [r x r] (rPSMF scales Q by omega).  Any output may be NULL.  Synchronous. */
int psmf_step_host(psmf_handle h, int64_t k, const double* mu_bar, const double* P_bar, double* mu_out, double* gf_out,
                   double* P_out, double* Q_out);
/* out[q] = C mu[q] for n given r-vectors (n x d_local float64): the y_hat of a roll-out the caller computed (psmf.py:182-188). */
int psmf_project(psmf_handle h, const double* mu, int64_t n, double* out);

/* y_hat for steps t0+1..t0+nt (needs store_y_pred) -> out (nt x d_local), dtype f32/f64 */
int psmf_download_y_pred(psmf_handle h, void* out, int dtype, int64_t t0, int64_t nt);
/* posterior means mu_{k0} .. mu_{k0+nk-1} of the last run (row k = state after step k; the row of the
 * run's first step index holds the mean it started from) -> out (nk x r float64).  What TrackingMixin
 * reads as `_mu[k]` (tracking.py:140-142) when the experiment keeps `_mu` un-pruned. */
int psmf_download_mu(psmf_handle h, double* out, int64_t k0, int64_t nk);
/* psmf.py:182-188: mu rolled forward n_pred steps from the current state, y_hat = C mu_pred;
 * out: n_pred x d_local float64.  T = index of the last filtered step. */
int psmf_predict(psmf_handle h, int64_t T, int64_t n_pred, double* out);
/* sum_t sum_i (y_hat - y)^2 over steps t0+1..t0+nt of the uploaded series (local rows);
 * tracking.py:63-76 error norms without copying y_pred back. */
int psmf_sq_error(psmf_handle h, int64_t t0, int64_t nt, double* out);
/* the same for the roll-out window: sum over q < n_pred and the local rows of (C mu_pred_q - Y_true[q])^2, Y_true the held-out
 * observations y_{T+1} .. y_{T+n_pred} (n_pred x d_local float64, host): tracking.py:74-76 (`_E_pred`). */
int psmf_predict_sq_error(psmf_handle h, int64_t T, int64_t n_pred, const double* Y_true, double* out);

/* masked = 2 / 3: the step size gam of the stochastic-gradient update of C for the runs that follow (the experiments use
 * 1e-6 / (pass + 1)^0.7, MLESMF.py:59-60, TMF.py:46-48). */
int psmf_set_step_size(psmf_handle h, double gam);
/* masked != 0, after psmf_run over the steps t0+1 .. t0+nt: the evaluation sums of ExperimentImpute over the held-out entries
 * Mmiss (nt x d_local uint8, 1 = artificially removed) of this handle's rows, reduced on the device:
 *   out4[0] = sum (y_hat - y)^2          RMSEM(Yrec, YorgInt, Mmiss)^2 * out4[3]            PSMF.py:88, common.py:79-84
 *   out4[1] = sum (c_i . x_t - y)^2      RMSEM(C @ X, ...) with the present C, x_t = posterior mean of step t   PSMF.py:86-89
 *   out4[2] = entries strictly inside y_hat -+ sig sqrt(N_t) (PSMF.py:83-84) resp. sig sqrt(s_t m_i + eta_t) (rPSMF.py:121-123)
 *   out4[3] = number of held-out entries                                                     common.py:87-94
 * (row-sharded filter: the caller adds the four sums over the shards).  y = the uploaded series (YorgInt). */
int psmf_masked_metrics(psmf_handle h, const uint8_t* Mmiss, int64_t t0, int64_t nt, double sig, double* out4);
/* masked = 1: (s_t, eta_t) of the steps t0+1 .. t0+nt -> out (nt x 2 float64): what the bands YrecL / YrecH are formed from. */
int psmf_download_step_scalars(psmf_handle h, double* out, int64_t t0, int64_t nt);

/* ---- multi-GPU (row shards, one process per GPU, RCCL over xGMI) ------------------------- */
#define PSMF_UNIQUE_ID_BYTES 128
int psmf_comm_unique_id(void* id_out /* PSMF_UNIQUE_ID_BYTES */);
int psmf_comm_init(psmf_handle h, int nranks, int rank, const void* unique_id);
/* Give up the handle's RCCL communicator WITHOUT waiting for its peers (ncclCommAbort; psmf_destroy calls ncclCommDestroy, which
 * may block when a peer never joined): for the failure path of a multi-rank start.  The handle is a single shard again afterwards.
 * (New; the reference is single-process.) */
int psmf_comm_abort(psmf_handle h);

/* Host-mediated communicator instead of RCCL: wherever a sharded engine needs its sum-all-reduce (per-step engine: r + 1
 * float64 per timestep; blocked engine: one 64 x 64 Gram per run and one 128 x 64 cross-Gram per block) the library copies
 * the message to the host and calls fn(ctx, buf, count), which must replace buf[0..count) by its sum over all ranks -- same
 * rank order on every rank, so that the replicated r x r state stays bit-identical -- and return 0.  For transports
 * the caller owns (MPI, gloo) and for exercising the sharded arithmetic with several shards on ONE GPU (tests).  Each call
 * synchronises the stream it sits on: correct, not fast.  (New: the reference is single-process, pypsmf/psmf/psmf.py:85-88.) */
typedef int (*psmf_allreduce_fn)(void* ctx, double* buf, int64_t count);
int psmf_comm_init_host(psmf_handle h, int nranks, int rank, psmf_allreduce_fn fn, void* ctx);

/* What the handle's communicator is: out4[0] = 0 none, 1 RCCL, 2 host-mediated; out4[1] = number of ranks, out4[2] = this rank,
 * out4[3] = HIP device -- for an RCCL communicator as RCCL itself reports them (ncclCommCount, ncclCommUserRank, ncclCommCuDevice),
 * so that a benchmark line can state how many ranks the exchange really spanned.  (New; the reference is single-process.) */
int psmf_comm_info(psmf_handle h, int32_t* out4);
/* PCI bus id ("0000:c1:00.0") of HIP device `device` into buf (len >= 16): which physical GPU a rank drives. */
int psmf_device_pci_bus_id(int device, char* buf, int len);

/* ---- measurement ------------------------------------------------------------------------ */
/* psmf_run bracketed by HIP events on the handle's stream; *ms = elapsed milliseconds. */
int psmf_run_timed(psmf_handle h, int64_t k_begin, int64_t k_end, float* ms);
/* average duration (microseconds) of `iters` back-to-back launches of one kernel of the step
 * on the handle's stream, HIP-event timed: which = 0 row sweep (+ concurrent r x r solve),
 * 1 = serial r x r stage.  Blocked engine: 0 = coefficient-space filter of one full block,
 * 1 = cross-Gram of the next block (+ reduction), 2 = apply.  State is saved and restored around the measurement: C, the
 * r x r state and its scalars, theta with its gradient sum and optimiser moments, and the y_hat rows and posterior means that
 * the measured kernels record for the first steps of the series (they run there whatever the handle has filtered so far). */
int psmf_time_kernel(psmf_handle h, int which, int iters, float* avg_us);
/* geometry actually used: out[0] = sweep workgroups, out[1] = rows per workgroup,
 * out[2] = padded row length (elements), out[3] = lanes per row, out[4] = graph chunk steps,
 * out[5] = engine in use (1 per-step, 2 blocked), out[6] = steps per block (blocked engine) */
int psmf_geometry(psmf_handle h, int32_t* out7);
/* Which kernel advances the r x r / coefficient-space state with the handle's present configuration (mode flags, dynamics, the Q
 * last uploaded, schedules, switches): 0 = per-step engine (psmf_sweep_solve + psmf_serial), 1 = psmf_blk_filter (general blocked
 * kernel), 2 = psmf_blk_filter2, 3 = psmf_blk_filter3, 4 = psmf_blk_filter3s, 5 = psmf_blk_filter4, 6 = psmf_blk_filter4s, 7 = psmf_blk_filter5,
 * 8 = psmf_blk_filter6 (every configuration at r <= 16 but the simplified hooks), 9 = psmf_blk_filter6d (its instantiation with the two
 * inversions side by side: random walk, Q = q I), 10 = psmf_blk_filter7 (the same design on 2 x 2 tiles: what is left at 17 <= r <= 32),
 * 11 = psmf_pstep_k, the per-step engine as ONE persistent launch per run (C on chip, device-flag hand-offs; psmf_pstep.hip).
 * The same function decides what is launched (select_filter_kernel, psmf_blocked.hip).
 * (New: diagnostics for tests and bench.py -- the reference has one code path, pypsmf/psmf/psmf.py:90-102.) */
int psmf_filter_kernel(psmf_handle h);
/* The persistent per-step kernel's launch geometry for this handle (read-only): out5[0] = 1 if the handle's next run goes through
 * psmf_pstep_k (the same function decides that at launch), out5[1] = row workgroups (the grid has one more: the hub),
 * out5[2] = rows per row workgroup, out5[3] = row passes NP of the kernel instance (4, 8, 12; 16 at 33 <= r <= 48),
 * out5[4] = compute units of the device.  out5[1..3] are 0 where the planner found no geometry at psmf_create.
 * The planner takes r <= 48 (masked handles r <= 32) and d_local rows in 2048 / RPAD-row passes, RPAD = 8, 16, 32, 64 the padded
 * rank: at most n_cu - 1 row workgroups of 12 passes (16 at RPAD = 64), and no more of them than the hub's fan-in sums -- 17 per
 * segment, min(24, 256 / ceil((r + 1) / 2)) segments (RPAD = 64: 20 per segment, at most 12 segments).  On 256 compute units:
 * d_local <= 783 360 / 391 680 / 195 840 at RPAD = 8 / 16 / 32; 122 880 at 33 <= r <= 41, 112 640 at r <= 45, 102 400 at
 * r <= 48.  Every d_local below the bound has a geometry (the smallest NP whose workgroups fit both counts).
 * (New: diagnostics for tests -- the reference has one code path, pypsmf/psmf/psmf.py:90-102.) */
int psmf_step_plan(psmf_handle h, int32_t* out5);
/* diagnostics of the blocked engine's r x r inversions since the last reset: out[0] = timesteps inverted by
 * Newton-Schulz refinement, out[1] = by the direct symmetric sweep, out[2] = Newton-Schulz iterations in
 * total, out[3] = failed Newton-Schulz attempts, out[4] / out[5] = summed in-kernel durations / gaps between
 * consecutive filter kernels in 10 ns ticks, out[7] = filter launches; reset != 0 clears them.  (New: the reference has no
 * counterpart; its np.linalg.inv calls are pypsmf/psmf/psmf.py:147-149.) */
int psmf_counters(psmf_handle h, int64_t* out8, int reset);
/* Blocked engine with chained blocks (one launch of the coefficient-space filter kernel per psmf_run): number of such
 * launches completed since the last reset and the sum of their durations, measured with HIP events recorded around each
 * launch on the stream it runs on (at most 256 runs between two psmf_sync calls are timed).  Waits like psmf_sync.
 * (New: measurement aid for bench.py; the reference times whole runs with time.time(), ExperimentImpute/PSMF.py:59,91.) */
int psmf_filter_kernel_time(psmf_handle h, int64_t* launches, double* total_ms, int reset);

/* Measured HBM bandwidth of a plain streaming copy (`bytes` read + `bytes` written per launch, `iters` launches, HIP events):
 * the "measured copy-kernel peak" SURVEY 8(d) asks for beside the nominal 8 TB/s.  *gbps = (read + written bytes) / time. */
int psmf_measure_copy_bandwidth(int device, size_t bytes, int iters, double* gbps);

/* ================= masked, batched small-d filter (ExperimentImpute) ==================== */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;       /* Y is d x n, C d x r, X r x n (reference layout)                  */
  int32_t batch;         /* independent replicas (seeds): own mask, C0, X0                    */
  int32_t method;        /* 0: PSMF.py:40-95   1: rPSMF.py:40-148   2: MLE-SMF, MLESMF.py:40-92 (V unused)
                          * 3: TMF, TMF.py:30-73 (V, P, Q, rho unused; nu = 2; no bands, inside = 0)        */
  int32_t n_iter;        /* passes over the n columns (Iter)                                  */
  int32_t device;
  int32_t want_bands;    /* also return Yrec, YrecL, YrecH                                    */
  double sig;            /* band half-width in standard deviations                             */
  double lambda0;
} psmf_impute_config;

/* Any d and 1 <= r <= PSMF_RMAX.  Shapes whose replica state fits one workgroup's LDS (d <= 512, r <= 16) run one workgroup per
 * replica, all replicas in one launch (psmf_impute_kernel3 / psmf_impute_kernel2); larger shapes run the replicas one after the
 * other on the masked per-step engine of the large-d handle (all four methods).  psmf_impute_kernel_id() tells which.
 * All arrays time-major (column t of the reference's d x n matrices is row t here):
 *   YorgInt  n x d  float64  data with native missing values set to 0        (shared)
 *   M        batch x n x d  uint8   1 = observed                              (per replica)
 *   Mmiss    batch x n x d  uint8   1 = artificially removed (evaluation set)
 *   C        batch x d x r  float64 in: C0   out: final C
 *   X        batch x n x r  float64 in: X0   out: final X (the reference mutates X in place)
 *   V, P, Q  r x r float64 (shared initial values);  rho = uniform diag(R) (R = rho I; a diagonal R with unequal entries:
 *            psmf_impute_run_rows below)
 *   Epred, Efull  batch x n_iter  (RMSE after each pass, PSMF.py:88-89)
 *   inside        batch           (coverage, common.py:87-94)
 *   Yrec, YrecL, YrecH  batch x n x d float64 or NULL
 *   status        batch int32 or NULL: per-replica outcome, PSMF_OK or PSMF_ERR_NUMERIC (r x r system lost positive definiteness,
 *                 or non-finite errors).  A failed replica gets NaN in Epred / Efull / inside, the others are unaffected and the
 *                 call returns PSMF_OK -- the reference records NaN for a diverged repeat and carries on (rPSMF.py:236-243).
 *                 With status = NULL a failed replica fails the call (PSMF_ERR_NUMERIC).
 * replaces ProbabilisticSequentialMatrixFactorizer / robust_PSMF (and, method 2 / 3, the baseline filters
 * stochasticGradientStateSpaceMF / temporalRegularizedMF that share their masked contractions) and the RMSEM /
 * compute_number_inside_bars calls made on their outputs. */
int psmf_impute_run(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                    const uint8_t* Mmiss, double* C, double* X, const double* V,
                    const double* P, const double* Q, double rho, double* Epred, double* Efull,
                    double* inside, double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms);
/* psmf_impute_run with per-row observation noise: R = diag(rho_rows), d values >= 0 shared by the replicas -- the reference's masked
 * filters read np.diag(R) row by row (ExperimentImpute/PSMF.py:70-72, rPSMF.py:91-98, MLESMF.py:70-76); rPSMF's R = omega R
 * (rPSMF.py:134) scales all of them.  Every other argument as in psmf_impute_run.  Entries all equal, and method 3 (TMF ignores R),
 * run psmf_impute_run's own kernels with rho = rho_rows[0] (the same bits).  Unequal entries run the row-noise instances of the
 * one-workgroup kernels (psmf_impute_kernel3w<NG>, psmf_impute_kernel2w), i.e. the shapes psmf_impute_kernel_id answers with 2 or
 * 300 + NG: d <= 512, r <= 16.  On a shape it answers with 4 (the masked per-step engine of the large-d handle, which carries one
 * scalar rho) unequal entries are PSMF_ERR_ARG; so is an entry that is negative or not finite. */
int psmf_impute_run_rows(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                         const uint8_t* Mmiss, double* C, double* X, const double* V,
                         const double* P, const double* Q, const double* rho_rows, double* Epred, double* Efull,
                         double* inside, double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms);
/* Which column loop psmf_impute_run uses for cfg->d, cfg->r (with the present environment switches): 1 = round 1's loop,
 * 2 = psmf_impute_kernel2, 300 + NG = psmf_impute_kernel3<NG> (d <= 80, r <= 14; NG = 4-row groups: 3, 5, 8, 12, 20),
 * 4 = masked per-step engine of the large-d handle.  Negative = error.  (Diagnostics; the reference has one code path.) */
int psmf_impute_kernel_id(const psmf_impute_config* cfg);

/* ================= batched PSMF with linear-Gaussian dynamics and an observation map (ExperimentChange) ==================== */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;       /* Y is d x n, C d x r (reference layout)                                          */
  int32_t p;             /* dimension of the latent state, r <= p <= 32: A, Q, P are p x p, H is r x p      */
  int32_t batch;         /* independent series (replicas): own Y, C, V, x, P                                 */
  int32_t device;
  int32_t carry_P;       /* 1: P_prev = P_{t-1} (the textbook recursion).  0: PSMF.m:30 as written -- P_prev = P0 at the first
                          * step of a series, 0 at every later step                                          */
  int32_t first_step;    /* 1: the call starts a series.  0: it continues one (x, P, C, V of the previous call); with
                          * carry_P = 0 every step of such a call uses P_prev = 0                            */
  int32_t want_pred;     /* also return Ypred                                                                */
} psmf_ssm_config;

/* The filter of ExperimentChange/PSMF.m:6-45 for a batch of independent series, float64 throughout, one workgroup per replica and
 * all replicas in one launch.  Per step: xbar = A x, Pbar = A P_prev A^T + Q, z = H xbar, w = V z, s = z^T w, yhat = C z,
 * e = y - yhat, P_z = H Pbar H^T, S = C P_z C^T + (rho + s) I, x = xbar + Pbar H^T C^T S^-1 e,
 * P = Pbar - Pbar H^T C^T S^-1 C H Pbar, eta = trace(C P_z C^T + rho I) / d, N = s + eta, C += e w^T / N, V -= w w^T / N
 * (S is never formed: two symmetric r x r inversions).  Limits: 1 <= d <= 512, 1 <= r <= 16, r <= p <= 32; anything else is
 * PSMF_ERR_ARG and the message names the limit.  All arrays row-major, time-major where there is a time axis:
 *   Y        batch x n x d              (row t = y_t)
 *   C        batch x d x r   in: C0     out: final C
 *   V        batch x r x r   in / out
 *   x        batch x p       in: x_0    out: x_n
 *   P        batch x p x p   in: P0 (read at the first step of a series, and at every call with carry_P = 1)   out: P_n
 *   A, Q     p x p, H r x p  shared by the replicas; Q symmetric positive definite (PSMF_ERR_ARG otherwise); rho >= 0, R = rho I
 *   X        batch x n x p   the filtered states x_t
 *   Ypred    batch x n x d or NULL (want_pred): the one-step predictions C z
 *   scalars  batch x n x 2 or NULL: (s, eta) of every step
 *   status   batch int32 or NULL, as in psmf_impute_run: PSMF_OK, or PSMF_ERR_NUMERIC for a replica whose r x r system lost
 *            positive definiteness or whose state is not finite; the other replicas are untouched by it and the call returns
 *            PSMF_OK.  With status = NULL such a replica fails the call (PSMF_ERR_NUMERIC).
 *   elapsed_ms  the kernel alone (HIP events), or NULL */
int psmf_ssm_run(const psmf_ssm_config* cfg, const double* Y, double* C, double* V, double* x, double* P, const double* A,
                 const double* Q, const double* H, double rho, double* X, double* Ypred, double* scalars, int32_t* status,
                 float* elapsed_ms);

/* psmf_ssm_run with the robust form (rPSMF: a t-distributed likelihood, ExperimentImpute/rPSMF.py:75-135 and
 * pypsmf/psmf/rpsmf.py:125-172) and with missing observations.  psmf_ssm_config's fields, then: */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;
  int32_t p;
  int32_t batch;
  int32_t device;
  int32_t carry_P;
  int32_t first_step;
  int32_t want_pred;
  int32_t robust;        /* 1: rPSMF -- the lines marked rob below                                           */
  int32_t fixed_lambda;  /* 1: lambda stays lambda0; 0: lambda <- lambda + d after every step                */
  double lambda0;        /* robust: degrees of freedom at the start of a series, finite and > 0              */
  double alpha, beta;    /* robust: the factors of V and of P (finite and > 0; 1 = the reference)            */
} psmf_ssm_config_ex;

/* Per replica and step t, float64 throughout; m is the 0/1 mask column (all ones with mask = NULL), M = diag(m), Omega the running
 * product of omega (1 at the start of a series, and always when not robust), e_i zero on unobserved rows:
 *   xbar = A x                         Pbar = A P_prev A^T + Omega Q            (carry_P as in psmf_ssm_run)
 *   z = H xbar, w = V z, s = z^T w     yhat = C z                               (Ypred: all rows, observed or not)
 *   e_i = m_i (y_i - yhat_i)           y_i is not read where m_i = 0 (it may be NaN)
 *   P_z = H Pbar H^T                   rho_t = Omega rho
 *   S = (M C) P_z (M C)^T + diag(rho_t m) + s I                                 (rPSMF.py:92-98: s I, not s M)
 *   x = xbar + Pbar H^T (MC)^T S^-1 e
 *   omega = (lambda + e^T S^-1 e) / (lambda + d)                           rob  (d, not the observed count)
 *   P = beta omega (Pbar - Pbar H^T (MC)^T S^-1 (MC) H Pbar)               rob: beta omega; else 1
 *   eta = (rho_t sum m_i + trace((MC) P_z (MC)^T)) / d,   N = s + eta
 *   C += e w^T / N                                                              (unobserved rows do not move)
 *   phi = (lambda + e^T e / N) / (lambda + d)                              rob
 *   V = alpha phi (V - w w^T / N)                                          rob: alpha phi; else 1
 *   Omega <- omega Omega;  lambda <- lambda + d unless fixed_lambda        rob
 * (S is never formed: G = sum m_i c_i c_i^T, h = sum m_i c_i e_i, the two r x r inversions of psmf_ssm_run, and
 * e^T S^-1 e = kappa e^T e - kappa^2 h^T P_z+ h.)  With robust = 0 and mask = NULL the call runs psmf_ssm_run's own kernel (the same
 * bits).  Limits and arguments as psmf_ssm_run, and:
 *   mask          batch x n x d uint8 (row t = m_t), 0 or 1, or NULL: all observed.  A step without an observed row is
 *                 PSMF_ERR_ARG (eta = 0 and phi = 0 / 0 there); the message names the replica and the step
 *   robust_state  batch x 2, in / out: (lambda, Omega) per replica -- what a continuing call takes.  Read when first_step = 0; with
 *                 first_step = 1 the call starts from (lambda0, 1).  May be NULL when not robust
 *   scalars       batch x n x 4 or NULL: (s, eta, omega, phi) of every step (omega = phi = 1 when not robust)
 * PSMF_ERR_ARG also for robust with lambda0 <= 0 or not finite, and alpha or beta <= 0. */
int psmf_ssm_run_ex(const psmf_ssm_config_ex* cfg, const double* Y, const uint8_t* mask, double* C, double* V, double* x, double* P,
                    const double* A, const double* Q, const double* H, double rho, double* robust_state, double* X, double* Ypred,
                    double* scalars, int32_t* status, float* elapsed_ms);

/* Batched multivariate Bayesian online change-point detection: the BOCPD baseline of the change-point experiment
 * (ExperimentChange/MVBOCPD.m: a normal-inverse-Wishart model per run length, Student-t predictive, constant hazard h = 1 / lambda,
 * and the reference's detection heuristic), float64 throughout, for a batch of independent series. */
typedef struct {
  int32_t abi_version;
  int32_t dim, T;          /* samples of dimension dim, T of them per series: 1 <= dim <= 32, 1 <= T <= 4096     */
  int32_t batch;           /* independent series                                                               */
  int32_t device;
  int32_t drop, settle, confirm;   /* the heuristic's constants (the reference: 10, 10, 10)                    */
  int32_t max_changepoints;        /* change points stored per series (every one is counted)                   */
  int32_t want_R;          /* also return every column of R                                                    */
  int32_t want_logpred;    /* also return the log predictive of every (step, age)                              */
  double lambda;           /* > 1: hazard h = 1 / lambda (the reference: 200)                                  */
  double kappa0, nu0;      /* prior: kappa0 > 0, nu0 > dim - 1 (the reference: 1, dim)                         */
  double sigma0;           /* prior scatter Sigma0 = sigma0 I, sigma0 > 0 (the reference: 1); mu0 = 0          */
} psmf_bocpd_config;

/* Per series, with time 1-based (t = 1 .. T) and n_t live hypotheses of ages 0 .. n_t - 1 at step t (n_1 = 1; a hypothesis of age a
 * has absorbed the a most recent samples: kappa = kappa0 + a, nu = nu0 + a; absorbing x: delta = x - mu,
 * mu <- (kappa mu + x) / (kappa + 1), Sigma <- Sigma + kappa / (2 (kappa + 1)) delta delta^T; age 0 is the prior):
 *   1. log p_a = lgamma((nu + dim) / 2) - lgamma(nu / 2) + log det(c) / 2 - dim / 2 log(nu pi) - (nu + dim) / 2 log1p(delta^T c delta / nu),
 *      c = [2 (kappa + 1) Sigma / (nu kappa)]^-1
 *   2. R(a + 1, t + 1) = R(a, t) p_a (1 - h),  R(0, t + 1) = sum_a R(a, t) p_a h  over a < n_t, the column normalised to sum 1
 *   3. m_t = 1 + argmax_a R(a, t) over the stored column t (lowest age on a tie)
 *   4. for t > 1: m_t - m_{t-1} < -drop sets a flag; otherwise, with the flag set, |m_t - m_{t-1}| < settle counts up and the count
 *      exceeding `confirm` declares the change point cp = t - m_t + 1, clears flag and count and discards the hypotheses of age
 *      >= m_t - 1 (n_{t+1} = m_t); |m_t - m_{t-1}| >= settle clears flag and count
 *   5. every remaining hypothesis absorbs x_t; a fresh prior enters at age 0
 * R is carried in the log domain: a step at which every p_a underflows leaves it finite.  One lane per hypothesis holds the Cholesky
 * factor of Sigma on chip (a forward substitution and a rank-one update per step, no inverse and no determinant); a second kernel
 * runs the recursion on R, one workgroup per series.  A batch whose scratch (T x T doubles per series) exceeds what is free on
 * the device is processed in chunks.
 *   X             batch x T x dim, time-major
 *   map_run       batch x T: m_t
 *   changepoints  batch x max_changepoints: the first max_changepoints cp values of every series (the rest of a row is 0);
 *                 may be NULL with max_changepoints = 0
 *   n_changepoints  batch: how many were declared (it may exceed max_changepoints)
 *   R_last        batch x (T + 1) or NULL: column T + 1 by age
 *   R             batch x (T + 1) x (T + 1), row t - 1 = column t by age, zero where nothing is stored; want_R = 1, else NULL
 *   logpred       batch x T x T, [t - 1][a] = log p_a of step t, NaN where age a is not live; want_logpred = 1, else NULL
 *   status        batch int32 or NULL, as in psmf_ssm_run: PSMF_OK, or PSMF_ERR_NUMERIC for a replica with a non-finite sample,
 *                 a non-finite state or a non-positive pivot; the other replicas are untouched by it.  Every other output of a
 *                 replica with a non-finite sample or a non-finite log p_a (an overflowing sample, a non-positive pivot) is zero,
 *                 R(0, 1) included: the recursion on R never starts.  (Only a log R that leaves the finite range with every
 *                 log p_a finite is found after the outputs are written; they are unspecified then.)  With status = NULL such a
 *                 replica fails the call (PSMF_ERR_NUMERIC)
 *   elapsed_ms    the kernels alone (HIP events, summed over the chunks), or NULL
 * PSMF_ERR_ARG, by message: dim > 32, T > 4096, batch < 1, lambda <= 1, kappa0 <= 0, nu0 <= dim - 1, sigma0 <= 0, and want_R or
 * want_logpred with more than 2^28 doubles (2 GiB) of output. */
int psmf_bocpd_run(const psmf_bocpd_config* cfg, const double* X, int32_t* map_run, int32_t* changepoints, int32_t* n_changepoints,
                   double* R_last, double* R, double* logpred, int32_t* status, float* elapsed_ms);

/* Batched probabilistic matrix factorisation: the PMF baseline of the imputation experiment (ExperimentImpute/PMF.py:43-159, mini-batch
 * gradient descent with momentum on the observed entries), float64 throughout, for a batch of independent replicas. */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;         /* Y is d x n, the factors have r features: 1 <= d <= 512, 1 <= r <= 16, n unlimited     */
  int32_t batch;           /* independent replicas                                                               */
  int32_t epochs;          /* passes over the training set, >= 1 (the reference: 2)                              */
  int32_t num_batches;     /* mini-batches of an epoch, 1 .. 254 (the reference: 9)                              */
  int32_t device;
  int32_t want_rec;        /* also return the reconstruction at the probe entries after the last epoch           */
  double epsilon;          /* learning rate (the reference: 50)                                                  */
  double lambda;           /* weight of the quadratic penalty (the reference: 0.01)                              */
  double momentum;         /* (the reference: 0.8)                                                               */
} psmf_pmf_config;

/* Per replica, with T = {(i, j): M_ij = 1} the training entries and N = |T|:
 *   mu = mean over T of y_ij,  v_ij = (y_ij - mu) / mu  (the reference divides by the mean),  mbar = mean over T of v_ij
 *   P = 0.1 C0 (d x r),  W = 0.1 X0^T (n x r),  incP = incW = 0                      -- formed by the caller
 *   per epoch the entries of T are dealt to num_batches batches (a random permutation cut as numpy.array_split cuts it); per batch b
 *   with N_b entries, everything from the W, P at the start of the batch:
 *     g_ij = 2 (w_j . p_i - (v_ij - mbar))                               for (i, j) in the batch
 *     dW_j = sum_i g_ij p_i + lambda c_j w_j,   dP_i = sum_j g_ij w_j + lambda c_i p_i,   c_j, c_i = batch entries of column j / row i
 *     incW = momentum incW + epsilon dW / N_b,  W -= incW;   incP = momentum incP + epsilon dP / N_b,  P -= incP
 *   (a column or row without an entry in the batch still moves by its momentum), and at the end of epoch e over the probe entries
 *   (Mmiss_ij = 1):   yhat_ij = (w_j . p_i + mbar) mu + mu,   Efull[e] = sqrt(sum (yhat_ij - y_ij)^2 / sum Mmiss)
 * The caller states the dealing as a BATCH MAP per replica and epoch: n x d bytes, time-major, the batch index of a training entry
 * and 255 elsewhere -- the order inside a batch only orders sums -- and hands over mu and mbar, so that they carry the bits of the
 * host's summation.  The three products of a batch (W P^T, G P, G^T W) run on the float64 matrix cores, a workgroup per range of
 * columns with P in LDS; W and incW are updated in place, the d x r sum dP crosses workgroups through partial sums that a second
 * kernel adds in a fixed order.  No atomics: the same call twice gives the same bits.  A batch whose maps and factors exceed what is
 * free on the device is processed in chunks of replicas.
 *   Y             n x d, time-major: the data, read at the training and the probe entries (shared by the replicas)
 *   maps          batch x epochs x n x d bytes
 *   Mmiss         batch x n x d bytes, nonzero = probe entry
 *   batch_sizes   batch x num_batches: N_b, every one >= 1
 *   row_counts    batch x epochs x num_batches x d: c_i of every batch
 *   mean, mean_rating   batch: mu (not 0) and mbar
 *   P             batch x d x r, in: 0.1 C0, out: the final P
 *   W             batch x n x r, in: 0.1 X0^T, out: the final W
 *   Efull         batch x epochs
 *   Yrec          batch x n x d, time-major, yhat at the probe entries after the last epoch and 0 elsewhere; want_rec = 1, else NULL
 *   status        batch int32 or NULL, as in psmf_ssm_run: PSMF_OK, or PSMF_ERR_NUMERIC for a replica whose factors or errors are
 *                 not finite (the steps diverged); the other replicas are untouched by it.  With status = NULL such a replica
 *                 fails the call (PSMF_ERR_NUMERIC)
 *   elapsed_ms    the kernels alone (HIP events, summed over the chunks), or NULL
 * PSMF_ERR_ARG, by message: d > 512, r > 16, num_batches outside 1 .. 254, an empty batch, a zero mean.  PSMF_PMF_COLS=n sets the
 * columns per workgroup, PSMF_PMF_CHUNK=n caps the replicas per chunk (both read at every call). */
int psmf_pmf_run(const psmf_pmf_config* cfg, const double* Y, const uint8_t* maps, const uint8_t* Mmiss, const int32_t* batch_sizes,
                 const int32_t* row_counts, const double* mean, const double* mean_rating, double* P, double* W, double* Efull,
                 double* Yrec, int32_t* status, float* elapsed_ms);

/* Batched Bayesian probabilistic matrix factorisation: the BPMF baseline of the imputation experiment (ExperimentImpute/BPMF.py:121-302,
 * a Gibbs sampler over the factors and their Gaussian-Wishart hyper-parameters), float64 throughout, for a batch of independent
 * replicas.  Every random number is drawn by the caller, up front: no draw of the sampler depends on the data. */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;         /* Y is d x n, the factors have r features: 2 <= d <= 512, 2 <= r <= 16, n >= 2            */
  int32_t batch;           /* independent replicas                                                               */
  int32_t epochs;          /* Gibbs epochs, >= 1 (the reference: 2): a hyper-parameter step and two sweeps each  */
  int32_t device;
  int32_t want_rec;        /* also return the reconstruction at the probe entries after the last epoch           */
  double beta;             /* observation precision (the reference: 2)                                           */
} psmf_bpmf_config;

/* Per replica, with T = {(i, j): M_ij != 0} the training entries, mu their mean, v_ij = (y_ij - mu) / mu (the reference divides by the
 * mean), mbar the mean of v over T, and W (n x r), P (d x r) the factors of the warm start (psmf_pmf_run's recursion, BPMF.py:43-105):
 *   avg_ij = w_j . p_i + mbar over the probe entries (Mmiss_ij != 0), c = 1
 *   epoch e = 1 .. epochs:
 *     for (F, N, A, z) = (W, n, A_m, z_m) and then (P, d, A_u, z_u), with b0 = 2:
 *       xbar = column mean of F,   S = sum_k (f_k - xbar)(f_k - xbar)^T / (N - 1)                    (numpy.cov, two passes)
 *       T = I + N S + N b0 / (b0 + N) xbar xbar^T = U U^T, U upper triangular, factored from the last row upwards
 *       alpha = X X^T with U^T X = A       (U^-T is the lower Cholesky factor of T^-1: alpha is the reference's wishart.rvs(r + N,
 *                                           sym(inv T)) where A is the standard Bartlett factor scipy draws for it)
 *       (b0 + N) alpha = V V^T the same way,   mu_h = V^-1 z + N xbar / (b0 + N)                     (cholesky(inv(.)).T z + ...)
 *     twice (the two Gibbs sweeps):
 *       every column j:  Lambda = alpha_m + beta sum_i m_ij p_i p_i^T = U U^T,  b = beta sum_i m_ij (v_ij - mbar) p_i + alpha_m mu_m,
 *                        w_j = U^-1 z_j + U^-T U^-1 b                            (cholesky(inv Lambda).T z_j + inv(Lambda) b)
 *       every row i, likewise over its training entries with the new W, alpha_u, mu_u and its own z_i
 *       (a column or row without a training entry has Lambda = alpha)
 *     avg = (c avg + w_j . p_i + mbar) / (c + 1),  c += 1,   yhat_ij = avg_ij mu + mu,
 *     Efull[e] = sqrt(sum over the probe entries of (yhat_ij - y_ij)^2 / their number)
 * The reference's "simple fit" (BPMF.py:197-201) is overwritten before it is used and is not computed.  The two Grams of a sweep and
 * the covariance of W run on the float64 matrix cores; the sums that cross workgroups are partial sums added in a fixed order.  No
 * atomics: the same call twice gives the same bits, a replica the same bits alone as inside a batch.  A batch that exceeds what is
 * free on the device is processed in chunks of replicas.
 *   Y             n x d, time-major: the data, read at the training and the probe entries (shared by the replicas)
 *   M, Mmiss      batch x n x d bytes each, nonzero = training entry / probe entry
 *   mean, mean_rating   batch: mu (not 0) and mbar
 *   bartlett      batch x epochs x 2 x r x r: A_m then A_u of every epoch, lower triangular (the diagonal: roots of chi-squares with
 *                 r + N - i degrees of freedom, i = 0 .. r - 1; below it standard normals)
 *   hyper_normals batch x epochs x 2 x r: z_m then z_u
 *   normals       batch x epochs x 2 x (n + d) x r: per sweep the z_j of the columns (n x r), then the z_i of the rows (d x r)
 *   P             batch x d x r, in: the warm start, out: the final P
 *   W             batch x n x r, likewise
 *   Efull         batch x epochs
 *   Yrec          batch x n x d, time-major, yhat at the probe entries after the last epoch and 0 elsewhere; want_rec = 1, else NULL
 *   status        batch int32 or NULL, as in psmf_pmf_run: PSMF_OK, or PSMF_ERR_NUMERIC for a replica in which a pivot of a factorisation
 *                 was not positive (numpy.linalg.LinAlgError upstream) or whose factors or errors are not finite; the other replicas
 *                 are untouched by it.  With status = NULL such a replica fails the call (PSMF_ERR_NUMERIC)
 *   elapsed_ms    the kernels alone (HIP events, summed over the chunks), or NULL
 * PSMF_ERR_ARG, by message: d outside 2 .. 512, r outside 2 .. 16, n < 2, a zero mean.  PSMF_BPMF_COLS=n sets the columns per
 * workgroup, PSMF_BPMF_CHUNK=n caps the replicas per chunk (both read at every call). */
int psmf_bpmf_run(const psmf_bpmf_config* cfg, const double* Y, const uint8_t* M, const uint8_t* Mmiss, const double* mean,
                  const double* mean_rating, const double* bartlett, const double* hyper_normals, const double* normals, double* P,
                  double* W, double* Efull, double* Yrec, int32_t* status, float* elapsed_ms);

/* The convergence experiment (Convergence/main.m, the paper's Figure 1): n_iter sweeps of the PSMF filter over one series of n steps,
 * each restarted from the first filtered state of the sweep before, every filtered posterior compared in Wasserstein-2 distance with
 * that of the Kalman filter that knows the true C.  Float64 throughout, R diagonal, for a batch of independent replicas; one lane per
 * replica with the whole state in registers. */
typedef struct {
  int32_t abi_version;
  int32_t d, n, r;         /* Y is d x n, the state has r components: 1 <= r <= 4, r <= d <= 16, n >= 2                 */
  int32_t batch;           /* independent replicas, >= 1                                                              */
  int32_t n_iter;          /* sweeps of this call, >= 1 (the reference: 10000)                                         */
  int32_t own_data;        /* 0: one Y, Ctrue and Kalman path for all replicas; 1: every replica has its own           */
  int32_t want_moments;    /* also return C, Sxy and Sxx of every iteration (what ErM = ||Y - C Xps||_2 is formed from) */
  int32_t device;
} psmf_conv_config;

/* The Kalman pass (main.m:15-34), once per call and series, from x = x0k, P = P0k, for t = 1 .. n:
 *   Pp = P + Q,  S = (R + Ctrue Pp Ctrue^T)^-1,  x <- x + Pp Ctrue^T S (y_t - Ctrue x),  P <- Pp - Pp Ctrue^T S Ctrue Pp;  Xk(:,t) = x, Pk(:,:,t) = P
 * One iteration (main.m:49-108), per replica, with V = v I at its top and (xp, Pprev) = (X0, P0) at t = 1, (Xps(:,t-1), Pps(:,:,t-1)) after:
 *   1. Pp = Pprev + q_scale Q                         (q_scale, r_scale: main.m:44-45's knobs; the Kalman pass uses Q and R as given)
 *   2. s = xp^T V xp
 *   3. eta = trace(r_scale R + C Pp C^T) / d
 *   4. S = (r_scale R + s I + C Pp C^T)^-1
 *   5. Xps(:,t) = xp + Pp C^T S (y_t - C xp)
 *   6. Pps(:,:,t) = Pp - Pp C^T S C Pp
 *   7. C <- C + (y_t - C xp) xp^T V / (s + eta)
 *   8. V <- V - V xp xp^T V / (s + eta)
 *   9. Cerr(t) = ||C - Ctrue||_2
 *  10. W(t) = W2(N(Xps_t, Pps_t), N(Xk_t, Pk_t)) for t >= 2, W(1) = 0
 *   then avW = mean of W over all n entries, CerrI = ||C - Ctrue||_2 (the largest singular value), and the next iteration starts from
 *   X0 = Xps(:,1), P0 = Pps(:,:,1) with the same C.  (main.m:54 writes P0ps = Pps(:,1), which is Pps(:,:,1) at r = 1, the reference's
 *   only shape, and no covariance at r > 1.)
 * S is applied through the r x r system (two Cholesky factorisations in registers per step; no d x d inverse is formed), and W2 through
 * the eigenvalues of an r x r product (closed form at r <= 2, cyclic Jacobi above; no matrix square root).  A W2^2 that cancellation
 * makes negative is returned as 0, where Matlab returns a complex number.  A launch covers at most K iterations, K the largest with
 * n K <= 2^20 steps (PSMF_CONV_ITERS=k: at most k); the state crosses launches in device memory as float64: the same bits at every K.
 * A batch that exceeds what is free on the device is processed in chunks of replicas (PSMF_CONV_CHUNK=n caps a chunk); both switches
 * are read at every call and change no output bit.  Symmetric r x r matrices are PACKED where noted: the lower triangle by rows,
 * nt = r (r + 1) / 2 elements, (i, j) at i (i + 1) / 2 + j.
 *   Y          n x d, time-major (own_data: batch x n x d)
 *   Ctrue      d x r (own_data: batch x d x r)
 *   Q          r x r, symmetric positive definite;  Rdiag: d, the diagonal of R, > 0 (both shared by the replicas)
 *   x0k, P0k   r and r x r, the start of the Kalman pass (own_data: batch x r, batch x r x r)
 *   v, q_scale, r_scale   batch each: v > 0, q_scale >= 0, r_scale > 0
 *   C, x0, P0  batch x d x r, batch x r, batch x r x r; in: the start, out: the final C, Xps(:,1) and Pps(:,:,1) of the last
 *              iteration -- what a continuing call takes: two calls of k iterations give the bits of one call of 2 k
 *   Xk, Pk     n x r and n x nt (packed), the Kalman path (own_data: batch x n x r, batch x n x nt)
 *   avW, CerrI batch x n_iter
 *   C_iter, Sxy, Sxx   batch x n_iter x (d x r | r x d | nt): the C at the end of every iteration, Sxy = sum_t Xps_t y_t^T and
 *              Sxx = sum_t Xps_t Xps_t^T (packed); want_moments = 1, else NULL.  (E E^T = Y Y^T - C Sxy - (C Sxy)^T + C Sxx C^T for
 *              E = Y - C Xps: the caller takes the d x d spectral norm.)
 *   Xps, Pps, W, Cerr  batch x n x (r | nt packed | 1 | 1): every step of the call's last iteration
 *   status     batch int32 or NULL, as in psmf_ssm_run: PSMF_OK, or PSMF_ERR_NUMERIC for a replica with a non-finite input, a pivot
 *              of an r x r factorisation that is not positive or a state that is not finite; it stops there (its outputs are
 *              unspecified) and the other replicas, those of its wave included, are untouched by it.  With status = NULL such a
 *              replica fails the call (PSMF_ERR_NUMERIC)
 *   elapsed_ms the kernels alone (HIP events, summed over the chunks), or NULL
 * PSMF_ERR_ARG, by message: r outside 1 .. 4, d outside r .. 16 (for d < r the factorisation is not identifiable and the recursion
 * amplifies rounding without bound), n < 2, n_iter < 1, batch < 1, a diagonal entry of R <= 0, a Q that is not symmetric, non-finite
 * shared data.  PSMF_ERR_NUMERIC for the call where the shared Kalman pass loses positive definiteness. */
int psmf_conv_run(const psmf_conv_config* cfg, const double* Y, const double* Ctrue, const double* Q, const double* Rdiag,
                  const double* x0k, const double* P0k, const double* v, const double* q_scale, const double* r_scale, double* C,
                  double* x0, double* P0, double* Xk, double* Pk, double* avW, double* CerrI, double* C_iter, double* Sxy, double* Sxx,
                  double* Xps, double* Pps, double* W, double* Cerr, int32_t* status, float* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* PSMF_HIP_H */
