// Masked, batched small-d engine: the filter loops of ExperimentImpute
//   ProbabilisticSequentialMatrixFactorizer   ExperimentImpute/PSMF.py:40-95
//   robust_PSMF                               ExperimentImpute/rPSMF.py:40-148
// and the two baseline filters of the imputation tables that share their masked contractions
//   stochasticGradientStateSpaceMF (MLE-SMF)  ExperimentImpute/MLESMF.py:40-92   weights m_i / rho_i, C += gam / eta (m o e) x_p^T
//   temporalRegularizedMF (TMF)               ExperimentImpute/TMF.py:30-73      x_t = x_p + (nu I + G)^-1 C^T e, C += gam (m o e) x_p^T
// plus the RMSEM / compute_number_inside_bars reductions made on their outputs
// (ExperimentImpute/common.py:79-94), for a whole batch of independent replicas (seeds).
//
// One 256-thread workgroup per replica; the replica's entire state (C d x r, V, P, Q, x) lives
// in LDS / registers in float64 and the kernel runs all n_iter * n columns without returning to
// the host.  The observation weights change every column (mask), so the r x r Gram
// sum_i m_i c_i c_i^T is recomputed per column (no algebraic tracking); d <= a few hundred here.
// Per column: masked residual, augmented Gram [C | e]^T diag(m) [C | e] (gives G, b = C^T e, e^T e in
// one pass), the two symmetric sweep inversions of the reference's Woodbury form
// (PSMF.py:30-36), the Kalman update of x, the rank-1 updates of C and V, error bands.
// Everything is latency-bound; inputs of column t+1 are prefetched while column t is processed, and the barriers inside the
// column loop order LDS only (solve_barrier<true>): the prefetch and the per-column stores (X, bands) stay in flight across them.
#include "psmf_host.h"        // Switches, g_create_error
#include "psmf_impute3.hip"    // (and, through it, psmf_impute2.hip)

#include <cmath>
#include <cstring>
#include <string>

namespace {
// Which column loop a shape gets (also what psmf_impute_kernel_id reports): 2 = psmf_impute_kernel2 (round 1's loop, id 1, was removed in round 5),
// 300 + NG = psmf_impute_kernel3<NG> (d <= 80, r <= 14), 4 = the masked per-step engine of the large-d handle (any d, r <= PSMF_RMAX):
// one workgroup per replica needs the replica's C, V, x in LDS (d <= 512, r <= 16).
int impute_select(int d, int r, bool allow_v3, size_t* lds_out, bool row_noise = false) {
  using namespace psmf;
  if (r > IR || d > 2 * WG) return 4;
  const bool v3 = impute3_ok(d, r) && allow_v3;   // small shapes: every wave its own Gram
  const size_t lds = v3 ? impute3_lds_bytes(d, r, row_noise) : impute2_lds_bytes(d, r, row_noise);
  if (lds > 160 * 1024) return 4;
  if (lds_out) *lds_out = lds;
  return v3 ? 300 + impute3_groups(d) : 2;
}
}  // namespace

extern "C" int psmf_impute_kernel_id(const psmf_impute_config* cfg) {
  if (!cfg || cfg->abi_version != PSMF_ABI_VERSION || cfg->d < 1 || cfg->r < 1 || cfg->r > PSMF_RMAX) return PSMF_ERR_ARG;
  return impute_select(cfg->d, cfg->r, Switches().impute_v3, nullptr);
}

namespace {
// psmf_impute_run (rho_rows == nullptr: R = rho I) and psmf_impute_run_rows (R = diag(rho_rows), entries not all equal; `rho` unused)
int impute_run_impl(const char* who, const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                    const uint8_t* Mmiss, double* C, double* X, const double* V, const double* P,
                    const double* Q, double rho, const double* rho_rows, double* Epred, double* Efull, double* inside,
                    double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  using namespace psmf;
  // every message starts with `who`; there is no handle here, and the three-argument form is the one HIP_TRY / ALLOC_TRY call
  const struct {
    const char* who;
    int operator()(int code, const std::string& msg) const { g_create_error = std::string(who) + ": " + msg; return code; }
    int operator()(psmf_handle, int code, const std::string& msg) const { return (*this)(code, msg); }
  } fail{who};
  const psmf_handle w = nullptr;
  if (!cfg || !YorgInt || !M || !Mmiss || !C || !X || !V || !P || !Q || !Epred || !Efull || !inside)
    return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const int d = cfg->d, n = cfg->n, r = cfg->r, B = cfg->batch;
  if (r < 1 || r > PSMF_RMAX) return fail(PSMF_ERR_ARG, "need 1 <= r <= PSMF_RMAX");
  if (d < 1) return fail(PSMF_ERR_ARG, "need d >= 1");
  if (n < 2 || B < 1 || cfg->n_iter < 1) return fail(PSMF_ERR_ARG, "bad n / batch / n_iter");
  if (cfg->method < 0 || cfg->method > 3) return fail(PSMF_ERR_ARG, "method must be 0 (PSMF), 1 (rPSMF), 2 (MLE-SMF) or 3 (TMF)");
  if (cfg->want_bands && (!Yrec || !YrecL || !YrecH)) return fail(PSMF_ERR_ARG, "want_bands needs Yrec, YrecL, YrecH");
  const Switches sw;      // no handle here: read at entry, on every call
  size_t lds = 0;
  const bool rw = rho_rows != nullptr;
  const int sel = impute_select(d, r, sw.impute_v3, &lds, rw);
  if (sel == 4 && rw)
    return fail(PSMF_ERR_ARG, "per-row observation noise (unequal entries of diag(R)) runs on the one-workgroup kernels only, "
                              "d <= 512 and r <= 16: this shape belongs to the masked per-step engine of the large-d handle, which takes R = rho I");
  if (sel == 4)       // beyond one workgroup's LDS: the replicas one after the other on the masked per-step engine (psmf_masked.hip)
    return impute_run_large(cfg, YorgInt, M, Mmiss, C, X, V, P, Q, rho, Epred, Efull, inside, Yrec, YrecL, YrecH, status, elapsed_ms);
  const bool v3 = sel >= 300;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PSMF_ERR_NO_DEVICE, "no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(PSMF_ERR_ARG, "bad device ordinal");

  const size_t nd = (size_t)n * d, bnd = (size_t)B * nd;
  Dev<double> dY, dC, dX, dV, dP, dQ, dEp, dEf, dIn, dYr, dYl, dYh, dRho;
  Dev<uint8_t> dM, dMm;
  Dev<int> dErr;
  Event e0, e1;
  std::vector<int> herr(B, 0);
  ImputeParams ip;
  HIP_TRY(w, hipSetDevice(cfg->device));
  ALLOC_TRY(w, dY.alloc(nd * 8));
  ALLOC_TRY(w, dM.alloc(bnd));
  ALLOC_TRY(w, dMm.alloc(bnd));
  ALLOC_TRY(w, dC.alloc((size_t)B * d * r * 8));
  ALLOC_TRY(w, dX.alloc((size_t)B * n * r * 8));
  ALLOC_TRY(w, dV.alloc(r * r * 8));
  ALLOC_TRY(w, dP.alloc(r * r * 8));
  ALLOC_TRY(w, dQ.alloc(r * r * 8));
  ALLOC_TRY(w, dEp.alloc((size_t)B * cfg->n_iter * 8));
  ALLOC_TRY(w, dEf.alloc((size_t)B * cfg->n_iter * 8));
  ALLOC_TRY(w, dIn.alloc((size_t)B * 8));
  ALLOC_TRY(w, dErr.alloc((size_t)B * 4));
  if (cfg->want_bands) {
    ALLOC_TRY(w, dYr.alloc(bnd * 8));
    ALLOC_TRY(w, dYl.alloc(bnd * 8));
    ALLOC_TRY(w, dYh.alloc(bnd * 8));
  }
  if (rw) {
    ALLOC_TRY(w, dRho.alloc((size_t)d * 8));
    HIP_TRY(w, hipMemcpy(dRho, rho_rows, (size_t)d * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(w, hipMemcpy(dY, YorgInt, nd * 8, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dM, M, bnd, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dMm, Mmiss, bnd, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dC, C, (size_t)B * d * r * 8, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dX, X, (size_t)B * n * r * 8, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dV, V, r * r * 8, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dP, P, r * r * 8, hipMemcpyHostToDevice));
  HIP_TRY(w, hipMemcpy(dQ, Q, r * r * 8, hipMemcpyHostToDevice));
  ip.d = d; ip.n = n; ip.r = r; ip.n_iter = cfg->n_iter; ip.robust = cfg->method == 1; ip.method = cfg->method; ip.want_bands = cfg->want_bands;
  ip.sig = cfg->sig; ip.lambda0 = cfg->lambda0; ip.rho0 = rho;
  ip.Yorg = dY; ip.M = dM; ip.Mmiss = dMm; ip.C = dC; ip.X = dX; ip.V0 = dV; ip.P0 = dP; ip.Q0 = dQ;
  ip.Epred = dEp; ip.Efull = dEf; ip.inside = dIn; ip.Yrec = dYr; ip.YrecL = dYl; ip.YrecH = dYh; ip.err = dErr; ip.prof = nullptr;
  ip.rho_rows = dRho;
  {
    bool iso = Q[0] > 0.0 && sw.impute_par;
    for (int i = 0; i < r && iso; ++i)
      for (int c = 0; c < r; ++c)
        if (Q[i * r + c] != (i == c ? Q[0] : 0.0)) { iso = false; break; }
    ip.q_iso = iso ? 1 : 0;
  }
  const void* const kern = v3 ? impute3_kernel(d, rw) : (rw ? (const void*)psmf_impute_kernel2w : (const void*)psmf_impute_kernel2);
  if (lds > 48 * 1024) HIP_TRY(w, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(w, hipEventCreate(e0.put()));
  HIP_TRY(w, hipEventCreate(e1.put()));
  HIP_TRY(w, hipEventRecord(e0, 0));
  { void* args[] = {&ip}; HIP_TRY(w, hipLaunchKernel(kern, dim3(B), dim3(WG), args, lds, 0)); }
  HIP_TRY(w, hipGetLastError());
  HIP_TRY(w, hipEventRecord(e1, 0));
  HIP_TRY(w, hipEventSynchronize(e1));
  if (elapsed_ms) HIP_TRY(w, hipEventElapsedTime(elapsed_ms, e0, e1));
  HIP_TRY(w, hipMemcpy(C, dC, (size_t)B * d * r * 8, hipMemcpyDeviceToHost));
  HIP_TRY(w, hipMemcpy(X, dX, (size_t)B * n * r * 8, hipMemcpyDeviceToHost));
  HIP_TRY(w, hipMemcpy(Epred, dEp, (size_t)B * cfg->n_iter * 8, hipMemcpyDeviceToHost));
  HIP_TRY(w, hipMemcpy(Efull, dEf, (size_t)B * cfg->n_iter * 8, hipMemcpyDeviceToHost));
  HIP_TRY(w, hipMemcpy(inside, dIn, (size_t)B * 8, hipMemcpyDeviceToHost));
  HIP_TRY(w, hipMemcpy(herr.data(), dErr, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (cfg->want_bands) {
    HIP_TRY(w, hipMemcpy(Yrec, dYr, bnd * 8, hipMemcpyDeviceToHost));
    HIP_TRY(w, hipMemcpy(YrecL, dYl, bnd * 8, hipMemcpyDeviceToHost));
    HIP_TRY(w, hipMemcpy(YrecH, dYh, bnd * 8, hipMemcpyDeviceToHost));
  }
  // Per-replica outcome (the reference records NaN for a diverged repeat and carries on, ExperimentImpute/rPSMF.py:236-243): a
  // replica whose r x r system lost positive definiteness -- or whose errors are not finite -- gets status PSMF_ERR_NUMERIC and NaN
  // results; the other replicas are untouched by it (one workgroup each).  Without a status array the call fails as a whole.
  for (int b = 0; b < B; ++b)
    if (herr[b] == 9) return fail(PSMF_ERR_HIP, "internal error: the wave programs of the column loop executed different numbers of barriers (imp_barrier_check)");
  for (int b = 0; b < B; ++b) {
    bool bad = herr[b] != 0;
    for (int it = 0; it < cfg->n_iter && !bad; ++it)
      bad = !std::isfinite(Epred[(size_t)b * cfg->n_iter + it]) || !std::isfinite(Efull[(size_t)b * cfg->n_iter + it]);
    if (status) status[b] = bad ? PSMF_ERR_NUMERIC : PSMF_OK;
    if (!bad) continue;
    if (!status) return fail(PSMF_ERR_NUMERIC, "singular r x r system in replica " + std::to_string(b));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int it = 0; it < cfg->n_iter; ++it) Epred[(size_t)b * cfg->n_iter + it] = Efull[(size_t)b * cfg->n_iter + it] = qnan;
    inside[b] = qnan;
  }
  return PSMF_OK;
}
}  // namespace

extern "C" int psmf_impute_run(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                               const uint8_t* Mmiss, double* C, double* X, const double* V, const double* P,
                               const double* Q, double rho, double* Epred, double* Efull, double* inside,
                               double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  return impute_run_impl("psmf_impute_run", cfg, YorgInt, M, Mmiss, C, X, V, P, Q, rho, nullptr, Epred, Efull, inside, Yrec, YrecL, YrecH,
                         status, elapsed_ms);
}

// R = diag(rho_rows), d entries shared by the replicas (the reference reads np.diag(R) row by row: ExperimentImpute/PSMF.py:70-72,
// rPSMF.py:91-98, MLESMF.py:70-76).  Entries all equal -- and TMF, which ignores R (TMF.py:30-73) -- are psmf_impute_run itself: the
// same kernels, the same bits.  Unequal entries run the row-noise instances of the one-workgroup kernels (psmf_impute_kernel3w<NG>,
// psmf_impute_kernel2w: d <= 512, r <= 16); a shape beyond them is PSMF_ERR_ARG.
extern "C" int psmf_impute_run_rows(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                                    const uint8_t* Mmiss, double* C, double* X, const double* V, const double* P,
                                    const double* Q, const double* rho_rows, double* Epred, double* Efull, double* inside,
                                    double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  const char* who = "psmf_impute_run_rows";
  if (!cfg || !rho_rows) { g_create_error = std::string(who) + ": null argument"; return PSMF_ERR_ARG; }
  if (cfg->abi_version != PSMF_ABI_VERSION) { g_create_error = std::string(who) + ": ABI version mismatch"; return PSMF_ERR_ARG; }
  if (cfg->d < 1) { g_create_error = std::string(who) + ": need d >= 1"; return PSMF_ERR_ARG; }
  bool uniform = true;
  for (int i = 0; i < cfg->d; ++i) {
    if (!std::isfinite(rho_rows[i]) || rho_rows[i] < 0.0) {
      g_create_error = std::string(who) + ": the entries of diag(R) must be finite and >= 0 (row " + std::to_string(i) + ")";
      return PSMF_ERR_ARG;
    }
    uniform = uniform && rho_rows[i] == rho_rows[0];
  }
  return impute_run_impl(who, cfg, YorgInt, M, Mmiss, C, X, V, P, Q, rho_rows[0], (uniform || cfg->method == 3) ? nullptr : rho_rows,
                         Epred, Efull, inside, Yrec, YrecL, YrecH, status, elapsed_ms);
}
