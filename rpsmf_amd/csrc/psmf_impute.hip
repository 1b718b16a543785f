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
#include "psmf_host.h"        // Switches
#include "psmf_batch.h"       // EntryFail, open_device, typed transfers, TimedLaunch, replica_status
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
// psmf_impute_run beyond one workgroup's LDS (d > 512 or r > 16): the replicas one after the other on the masked per-step engine
// of the large-d handle (psmf_masked.hip), float64 storage, through the public ABI alone.  ExperimentImpute/PSMF.py:59-95,
// rPSMF.py:75-148: the prior mean of column 0 is X[:, n - 1] (the initial X on pass 0, the last posterior afterwards -- i.e. the
// running mean), C, V, P carry over the passes, rPSMF restarts Q, rho, lambda at every pass; X[:, t] is the posterior mean of column t
// (the mean history).
hipError_t destroy_filter(psmf_handle h) { psmf_destroy(h); return hipSuccess; }
using OwnedFilter = Owned<psmf_handle, destroy_filter>;

int impute_run_large(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M, const uint8_t* Mmiss, double* C, double* X,
                     const double* V, const double* P, const double* Q, double rho, double* Epred, double* Efull, double* inside,
                     double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  const int d = cfg->d, n = cfg->n, r = cfg->r, B = cfg->batch, robust = cfg->method == 1, meth = cfg->method;
  psmf_config pc;
  memset(&pc, 0, sizeof(pc));
  pc.abi_version = PSMF_ABI_VERSION; pc.d = d; pc.r = r; pc.row0 = 0; pc.d_local = d; pc.robust = robust;
  pc.coef_update = 1; pc.eta_full = 1; pc.pbar_predict = 1; pc.dyn_kind = PSMF_DYN_RANDOM_WALK; pc.n_theta = 0;
  pc.storage = PSMF_F64; pc.store_y_pred = 1; pc.update_every = 1; pc.device = cfg->device; pc.use_graph = 1; pc.engine = 1; pc.masked = meth >= 2 ? meth : 1;
  pc.alpha = pc.beta = 1.0; pc.adam_lr = 1e-3; pc.adam_b1 = 0.9; pc.adam_b2 = 0.999;
  OwnedFilter h;                   // released on every return, after `bail` has read its message
  PSMF_TRY(psmf_create(h.put(), &pc));      // (g_create_error holds the message)
  // a failed call's code, with the handle's message left where a caller without a handle looks for it
  auto bail = [&](int code) { if (code) g_create_error = std::string("psmf_impute_run: ") + psmf_last_error(h); return code; };
  PSMF_TRY(bail(psmf_upload_series(h, YorgInt, PSMF_F64, 0, n, n)));
  const size_t nd = (size_t)n * d;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> yp, sc;
  double total_ms = 0.0;
  for (int b = 0; b < B; ++b) {
    double* Cb = C + (size_t)b * d * r;
    double* Xb = X + (size_t)b * n * r;
    PSMF_TRY(bail(psmf_upload_mask(h, M + (size_t)b * nd, 0, n)));
    int rc;
    if (meth == 3) {       // TMF (TMF.py:47,60): Pbar = I / nu at every step, nu = 2 -- as Q with P = 0 (the serial stage keeps P at 0); V unused
      std::vector<double> Inu((size_t)r * r, 0.0), Zr((size_t)r * r, 0.0), Iv((size_t)r * r, 0.0);
      for (int i = 0; i < r; ++i) { Inu[(size_t)i * r + i] = 0.5; Iv[(size_t)i * r + i] = 1.0; }
      rc = psmf_set_state(h, Cb, Iv.data(), Zr.data(), Inu.data(), Xb + (size_t)(n - 1) * r, 1.0, 0.0, nullptr);
    } else {
      rc = psmf_set_state(h, Cb, V, P, Q, Xb + (size_t)(n - 1) * r, rho, robust ? cfg->lambda0 : 0.0, nullptr);
    }
    PSMF_TRY(bail(rc));
    bool bad = false;
    double m4[4] = {0, 0, 0, 0};
    const auto t_start = std::chrono::steady_clock::now();
    for (int it = 0; it < cfg->n_iter && !bad; ++it) {
      if (it > 0 && robust) {        // rPSMF.py:77-79: Q, R, lambda restart; V, P, C and the mean carry over
        PSMF_TRY(bail(psmf_set_state(h, nullptr, nullptr, nullptr, Q, nullptr, rho, cfg->lambda0, nullptr)));
      }
      if (meth >= 2) {       // gam = 1e-6 / (pass + 1)^0.7  (MLESMF.py:59-60, TMF.py:46-48)
        PSMF_TRY(bail(psmf_set_step_size(h, 1e-6 / std::pow((double)(it + 1), 0.7))));
      }
      PSMF_TRY(bail(psmf_run(h, 0, n)));
      rc = psmf_masked_metrics(h, Mmiss + (size_t)b * nd, 0, n, meth == 3 ? 0.0 : cfg->sig, m4);
      if (rc == PSMF_ERR_NUMERIC) { bad = true; break; }
      PSMF_TRY(bail(rc));
      Epred[(size_t)b * cfg->n_iter + it] = std::sqrt(m4[0] / m4[3]);
      Efull[(size_t)b * cfg->n_iter + it] = std::sqrt(m4[1] / m4[3]);
      if (!std::isfinite(m4[0]) || !std::isfinite(m4[1])) bad = true;
    }
    total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (!bad) {
      inside[b] = m4[2] / m4[3];
      rc = psmf_get_state(h, Cb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
      if (!rc) rc = psmf_download_mu(h, Xb, 1, n);
      if (!rc && cfg->want_bands) {
        yp.resize(nd); sc.resize((size_t)2 * n);
        rc = psmf_download_y_pred(h, yp.data(), PSMF_F64, 0, n);
        if (!rc) rc = psmf_download_step_scalars(h, sc.data(), 0, n);
        if (!rc) {
          const uint8_t* Mb = M + (size_t)b * nd;
          for (int t = 0; t < n; ++t)
            for (int i = 0; i < d; ++i) {
              const size_t at = (size_t)b * nd + (size_t)t * d + i;
              const double yh = yp[(size_t)t * d + i];
              const double band = meth == 3 ? 0.0 : cfg->sig * std::sqrt(robust ? (Mb[(size_t)t * d + i] ? sc[2 * t] : 0.0) + sc[2 * t + 1] : sc[2 * t] + sc[2 * t + 1]);
              Yrec[at] = yh; YrecL[at] = yh - band; YrecH[at] = yh + band;
            }
        }
      }
      if (rc == PSMF_ERR_NUMERIC) bad = true;
      else PSMF_TRY(bail(rc));
    }
    if (status) status[b] = bad ? PSMF_ERR_NUMERIC : PSMF_OK;
    if (bad) {
      if (!status) return bail(PSMF_ERR_NUMERIC);
      for (int it = 0; it < cfg->n_iter; ++it) Epred[(size_t)b * cfg->n_iter + it] = Efull[(size_t)b * cfg->n_iter + it] = qnan;
      inside[b] = qnan;
    }
  }
  if (elapsed_ms) *elapsed_ms = (float)total_ms;
  return PSMF_OK;
}

// psmf_impute_run (rho_rows == nullptr: R = rho I) and psmf_impute_run_rows (R = diag(rho_rows), entries not all equal; `rho` unused)
int impute_run_impl(const EntryFail& fail, const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                    const uint8_t* Mmiss, double* C, double* X, const double* V, const double* P,
                    const double* Q, double rho, const double* rho_rows, double* Epred, double* Efull, double* inside,
                    double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  using namespace psmf;
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
  PSMF_TRY(open_device(fail, cfg->device));

  const size_t nd = (size_t)n * d, bnd = (size_t)B * nd, nC = (size_t)B * d * r, nX = (size_t)B * n * r, rr = (size_t)r * r;
  const size_t ni = cfg->n_iter, nbands = cfg->want_bands ? bnd : 0;
  Dev<double> dY, dC, dX, dV, dP, dQ, dEp, dEf, dIn, dYr, dYl, dYh, dRho;
  Dev<uint8_t> dM, dMm;
  Dev<int> dErr;
  TimedLaunch timed;
  std::vector<int> herr(B, 0);
  ImputeParams ip;
  const auto io = std::make_tuple(      // buffer, filled from, read back to, elements
      slot(dY, YorgInt, nullptr, nd), slot(dM, M, nullptr, bnd), slot(dMm, Mmiss, nullptr, bnd),
      slot(dC, C, C, nC), slot(dX, X, X, nX), slot(dV, V, nullptr, rr), slot(dP, P, nullptr, rr), slot(dQ, Q, nullptr, rr),
      slot(dEp, nullptr, Epred, B * ni), slot(dEf, nullptr, Efull, B * ni), slot(dIn, nullptr, inside, B), slot(dErr, nullptr, herr.data(), B),
      slot(dYr, nullptr, Yrec, nbands), slot(dYl, nullptr, YrecL, nbands), slot(dYh, nullptr, YrecH, nbands));
  PSMF_TRY(alloc_all(fail, io));
  if (rw) PSMF_TRY(alloc_copy_in(fail, dRho, rho_rows, d));
  PSMF_TRY(copy_in_all(fail, io));
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
  PSMF_TRY(timed.run(fail, kern, dim3(B), dim3(WG), &ip, lds, elapsed_ms));
  PSMF_TRY(copy_out_all(fail, io));
  // Per-replica outcome (the reference records NaN for a diverged repeat and carries on, ExperimentImpute/rPSMF.py:236-243): a
  // replica whose r x r system lost positive definiteness -- or whose errors are not finite -- gets status PSMF_ERR_NUMERIC and NaN
  // results; the other replicas are untouched by it (one workgroup each).  Without a status array the call fails as a whole.
  for (int b = 0; b < B; ++b)
    if (herr[b] == 9) return fail(PSMF_ERR_HIP, "internal error: the wave programs of the column loop executed different numbers of barriers (imp_barrier_check)");
  const auto bad = [&](int b) {
    bool nf = herr[b] != 0;
    for (size_t i = b * ni; i < (b + 1) * ni && !nf; ++i) nf = !std::isfinite(Epred[i]) || !std::isfinite(Efull[i]);
    return nf;
  };
  PSMF_TRY(replica_status(fail, B, status, bad, [](int b) { return "singular r x r system in replica " + std::to_string(b); }));
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; status && b < B; ++b) {      // (without a status array a bad replica has failed the call above)
    if (status[b] == PSMF_OK) continue;
    for (size_t i = b * ni; i < (b + 1) * ni; ++i) Epred[i] = Efull[i] = qnan;
    inside[b] = qnan;
  }
  return PSMF_OK;
}
}  // namespace

extern "C" int psmf_impute_run(const psmf_impute_config* cfg, const double* YorgInt, const uint8_t* M,
                               const uint8_t* Mmiss, double* C, double* X, const double* V, const double* P,
                               const double* Q, double rho, double* Epred, double* Efull, double* inside,
                               double* Yrec, double* YrecL, double* YrecH, int32_t* status, float* elapsed_ms) {
  return impute_run_impl(EntryFail{"psmf_impute_run"}, cfg, YorgInt, M, Mmiss, C, X, V, P, Q, rho, nullptr, Epred, Efull, inside, Yrec, YrecL, YrecH,
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
  const EntryFail fail{"psmf_impute_run_rows"};
  if (!cfg || !rho_rows) return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  if (cfg->d < 1) return fail(PSMF_ERR_ARG, "need d >= 1");
  bool uniform = true;
  for (int i = 0; i < cfg->d; ++i) {
    if (!std::isfinite(rho_rows[i]) || rho_rows[i] < 0.0)
      return fail(PSMF_ERR_ARG, "the entries of diag(R) must be finite and >= 0 (row " + std::to_string(i) + ")");
    uniform = uniform && rho_rows[i] == rho_rows[0];
  }
  return impute_run_impl(fail, cfg, YorgInt, M, Mmiss, C, X, V, P, Q, rho_rows[0], (uniform || cfg->method == 3) ? nullptr : rho_rows,
                         Epred, Efull, inside, Yrec, YrecL, YrecH, status, elapsed_ms);
}
