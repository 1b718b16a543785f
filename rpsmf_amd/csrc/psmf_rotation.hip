// The noise rotation of a handle with a non-diagonal R = U diag(lam) U^T: the handle keeps the series, C and y_hat in the rotated
// coordinates, and these float64 GEMMs against the resident U (psmf_rotate.hip) take rows and the dictionary in and out.
#include "psmf_host.h"
#include "psmf_rotate.hip"

#include <cmath>
#include <string>
#include <vector>

namespace {

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

}  // namespace

// the dictionary (d x rp, storage type): dst = U^T src (fwd) or U src (back)
int rot_dict(psmf_filter* h, const void* src, void* dst, bool fwd) {
  const long long d = h->cfg.d_local, rp = h->geo.rp, r = h->cfg.r;
  const long long ai = fwd ? 1 : d, ak = fwd ? d : 1;
  return by_storage(h, [&](auto t) { return rot_gemm(h, (const double*)h->rotU, ai, ak, (const decltype(t)*)src, rp, 1LL, (decltype(t)*)dst, rp, d, r, d); });
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

// float64 rows (n x d, row stride d: the projections of psmf_project) times U^T, back into the caller's coordinates: src -> dst
int rot_rows_back_f64(psmf_filter* h, const double* src, double* dst, long long n) {
  const long long dl = h->cfg.d_local;
  return rot_gemm(h, src, dl, 1LL, (const double*)h->rotU, 1LL, dl, dst, dl, n, dl, dl);
}

extern "C" {

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

}  // extern "C"
