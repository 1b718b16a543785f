// The convergence experiment (Convergence/main.m, the appendix experiment behind the paper's Figure 1): the PSMF filter swept n_iter
// times over one series of n steps, every sweep restarted from the first filtered state of the one before, and every filtered posterior
// compared in Wasserstein-2 distance with that of the Kalman filter that knows the true C.  Float64 throughout, R diagonal, for a batch
// of independent replicas: n_iter * n strictly serial steps of r x r algebra each.
//
// One LANE per replica, 64-lane workgroups, no barrier, nothing between lanes.  C (d x r), the state, P, V, the sums of an iteration
// and y_t are registers (but the 64 sums of Sxy at r = 4 under the capacity 16, which would push that instance into scratch memory:
// they are a lane's own column of LDS): r is a template parameter, d a run-time value under a compile-time capacity D (4, 8 or 16), every
// loop over rows and columns is unrolled with compile-time bounds and the tail rows are predicated on i < d (uniform over the wave);
// no register array is indexed with a run-time value.  Twelve instances (r x D) of each kernel, dispatched from one table.
//
//   psmf_conv_kalman_kernel<R, D>      the Kalman pass (main.m:15-34), one lane per series (one lane in all with shared data):
//       Pp = P + Q,  x <- x + Pp Ct^T S (y_t - Ct x),  P <- Pp - Pp Ct^T S Ct Pp,  S = (R + Ct Pp Ct^T)^-1
//       It keeps x and P (packed lower triangle) of every step on the device for the sweeps, replica-minor (element e of step t of
//       replica b at (t * per + e) * stride + b: the load of a wave is one contiguous line), and copies each replica's Y into that
//       layout on its way.
//   psmf_conv_sweep_kernel<R, D, OWN>  at most K iterations of main.m:49-108 per launch; per step, xp and Pprev being (X0, P0) at
//       t = 1 and the step before's (x, P) after that, V = v I at the top of an iteration:
//         Pp = Pprev + q_scale Q          w = V xp,  s = xp^T w           e = y_t - C xp
//         eta = trace(r_scale R + C Pp C^T) / d                           S = (r_scale R + s I + C Pp C^T)^-1
//         x = xp + Pp C^T S e             P = Pp - Pp C^T S C Pp
//         C += e w^T / (s + eta)          V -= w w^T / (s + eta)
//         W_t = W2(N(x, P), N(xk_t, Pk_t)) for t >= 2, 0 at t = 1
//       after the sweep avW = mean_t W_t and CerrI = ||C - Ctrue||_2; the next iteration starts from X0 = x_1, P0 = P_1 and keeps C.
//       OWN = false: Y, Ctrue and the Kalman path are shared, their addresses depend on t alone (uniform loads);  OWN = true: every
//       replica has its own, replica-minor.
//
// The d x d inverse is never formed.  With D_b = r_scale R + s I (diagonal), Pp = L L^T and g_i = L^T c_i:
//       M = I + sum_i g_i g_i^T / D_b,i = K K^T        T = K^-1 L^T         P = T^T T        x = xp + T^T K^-1 sum_i g_i e_i / D_b,i
// (P = (Pp^-1 + C^T D_b^-1 C)^-1 and Pp C^T S = P C^T D_b^-1), and trace(C Pp C^T) = sum_i |g_i|^2: two Cholesky factorisations of
// r x r in registers per step, M with eigenvalues >= 1.  W2 needs no matrix square root either: trace sqrtm(S1^1/2 S2 S1^1/2) =
// sum sqrt(eig(T S2 T^T)) for S1 = T^T T, so the T of the step serves again.  Eigenvalues of a symmetric r x r: closed form at r = 1, 2,
// cyclic Jacobi at r = 3, 4 (a lane leaves the sweeps when its off-diagonal part is below 3e-17 of the diagonal, 10 sweeps at most);
// the same routine gives ||C - Ctrue||_2 = sqrt(lambda_max((C - Ctrue)^T (C - Ctrue))).  A W^2 that cancellation makes negative is 0.
//
// A lane whose pivot is not positive or whose s + eta is not finite and positive marks its replica and returns; the other lanes of
// its wave go on.  The state (C, X0, P0) crosses launches in device memory as float64, hence exactly: a run gives the same bits at
// every K.  The unit is compiled without floating-point contraction and writes its fused multiply-adds out, so that the shared and the
// own instance of a shape are the same arithmetic.
#include "psmf_host.h"        // Switches
#include "psmf_batch.h"       // EntryFail, open_device, plan_chunk, per-item slots, TimedLaunch, all_finite, replica_status

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace psmf {

constexpr int CONV_MAX_R = 4, CONV_MAX_D = 16, CONV_WG = 64;
constexpr int CONV_MAX_NT = CONV_MAX_R * (CONV_MAX_R + 1) / 2;
constexpr long long CONV_LAUNCH_STEPS = 1LL << 20;      // steps of a launch, at most (n * K)

// index of (i, j) in a symmetric matrix packed by rows of its lower triangle
__host__ __device__ constexpr int conv_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

struct ConvKalmanParams {
  int d, n, nser;
  size_t stride;          // of the replica-minor buffers: the chunk's replicas (1 with shared data)
  double Q[CONV_MAX_NT], Rd[CONV_MAX_D];
  const double* Y;        // series x n x d, time-major
  const double* Ctrue;    // series x d x r
  const double* x0;       // series x r
  const double* P0;       // series x r x r
  double* YT;             // n x d x stride, or null (shared data: Y is read where it lies)
  double* XkT;            // n x r x stride
  double* PkT;            // n x nt x stride
  double* XkOut;          // series x n x r, or null (shared data: XkT is that already)
  double* PkOut;          // series x n x nt, or null
  int* err;               // series: non-zero on entry = skip; set to 1 on a non-positive pivot
};

struct ConvParams {
  int d, n, nrep, n_iter, it0, nit, want_moments;
  size_t stride;
  double Q[CONV_MAX_NT], Rd[CONV_MAX_D];
  const double* Y;        // shared: n x d;  own: n x d x stride
  const double* Xk;       // shared: n x r;  own: n x r x stride
  const double* Pk;       // shared: n x nt; own: n x nt x stride
  const double* Ctrue;    // shared: d x r;  own: replicas x d x r
  const double *v, *qs, *rs;      // replicas
  double *C, *x0, *P0;    // replicas x (d x r | r | r x r): the state between launches and calls
  double *avW, *CerrI;    // replicas x n_iter
  double *Cit, *Sxy, *Sxx;        // replicas x n_iter x (d x r | r x d | nt), want_moments
  double *Xps, *Pps, *W, *Cerr;   // replicas x n x (r | nt | 1 | 1): the last iteration
  int* err;
};

// A = L L^T, packed; Li = 1 / diag(L).  false where a pivot is not positive (a NaN is not).
template <int R>
__device__ __forceinline__ bool conv_chol(const double (&A)[R * (R + 1) / 2], double (&L)[R * (R + 1) / 2], double (&Li)[R]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    double s = A[conv_tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) s = fma(-L[conv_tri(j, k)], L[conv_tri(j, k)], s);
    ok = ok && s > 0.0;
    const double dj = sqrt(s);
    Li[j] = 1.0 / dj;
    L[conv_tri(j, j)] = dj;
#pragma unroll
    for (int i = j + 1; i < R; ++i) {
      double v = A[conv_tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-L[conv_tri(i, k)], L[conv_tri(j, k)], v);
      L[conv_tri(i, j)] = v * Li[j];
    }
  }
  return ok;
}

// eigenvalues of a symmetric R x R matrix, packed, in no order
template <int R>
__device__ __forceinline__ void conv_eig(const double (&A)[R * (R + 1) / 2], double (&lam)[R]) {
  if constexpr (R == 1) {
    lam[0] = A[0];
  } else if constexpr (R == 2) {
    const double a = A[0], b = A[1], c = A[2];
    const double m = 0.5 * (a + c), h = 0.5 * (a - c), q = sqrt(fma(h, h, b * b));
    lam[0] = m + q;
    lam[1] = lam[0] > 0.0 ? fma(a, c, -(b * b)) / lam[0] : m - q;      // (the product of the two is the determinant)
  } else {
    double a[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) a[i][j] = A[conv_tri(i, j)];
#pragma unroll 1
    for (int sweep = 0; sweep < 10; ++sweep) {
      double off = 0.0, dg = 0.0;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        dg = fma(a[i][i], a[i][i], dg);
#pragma unroll
        for (int j = i + 1; j < R; ++j) off = fma(a[i][j], a[i][j], off);
      }
      if (!(off > 1e-33 * dg)) break;
#pragma unroll
      for (int p = 0; p < R; ++p)
#pragma unroll
        for (int q = p + 1; q < R; ++q) {
          const double apq = a[p][q];
          if (apq != 0.0) {
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
            const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
            a[p][p] = fma(-t, apq, a[p][p]);
            a[q][q] = fma(t, apq, a[q][q]);
            a[p][q] = 0.0;
            a[q][p] = 0.0;
#pragma unroll
            for (int k = 0; k < R; ++k)
              if (k != p && k != q) {
                const double akp = a[k][p], akq = a[k][q];
                const double np_ = fma(c, akp, -(s * akq)), nq_ = fma(s, akp, c * akq);
                a[k][p] = np_; a[p][k] = np_;
                a[k][q] = nq_; a[q][k] = nq_;
              }
          }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) lam[i] = a[i][i];
  }
}

// The measurement update of the header comment, for the rows i < d of C: e, sumR = sum_i r_scale R_i, trc = trace(C Pp C^T), T, the
// new x and P.  false where a pivot is not positive.
template <int R, int D>
__device__ __forceinline__ bool conv_update(int d, const double (&C)[D][R], const double (&Pp)[R * (R + 1) / 2], const double (&xp)[R],
                                            const double (&y)[D], const double (&Rd)[CONV_MAX_D], double rscale, double s, double (&e)[D],
                                            double& sumR, double& trc, double (&T)[R][R], double (&x)[R], double (&P)[R * (R + 1) / 2]) {
  constexpr int NT = R * (R + 1) / 2;
  double L[NT], Li[R], M[NT], K[NT], Ki[R], hL[R], z[R];
  bool ok = conv_chol<R>(Pp, L, Li);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    hL[k] = 0.0;
#pragma unroll
    for (int l = 0; l <= k; ++l) M[conv_tri(k, l)] = k == l ? 1.0 : 0.0;
  }
  sumR = 0.0;
  trc = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    e[i] = 0.0;
    if (i < d) {
      double pred = 0.0, g[R];
#pragma unroll
      for (int j = 0; j < R; ++j) pred = fma(C[i][j], xp[j], pred);
      e[i] = y[i] - pred;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        g[k] = 0.0;
#pragma unroll
        for (int j = k; j < R; ++j) g[k] = fma(L[conv_tri(j, k)], C[i][j], g[k]);
      }
      const double rd = Rd[i] * rscale, ri = 1.0 / (rd + s), rie = ri * e[i];
      sumR += rd;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        trc = fma(g[k], g[k], trc);
        hL[k] = fma(rie, g[k], hL[k]);
        const double rg = ri * g[k];
#pragma unroll
        for (int l = 0; l <= k; ++l) M[conv_tri(k, l)] = fma(rg, g[l], M[conv_tri(k, l)]);
      }
    }
  }
  ok = conv_chol<R>(M, K, Ki) && ok;
#pragma unroll
  for (int k = 0; k < R; ++k) {      // z = K^-1 hL
    double v = hL[k];
#pragma unroll
    for (int l = 0; l < k; ++l) v = fma(-K[conv_tri(k, l)], z[l], v);
    z[k] = v * Ki[k];
  }
#pragma unroll
  for (int c = 0; c < R; ++c)        // T = K^-1 L^T, column c
#pragma unroll
    for (int k = 0; k < R; ++k) {
      double v = k <= c ? L[conv_tri(c, k)] : 0.0;
#pragma unroll
      for (int l = 0; l < k; ++l) v = fma(-K[conv_tri(k, l)], T[l][c], v);
      T[k][c] = v * Ki[k];
    }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    double v = xp[j];
#pragma unroll
    for (int k = 0; k < R; ++k) v = fma(T[k][j], z[k], v);
    x[j] = v;
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) q = fma(T[k][j], T[k][i], q);
      P[conv_tri(j, i)] = q;
    }
  }
  return ok;
}

// W2^2 of N(x, P = T^T T) and N(xk, Pk), not below 0
template <int R>
__device__ __forceinline__ double conv_w2sq(const double (&T)[R][R], const double (&x)[R], const double (&P)[R * (R + 1) / 2],
                                            const double (&xk)[R], const double (&Pk)[R * (R + 1) / 2]) {
  constexpr int NT = R * (R + 1) / 2;
  double acc = 0.0, A[NT], lam[R], B[R][R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double dm = x[j] - xk[j];
    acc = fma(dm, dm, acc);
  }
#pragma unroll
  for (int j = 0; j < R; ++j) acc += P[conv_tri(j, j)] + Pk[conv_tri(j, j)];
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < R; ++m) v = fma(T[k][m], Pk[conv_tri(m, j)], v);
      B[k][j] = v;
    }
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < R; ++j) v = fma(B[k][j], T[l][j], v);
      A[conv_tri(k, l)] = v;
    }
  conv_eig<R>(A, lam);
  double roots = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) roots += sqrt(fmax(lam[k], 0.0));
  return fmax(acc - 2.0 * roots, 0.0);
}

// ||C - Ctrue||_2; element (i, j) of Ctrue at Ct[i * R + j]
template <int R, int D>
__device__ __forceinline__ double conv_cerr(int d, const double (&C)[D][R], const double* __restrict__ Ct) {
  constexpr int NT = R * (R + 1) / 2;
  double A[NT], lam[R];
#pragma unroll
  for (int k = 0; k < NT; ++k) A[k] = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < d) {
      double dl[R];
#pragma unroll
      for (int j = 0; j < R; ++j) dl[j] = C[i][j] - Ct[i * R + j];
#pragma unroll
      for (int k = 0; k < R; ++k)
#pragma unroll
        for (int l = 0; l <= k; ++l) A[conv_tri(k, l)] = fma(dl[k], dl[l], A[conv_tri(k, l)]);
    }
  conv_eig<R>(A, lam);
  double top = lam[0];
#pragma unroll
  for (int k = 1; k < R; ++k) top = fmax(top, lam[k]);
  return sqrt(fmax(top, 0.0));
}

template <int R, int D>
__global__ __launch_bounds__(CONV_WG) void psmf_conv_kalman_kernel(ConvKalmanParams p) {
  constexpr int NT = R * (R + 1) / 2;
  const int b = blockIdx.x * CONV_WG + threadIdx.x;
  if (b >= p.nser) return;
  if (p.err[b] != 0) return;
  const int d = p.d, n = p.n;
  const size_t st = p.stride;
  const double* __restrict__ Y = p.Y + (size_t)b * n * d;
  const double* __restrict__ Ct = p.Ctrue + (size_t)b * d * R;
  double C[D][R], x[R], P[NT];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) C[i][j] = i < d ? Ct[i * R + j] : 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    x[j] = p.x0[(size_t)b * R + j];
#pragma unroll
    for (int i = 0; i <= j; ++i) P[conv_tri(j, i)] = p.P0[(size_t)b * R * R + j * R + i];
  }
  for (int t = 0; t < n; ++t) {
    double Pp[NT], y[D], e[D], T[R][R], xn[R], Pn[NT], sumR, trc;
#pragma unroll
    for (int k = 0; k < NT; ++k) Pp[k] = P[k] + p.Q[k];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      y[i] = 0.0;
      if (i < d) {
        y[i] = Y[(size_t)t * d + i];
        if (p.YT) p.YT[((size_t)t * d + i) * st + b] = y[i];
      }
    }
    if (!conv_update<R, D>(d, C, Pp, x, y, p.Rd, 1.0, 0.0, e, sumR, trc, T, xn, Pn)) {
      p.err[b] = 1;
      return;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      x[j] = xn[j];
      p.XkT[((size_t)t * R + j) * st + b] = xn[j];
      if (p.XkOut) p.XkOut[((size_t)b * n + t) * R + j] = xn[j];
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      P[k] = Pn[k];
      p.PkT[((size_t)t * NT + k) * st + b] = Pn[k];
      if (p.PkOut) p.PkOut[((size_t)b * n + t) * NT + k] = Pn[k];
    }
  }
}

template <int R, int D, bool OWN>
__global__ __launch_bounds__(CONV_WG) void psmf_conv_sweep_kernel(ConvParams p) {
  constexpr int NT = R * (R + 1) / 2;
  // Sxy = sum_t x_t y_t^T, R x D sums: registers, but at r = 4 under the capacity 16, where the 64 of them would push the instance
  // into scratch memory: there they live in LDS, element-major and lane-minor (consecutive lanes, consecutive words)
  constexpr bool LDS_SXY = R * D > 48;
  __shared__ double s_sxy[LDS_SXY ? R * D * CONV_WG : 1];
  double* const my_sxy = s_sxy + threadIdx.x;
  const int b = blockIdx.x * CONV_WG + threadIdx.x;
  if (b >= p.nrep) return;
  if (p.err[b] != 0) return;
  const int d = p.d, n = p.n;
  const size_t st = OWN ? p.stride : 1, me = OWN ? (size_t)b : 0;
  const double* __restrict__ Y = p.Y + me;
  const double* __restrict__ Xk = p.Xk + me;
  const double* __restrict__ Pk = p.Pk + me;
  const double* __restrict__ Ct = p.Ctrue + (OWN ? (size_t)b * d * R : 0);
  double* Cst = p.C + (size_t)b * d * R;
  const double v0 = p.v[b], qs = p.qs[b], rs = p.rs[b], inv_d = 1.0 / d, inv_n = 1.0 / n;
  double C[D][R], x0[R], P0[NT], Qs[NT];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) C[i][j] = i < d ? Cst[i * R + j] : 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    x0[j] = p.x0[(size_t)b * R + j];
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      P0[conv_tri(j, i)] = p.P0[(size_t)b * R * R + j * R + i];
      Qs[conv_tri(j, i)] = qs * p.Q[conv_tri(j, i)];
    }
  }
  for (int it = 0; it < p.nit; ++it) {
    const size_t iter = (size_t)b * p.n_iter + p.it0 + it;      // this iteration's place in the per-iteration outputs
    const bool last = p.it0 + it == p.n_iter - 1;
    double V[NT], xp[R], Pv[NT], x1[R], P1[NT], Sxy[LDS_SXY ? 1 : R][LDS_SXY ? 1 : D], Sxx[NT], sumW = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      xp[j] = x0[j];
      x1[j] = x0[j];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        if constexpr (LDS_SXY) my_sxy[(j * D + i) * CONV_WG] = 0.0;
        else Sxy[j][i] = 0.0;
      }
#pragma unroll
      for (int i = 0; i <= j; ++i) {
        V[conv_tri(j, i)] = i == j ? v0 : 0.0;
        Pv[conv_tri(j, i)] = P0[conv_tri(j, i)];
        P1[conv_tri(j, i)] = P0[conv_tri(j, i)];
        Sxx[conv_tri(j, i)] = 0.0;
      }
    }
    for (int t = 0; t < n; ++t) {
      double Pp[NT], w[R], y[D], e[D], T[R][R], x[R], P[NT], sumR, trc, s = 0.0;
#pragma unroll
      for (int k = 0; k < NT; ++k) Pp[k] = Pv[k] + Qs[k];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) q = fma(V[conv_tri(j, k)], xp[k], q);
        w[j] = q;
      }
#pragma unroll
      for (int j = 0; j < R; ++j) s = fma(xp[j], w[j], s);
#pragma unroll
      for (int i = 0; i < D; ++i) y[i] = i < d ? Y[((size_t)t * d + i) * st] : 0.0;
      const bool ok = conv_update<R, D>(d, C, Pp, xp, y, p.Rd, rs, s, e, sumR, trc, T, x, P);
      const double N = s + (sumR + trc) * inv_d;
      if (!(ok && N > 0.0 && N < INFINITY)) {
        p.err[b] = 1;
        return;
      }
      const double inv_N = 1.0 / N;
#pragma unroll
      for (int i = 0; i < D; ++i)
        if (i < d) {
          const double coef = e[i] * inv_N;
#pragma unroll
          for (int j = 0; j < R; ++j) C[i][j] = fma(coef, w[j], C[i][j]);
        }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const double wj = w[j] * inv_N;
#pragma unroll
        for (int i = 0; i <= j; ++i) V[conv_tri(j, i)] = fma(-wj, w[i], V[conv_tri(j, i)]);
      }
      double Wt = 0.0;
      if (t >= 1) {
        double xk[R], pk[NT];
#pragma unroll
        for (int j = 0; j < R; ++j) xk[j] = Xk[((size_t)t * R + j) * st];
#pragma unroll
        for (int k = 0; k < NT; ++k) pk[k] = Pk[((size_t)t * NT + k) * st];
        Wt = sqrt(conv_w2sq<R>(T, x, P, xk, pk));
        sumW += Wt;
      } else {
#pragma unroll
        for (int j = 0; j < R; ++j) x1[j] = x[j];
#pragma unroll
        for (int k = 0; k < NT; ++k) P1[k] = P[k];
      }
      if (p.want_moments) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
#pragma unroll
          for (int i = 0; i < D; ++i) {
            if constexpr (LDS_SXY) my_sxy[(j * D + i) * CONV_WG] = fma(x[j], y[i], my_sxy[(j * D + i) * CONV_WG]);
            else Sxy[j][i] = fma(x[j], y[i], Sxy[j][i]);
          }
#pragma unroll
          for (int i = 0; i <= j; ++i) Sxx[conv_tri(j, i)] = fma(x[j], x[i], Sxx[conv_tri(j, i)]);
        }
      }
      if (last) {
        const size_t row = (size_t)b * n + t;
#pragma unroll
        for (int j = 0; j < R; ++j) p.Xps[row * R + j] = x[j];
#pragma unroll
        for (int k = 0; k < NT; ++k) p.Pps[row * NT + k] = P[k];
        p.W[row] = Wt;
        p.Cerr[row] = conv_cerr<R, D>(d, C, Ct);
      }
#pragma unroll
      for (int j = 0; j < R; ++j) xp[j] = x[j];
#pragma unroll
      for (int k = 0; k < NT; ++k) Pv[k] = P[k];
    }
    const double avw = sumW * inv_n, cerr = conv_cerr<R, D>(d, C, Ct);
    if (!(avw < INFINITY && cerr < INFINITY)) {
      p.err[b] = 1;
      return;
    }
    p.avW[iter] = avw;
    p.CerrI[iter] = cerr;
    if (p.want_moments) {
#pragma unroll
      for (int i = 0; i < D; ++i)
        if (i < d) {
#pragma unroll
          for (int j = 0; j < R; ++j) {
            p.Cit[(iter * d + i) * R + j] = C[i][j];
            if constexpr (LDS_SXY) p.Sxy[(iter * R + j) * d + i] = my_sxy[(j * D + i) * CONV_WG];
            else p.Sxy[(iter * R + j) * d + i] = Sxy[j][i];
          }
        }
#pragma unroll
      for (int k = 0; k < NT; ++k) p.Sxx[iter * NT + k] = Sxx[k];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) x0[j] = x1[j];
#pragma unroll
    for (int k = 0; k < NT; ++k) P0[k] = P1[k];
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < d) {
#pragma unroll
      for (int j = 0; j < R; ++j) Cst[i * R + j] = C[i][j];
    }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    p.x0[(size_t)b * R + j] = x0[j];
#pragma unroll
    for (int i = 0; i < R; ++i) p.P0[(size_t)b * R * R + j * R + i] = P0[conv_tri(j, i)];
  }
}

namespace {

// the kernels of a shape: the Kalman pass, the sweep over shared data, the sweep over own data
struct ConvInstance { const void *kalman, *shared, *own; };
template <int R, int D> constexpr ConvInstance conv_instance() {
  return {(const void*)psmf_conv_kalman_kernel<R, D>, (const void*)psmf_conv_sweep_kernel<R, D, false>, (const void*)psmf_conv_sweep_kernel<R, D, true>};
}
constexpr int kConvCaps[3] = {4, 8, 16};
const ConvInstance kConvTable[CONV_MAX_R][3] = {      // [r - 1][capacity]
    {conv_instance<1, 4>(), conv_instance<1, 8>(), conv_instance<1, 16>()},
    {conv_instance<2, 4>(), conv_instance<2, 8>(), conv_instance<2, 16>()},
    {conv_instance<3, 4>(), conv_instance<3, 8>(), conv_instance<3, 16>()},
    {conv_instance<4, 4>(), conv_instance<4, 8>(), conv_instance<4, 16>()},
};

int conv_run(const psmf_conv_config* cfg, const double* Y, const double* Ctrue, const double* Q, const double* Rdiag, const double* x0k,
             const double* P0k, const double* v, const double* q_scale, const double* r_scale, double* C, double* x0, double* P0,
             double* Xk, double* Pk, double* avW, double* CerrI, double* C_iter, double* Sxy, double* Sxx, double* Xps, double* Pps,
             double* W, double* Cerr, int32_t* status, float* elapsed_ms) {
  const EntryFail fail{"psmf_conv_run"};
  const Switches sw;      // no handle here: read at entry, on every call
  if (!cfg || !Y || !Ctrue || !Q || !Rdiag || !x0k || !P0k || !v || !q_scale || !r_scale || !C || !x0 || !P0 || !Xk || !Pk || !avW || !CerrI ||
      !Xps || !Pps || !W || !Cerr)
    return fail(PSMF_ERR_ARG, "null argument");
  if (cfg->abi_version != PSMF_ABI_VERSION) return fail(PSMF_ERR_ARG, "ABI version mismatch");
  const int d = cfg->d, n = cfg->n, r = cfg->r, B = cfg->batch, n_iter = cfg->n_iter;
  const bool own = cfg->own_data != 0, moments = cfg->want_moments != 0;
  if (r < 1 || r > CONV_MAX_R) return fail(PSMF_ERR_ARG, "need 1 <= r <= 4 (the r x r state lives in a lane's registers; r = " + std::to_string(r) + ")");
  if (d < r || d > CONV_MAX_D)
    return fail(PSMF_ERR_ARG, "need r <= d <= 16 (C lives in a lane's registers, and d < r is not identifiable; d = " + std::to_string(d) + ", r = " + std::to_string(r) + ")");
  if (n < 2) return fail(PSMF_ERR_ARG, "need n >= 2 (n = " + std::to_string(n) + ")");
  if (n_iter < 1) return fail(PSMF_ERR_ARG, "need n_iter >= 1 (n_iter = " + std::to_string(n_iter) + ")");
  if (B < 1) return fail(PSMF_ERR_ARG, "need batch >= 1 (batch = " + std::to_string(B) + ")");
  if (moments && (!C_iter || !Sxy || !Sxx)) return fail(PSMF_ERR_ARG, "want_moments needs C_iter, Sxy and Sxx");
  if (sw.conv_chunk < 0 || sw.conv_iters < 0) return fail(PSMF_ERR_ARG, "PSMF_CONV_CHUNK and PSMF_CONV_ITERS must be >= 0 (0 = chosen by the library)");
  const int nt = r * (r + 1) / 2;
  for (int i = 0; i < d; ++i)
    if (!(Rdiag[i] > 0.0) || !std::isfinite(Rdiag[i])) return fail(PSMF_ERR_ARG, "need a finite diagonal R > 0 (row " + std::to_string(i) + ")");
  if (!all_finite(Q, (size_t)r * r)) return fail(PSMF_ERR_ARG, "Q must be finite");
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < i; ++j)
      if (Q[i * r + j] != Q[j * r + i]) return fail(PSMF_ERR_ARG, "Q must be symmetric");

  // what makes a replica fail before it starts: a non-finite entry in what is its own
  const size_t nY = (size_t)n * d, nC = (size_t)d * r, nX = (size_t)n * r, nP = (size_t)n * nt, nR = r, nRR = (size_t)r * r, nIt = n_iter, nN = n;
  std::vector<int> herr(B, 0);
  for (int b = 0; b < B; ++b) {
    bool fin = all_finite(C + b * nC, nC) && all_finite(x0 + b * nR, nR) && all_finite(P0 + b * nRR, nRR) && all_finite(v + b, 1) &&
               all_finite(q_scale + b, 1) && all_finite(r_scale + b, 1) && r_scale[b] > 0.0 && q_scale[b] >= 0.0;
    if (own) fin = fin && all_finite(Y + b * nY, nY) && all_finite(Ctrue + b * nC, nC) && all_finite(x0k + b * nR, nR) && all_finite(P0k + b * nRR, nRR);
    herr[b] = fin ? 0 : 1;
  }
  if (!own && !(all_finite(Y, nY) && all_finite(Ctrue, nC) && all_finite(x0k, nR) && all_finite(P0k, nRR)))
    return fail(PSMF_ERR_ARG, "the shared Y, Ctrue, x0_kalman and P0_kalman must be finite");
  PSMF_TRY(open_device(fail, cfg->device));

  const size_t nMom = moments ? nIt : 0, nOwn = own ? 1 : 0, nShared = own ? 0 : 1;
  const size_t per_replica = (2 * nC + 3 + nR + nRR + 2 * nIt + nMom * (2 * nC + nt) + nX + nP + 2 * nN + nOwn * (2 * nY + nC + nR + nRR + 2 * (nX + nP))) * sizeof(double) +
                             sizeof(int);
  const size_t shared_bytes = nShared * (nY + nC + nR + nRR + nX + nP) * sizeof(double) + sizeof(int);
  int chunk = 0;      // replicas per chunk (PSMF_CONV_CHUNK: smaller chunks than memory asks for)
  PSMF_TRY(plan_chunk(fail, B, shared_bytes, per_replica, kNoItemCap, sw.conv_chunk, "replica", &chunk));
  long long K = std::max(1LL, CONV_LAUNCH_STEPS / n);      // iterations per launch (PSMF_CONV_ITERS: fewer)
  if (sw.conv_iters > 0) K = std::min<long long>(K, sw.conv_iters);

  Dev<double> dY, dCt, dX0k, dP0k, dYT, dXkT, dPkT, dXk, dPk, dV, dQs, dRs, dC, dx0, dP0, dAvW, dCerrI, dCit, dSxy, dSxx, dXps, dPps, dW, dCerr;
  Dev<int> dErr, dKerr;
  int kerr = 0;
  TimedLaunch timed;
  // with shared data XkT / PkT (stride 1) are what is returned; with own data the Kalman pass writes both layouts
  const auto items = std::make_tuple(      // buffer, filled from, read back to, elements per replica, cleared for every chunk
      item_slot(dY, Y, nullptr, nOwn * nY), item_slot(dCt, Ctrue, nullptr, nOwn * nC), item_slot(dX0k, x0k, nullptr, nOwn * nR),
      item_slot(dP0k, P0k, nullptr, nOwn * nRR), item_slot(dYT, nullptr, nullptr, nOwn * nY), item_slot(dXkT, nullptr, nullptr, nOwn * nX),
      item_slot(dPkT, nullptr, nullptr, nOwn * nP), item_slot(dXk, nullptr, Xk, nOwn * nX, true), item_slot(dPk, nullptr, Pk, nOwn * nP, true),
      item_slot(dV, v, nullptr, 1), item_slot(dQs, q_scale, nullptr, 1), item_slot(dRs, r_scale, nullptr, 1),
      item_slot(dC, C, C, nC), item_slot(dx0, x0, x0, nR), item_slot(dP0, P0, P0, nRR), item_slot(dErr, herr.data(), herr.data(), 1),
      item_slot(dAvW, nullptr, avW, nIt, true), item_slot(dCerrI, nullptr, CerrI, nIt, true), item_slot(dCit, nullptr, C_iter, nMom * nC, true),
      item_slot(dSxy, nullptr, Sxy, nMom * nC, true), item_slot(dSxx, nullptr, Sxx, nMom * nt, true), item_slot(dXps, nullptr, Xps, nX, true),
      item_slot(dPps, nullptr, Pps, nP, true), item_slot(dW, nullptr, W, nN, true), item_slot(dCerr, nullptr, Cerr, nN, true));
  const auto shared = std::make_tuple(      // what every chunk shares, filled once
      slot(dY, Y, nullptr, nShared * nY), slot(dCt, Ctrue, nullptr, nShared * nC), slot(dX0k, x0k, nullptr, nShared * nR),
      slot(dP0k, P0k, nullptr, nShared * nRR), slot(dXkT, nullptr, Xk, nShared * nX), slot(dPkT, nullptr, Pk, nShared * nP),
      slot(dKerr, &kerr, &kerr, 1));
  PSMF_TRY(alloc_all(fail, shared));
  PSMF_TRY(alloc_items(fail, items, chunk));
  PSMF_TRY(copy_in_all(fail, shared));
  PSMF_TRY(timed.create(fail));

  int cap = 0;
  while (kConvCaps[cap] < d) ++cap;
  const ConvInstance& inst = kConvTable[r - 1][cap];
  ConvKalmanParams kp;
  ConvParams cp;
  kp.d = cp.d = d; kp.n = cp.n = n;
  for (int i = 0; i < CONV_MAX_D; ++i) kp.Rd[i] = cp.Rd[i] = i < d ? Rdiag[i] : 1.0;
  for (int k = 0; k < CONV_MAX_NT; ++k) kp.Q[k] = cp.Q[k] = 0.0;
  for (int i = 0; i < r; ++i)
    for (int j = 0; j <= i; ++j) kp.Q[conv_tri(i, j)] = cp.Q[conv_tri(i, j)] = Q[i * r + j];
  kp.Y = dY; kp.Ctrue = dCt; kp.x0 = dX0k; kp.P0 = dP0k; kp.XkT = dXkT; kp.PkT = dPkT;
  kp.YT = own ? dYT.get() : nullptr; kp.XkOut = own ? dXk.get() : nullptr; kp.PkOut = own ? dPk.get() : nullptr;
  kp.err = own ? dErr.get() : dKerr.get();
  cp.n_iter = n_iter; cp.want_moments = moments;
  cp.Y = own ? dYT.get() : dY.get(); cp.Xk = dXkT; cp.Pk = dPkT; cp.Ctrue = dCt; cp.v = dV; cp.qs = dQs; cp.rs = dRs;
  cp.C = dC; cp.x0 = dx0; cp.P0 = dP0; cp.avW = dAvW; cp.CerrI = dCerrI; cp.Cit = dCit; cp.Sxy = dSxy; cp.Sxx = dSxx;
  cp.Xps = dXps; cp.Pps = dPps; cp.W = dW; cp.Cerr = dCerr; cp.err = dErr;

  float total_ms = 0.0f;
  if (!own) {      // the one Kalman pass of the call: a batch of one
    kp.nser = 1; kp.stride = 1;
    float ms = 0.0f;
    PSMF_TRY(timed.start(fail));
    PSMF_TRY(launch(fail, inst.kalman, dim3(1), dim3(CONV_WG), &kp, 0));
    PSMF_TRY(timed.finish(fail, &ms));
    total_ms += ms;
    PSMF_TRY(copy_out_all(fail, shared));
    if (kerr != 0) return fail(PSMF_ERR_NUMERIC, "the Kalman pass lost positive definiteness (R + Ctrue P Ctrue^T)");
  }
  for (int s0 = 0; s0 < B; s0 += chunk) {      // s0: the chunk's first replica = its element offset in the host arrays, per replica
    const size_t ns = std::min(chunk, B - s0);
    const dim3 grid((unsigned)((ns + CONV_WG - 1) / CONV_WG));
    PSMF_TRY(fill_items(fail, items, s0, ns));
    PSMF_TRY(timed.start(fail));
    if (own) {
      kp.nser = (int)ns; kp.stride = ns;
      PSMF_TRY(launch(fail, inst.kalman, grid, dim3(CONV_WG), &kp, 0));
    }
    cp.nrep = (int)ns; cp.stride = own ? ns : 1;
    for (long long it0 = 0; it0 < n_iter; it0 += K) {
      cp.it0 = (int)it0; cp.nit = (int)std::min<long long>(K, n_iter - it0);
      PSMF_TRY(launch(fail, own ? inst.own : inst.shared, grid, dim3(CONV_WG), &cp, 0));
    }
    float ms = 0.0f;
    PSMF_TRY(timed.finish(fail, &ms));
    total_ms += ms;
    PSMF_TRY(read_items(fail, items, s0, ns));
  }
  if (elapsed_ms) *elapsed_ms = total_ms;
  // Per-replica outcome, as psmf_ssm_run; the other replicas are untouched by a bad one.
  return replica_status(fail, B, status, [&](int b) { return herr[b] != 0; }, [](int b) {
    return "non-finite input, a non-finite state or a non-positive pivot in replica " + std::to_string(b);
  });
}

}  // namespace
}  // namespace psmf

extern "C" int psmf_conv_run(const psmf_conv_config* cfg, const double* Y, const double* Ctrue, const double* Q, const double* Rdiag,
                             const double* x0k, const double* P0k, const double* v, const double* q_scale, const double* r_scale, double* C,
                             double* x0, double* P0, double* Xk, double* Pk, double* avW, double* CerrI, double* C_iter, double* Sxy, double* Sxx,
                             double* Xps, double* Pps, double* W, double* Cerr, int32_t* status, float* elapsed_ms) {
  return psmf::conv_run(cfg, Y, Ctrue, Q, Rdiag, x0k, P0k, v, q_scale, r_scale, C, x0, P0, Xk, Pk, avW, CerrI, C_iter, Sxy, Sxx, Xps, Pps, W, Cerr,
                        status, elapsed_ms);
}
