// GPU-box diagnostic: per-phase cycles of the two-group block filter (stamps via PSMF_BLK_STAMPS).
#define PSMF_BLK_STAMPS 1
#include "../rpsmf_amd/csrc/psmf_blk34.hip"
#include <cstdio>
#include <vector>
#include <cmath>
using namespace psmf;
int main() {
  const int r = 32, nb = 32;
  DevState* st; hipMalloc((void**)&st, sizeof(DevState)); hipMemset(st, 0, sizeof(DevState));
  std::vector<double> I(r * r, 0.0), Q(r * r, 0.0); for (int i = 0; i < r; ++i) { I[i * r + i] = 1.0; Q[i * r + i] = 0.1; }
  hipMemcpy(st->V, I.data(), r * r * 8, hipMemcpyHostToDevice); hipMemcpy(st->P, I.data(), r * r * 8, hipMemcpyHostToDevice);
  hipMemcpy(st->Q, Q.data(), r * r * 8, hipMemcpyHostToDevice);
  double one = 1.0; hipMemcpy(&st->rho, &one, 8, hipMemcpyHostToDevice);
  // a filter-like Gram: Z = [C0 | y_1 .. y_32], y_t = Ctrue x_t + noise, x_t a smooth trajectory
  const int dd = 4096;
  std::vector<double> Z((size_t)dd * RB), K(RB * RB, 0.0), Ct((size_t)dd * r);
  unsigned s = 1; auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0 - 0.5; };
  for (auto& c : Ct) c = 2.0 * rnd();
  for (int i = 0; i < dd; ++i) for (int c = 0; c < r; ++c) Z[(size_t)i * RB + c] = 0.2 * rnd();
  for (int t = 0; t < nb; ++t) {
    std::vector<double> x(r); for (int c = 0; c < r; ++c) x[c] = std::cos(0.01 * (c + 1) * (t + 1) + c);
    for (int i = 0; i < dd; ++i) { double acc = 0; for (int c = 0; c < r; ++c) acc += Ct[(size_t)i * r + c] * x[c]; Z[(size_t)i * RB + r + t] = acc + 0.6 * rnd(); }
  }
  for (int a = 0; a < RB; ++a) for (int c = 0; c < RB; ++c) { double acc = 0; for (int i = 0; i < dd; ++i) acc += Z[(size_t)i * RB + a] * Z[(size_t)i * RB + c]; K[a * RB + c] = acc; }
  double *dK, *dA, *dB, *dKp; hipMalloc((void**)&dK, RB * RB * 8); hipMalloc((void**)&dA, RB * RM * 8); hipMalloc((void**)&dB, RB * RB * 8); hipMalloc((void**)&dKp, 1 << 20);
  hipMemcpy(dK, K.data(), RB * RB * 8, hipMemcpyHostToDevice);
  BlockParams b{}; b.sp.st = st; b.sp.r = r; b.sp.d = getenv("D") ? atoi(getenv("D")) : 4096; b.sp.d_local = b.sp.d; b.sp.use_ns = 1; b.sp.coef_update = 1; b.sp.eta_full = 1; b.sp.pbar_predict = 1;
  b.sp.alpha = b.sp.beta = 1.0; b.sp.ns_predict = getenv("PRED") ? atoi(getenv("PRED")) : 7; b.sp.ns_far2 = 0.09; b.sp.ns_tol2 = getenv("TOL") ? atof(getenv("TOL")) * atof(getenv("TOL")) : 9e-14; b.K = dK; b.Acoef = dA; b.Bcoef = dB; b.Kpart = dKp; b.k0 = 0; b.nb = nb;
  const size_t lds = blk_filter3_lds_bytes();
  hipFuncSetAttribute((const void*)psmf_blk_filter3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  for (int it = 0; it < 2; ++it) { psmf_blk_filter3<<<1, F3_NT, lds>>>(b); hipDeviceSynchronize(); }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0); psmf_blk_filter3<<<1, F3_NT, lds>>>(b); hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  for (int it = 0; it < 40; ++it) { psmf_blk_filter3<<<1, F3_NT, lds>>>(b); }   // carry the state: steady regime
  hipDeviceSynchronize();
  hipEventRecord(e0); psmf_blk_filter3<<<1, F3_NT, lds>>>(b); hipEventRecord(e1); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
  hipMemset(dKp, 0, 4096); psmf_blk_filter3<<<1, F3_NT, lds>>>(b); hipDeviceSynchronize();
  unsigned long long h[8 * 12], cnt[16]; hipMemcpy(h, dKp, sizeof(h), hipMemcpyDeviceToHost); hipMemcpy(cnt, reinterpret_cast<unsigned long long*>(dKp) + 200, sizeof(cnt), hipMemcpyDeviceToHost);
  printf("NS converged on %llu steps, sweep on %llu; residual evaluations by iteration:", cnt[0], cnt[1]); for (int q = 2; q < 10; ++q) printf(" %llu", cnt[q]); printf("; mean initial ||R|| = %.3f\n", 1e-6 * cnt[12] / (double)(cnt[2] ? cnt[2] : 1));
  const char* nm[10] = {"phase 0 (idle)", "barrier waits", "phase 1 (M, it 0)", "phase 2 (it 1, G)", "further iterations", "phase F", "phase 0: W fill", "phase 0: traces", "-", "-"};
  printf("block of %d steps: %.1f us = %.2f us/step; err flag field k=%d\n", nb, ms * 1e3, ms * 1e3 / nb, 0);
  for (int w : {0, 2, 4, 5, 7}) { printf("wave %d (%s):\n", w, w < 2 ? "X" : (w < 4 ? "Y" : "V: phase 0 | barrier waits | phase 1 | phase 2 | to BF")); for (int q = 0; q < 10; ++q) printf("   %-22s %7.0f cycles/step\n", nm[q], (double)h[w * 12 + q] / nb); }
  // arrival profile: cycles per step from the release of a barrier to the wave's arrival at the next one (its own work in that
  // phase; the wave with the largest figure is the one the barrier waits for).  Inversion waves: B1 <- phase 0 (stamps 6 + 7),
  // B2 <- phase 1 (2), BF <- phase 2, further iterations, phase F (3 + 4 + 5); vector waves: 0 | 2 | 3 + 4.  Stamp 1 = all waits.
  printf("arrival (cycles per step)   BF->B1   B1->B2   B2->BF     waits\n");
  for (int w = 0; w < 8; ++w) {
    const unsigned long long* t = h + w * 12;
    const double p0 = w < 4 ? t[6] + t[7] : t[0], p1 = t[2], p2 = w < 4 ? t[3] + t[4] + t[5] : t[3] + t[4];
    printf("  wave %d (%s)            %8.0f %8.0f %8.0f  %8.0f\n", w, w < 2 ? "X" : (w < 4 ? "Y" : "V"), p0 / nb, p1 / nb, p2 / nb, (double)t[1] / nb);
  }
  return 0;
}
