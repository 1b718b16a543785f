// Blocked engine: what its kernels share -- the parameter block, the sizes, the device-flag hand-off and the K assembly.
// Defines no kernel (those are in psmf_block.hip, psmf_bulk.hip and psmf_blk*.hip), so any translation unit may include it.
#pragma once
#include "psmf_device.h"

namespace psmf {

// per-phase cycle accumulation for tools/blk_prof.hip (PSMF_BLK_STAMPS); no-ops in the product
#ifdef PSMF_BLK_STAMPS
#define BLK_T0() unsigned long long bt_[12] = {0,0,0,0,0,0,0,0,0,0,0,0}, bl_, bn_; { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(bl_) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
#define BLK_T(n) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(bn_) :: "memory"); __builtin_amdgcn_sched_barrier(0); bt_[n] += bn_ - bl_; bl_ = bn_; }
#define BLK_COUNT(i, v) if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(b.Kpart)[200 + (i)] += (v);
#define BLK_TOUT() if ((threadIdx.x & 63) == 0) for (int q_ = 0; q_ < 12; ++q_) reinterpret_cast<unsigned long long*>(b.Kpart)[(threadIdx.x >> 6) * 12 + q_] = bt_[q_];
#else
#define BLK_T0()
#define BLK_T(n)
#define BLK_COUNT(i, v)
#define BLK_TOUT()
#endif

constexpr int RB = 64;           // r + B, padded coefficient dimension (r <= 32)
constexpr int RS = RM / 2 + 1;   // LDS row stride of the RB x r coefficient matrices (odd: lane = row reads are conflict-free)
constexpr int BLK_GRAM_WG = 256; // workgroups (= partials) of the block Gram
constexpr int XGB = 64;          // column capacity of the cross-Gram (>= block length)
constexpr int BLK_TH_CAP = 2304; // theta / gradient sums of at most this many parameters live in LDS during a block (FourierBasis N = 1 at r = 32: 2176; 147 KB of LDS in all)

struct BlockParams {
  StepParams sp;
  double* Kpart;      // BLK_GRAM_WG x RB*RB
  double* K;          // RB x RB
  double* Acoef;      // RB x r   (A_nb)
  double* Bcoef;      // RB x RB  (column j = b_j, stored [j][m])
  long long k0;       // first step of the block is k0 + 1 (0-based series row k0)
  int nb;             // steps in this block
  int gram_rows;      // rows per Gram workgroup
  // pipelined blocks: K of this block is ASSEMBLED from the previous block instead of read from K:
  //   K[0:r,0:r] = G (tracked), K[0:r, r+q] = Aprev^T XG[0:RB, q], K[r+q, r+q'] = XG[RB+q, q']
  // with XG = [Z_prev^T Y ; Y^T Y] computed off the critical path (psmf_blk_xgram_mfma).
  int assemble;
  const double* XG;       // (RB + XGB) x XGB
  const double* Aprev;    // RB x r: coefficient matrix at the end of the previous block
  double* XGpart;         // BLK_GRAM_WG x (RB + XGB) * XGB
  long long k1;           // xgram: first row of the NEXT block in the series
  int nb1;                // xgram: steps of the next block
  // device-flag hand-off of the pipelined blocks (nullptr: the host orders the kernels with events):
  //   flags[0] = xg_seq   highest block sequence number whose K / cross-Gram is complete      (set on the bulk stream)
  //   flags[1] = filt_seq number of blocks whose filter kernel has finished                   (set by the NEXT filter kernel)
  //   flags[2] = abort    a wait timed out
  long long* flags;
  long long seq;          // this block's sequence number
  int last;               // filter3: last block of the run -> also write the row-major r x r state (DevState)
  // chain (filter3): ONE launch advances `chain` consecutive blocks of `chain_B` steps (the last one may be shorter, the
  // run ends at chain_kend); block j of the launch uses slot j & 1 of the ping-pong buffers below, sequence number seq + j,
  // and is assembled from block j - 1 (j > 0).  See psmf_blk_filter3.
  int chain;
  int chain_B;
  long long chain_kend;
  double* Acoef0;         // 2 x RB x RM
  double* Bcoef0;         // 2 x RB x RB
  const double* XG0;      // 2 x (RB + XGB) x XGB
  int carry;              // filter3, chain > 1: blocks hand the r x r state on in LDS; DevState gets it when the launch ends (PSMF_CHAIN_CARRY)
  int xg_ahead;           // filter3, carry: a fast hand-off fetches the next block's cross-Gram in front of its store drain (PSMF_XG_AHEAD)
  int dual6;              // psmf_blk_filter6: random walk, Q = q I, full filter, no schedules -> the two inversions of a step side by side
};

// ---- hand-off through device flags -------------------------------------------------------------------------------
// An event wait or an event record between two kernels of one stream costs 5-8 us on this stack (measured gap between
// consecutive filter kernels: 4 us bare, 9.4 with the record, 14.9 with both).  So the filter stream carries nothing
// but filter kernels; each one, when it starts, (a) announces that its predecessor has finished -- the kernel boundary
// made that kernel's stores visible -- which releases the bulk stream's apply, and (b) checks that its own K is there
// (it practically always is: the cross-Gram runs one block ahead).  Every wait is bounded.
constexpr long long HANDOFF_MAX_TICKS = 20LL * 100000000LL;   // 20 s of the 100 MHz real-time counter, then the abort flag
                                                               // (a first RCCL collective may take seconds to connect)

// Relaxed agent-scope accesses: every flag is written by a kernel that starts AFTER the kernel whose data it announces has
// ended, and (in the normal case) read before the reader touches that data for the first time in a kernel that started
// after it was set -- the kernel boundaries are the release and the acquire.  (Acquire loads / release stores here cost an
// L1 invalidate / L2 write-back each: ~1 us per block.)  The one exception, a flag observed only after polling, is
// followed by an explicit acquire fence in blk_handoff_begin.
__device__ __forceinline__ long long flag_load(const long long* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void flag_store(long long* f, long long v) { __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// returns false (uniformly) if the run was aborted; ends with a workgroup barrier
__device__ __forceinline__ bool blk_handoff_begin(const BlockParams& b) {
  __shared__ int s_ok;            // a slot of its own: nothing else writes it
  int* s_flag = &s_ok;
  if (!b.flags) return true;
  if (threadIdx.x == 0) {
    int ok = 1;
    flag_store(b.flags + 1, b.seq);                      // blocks < seq are complete
    const long long xg0 = flag_load(b.flags + 0), ab0 = flag_load(b.flags + 2);   // both loads in flight together
    if (ab0 != 0) ok = 0;
    if (ok && xg0 < b.seq) {
      long long polls = 0;
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      while (flag_load(b.flags + 0) < b.seq) {
        __builtin_amdgcn_s_sleep(16);
        ++polls;
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > HANDOFF_MAX_TICKS || flag_load(b.flags + 2) != 0) { ok = 0; break; }
      }
      if (polls > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // K was written after this kernel started
      if (!ok) { flag_store(b.flags + 2, 1); if (b.sp.st->err == 0) b.sp.st->err = -7; }
    }
    *s_flag = ok;
  }
  __syncthreads();
  return *s_flag != 0;
}

// chain: between two blocks of one launch.  The stores of the block that just ended are complete (coefficients for the
// apply kernel were stored with agent scope, see coef_store), so it is announced; then the block's own cross-Gram is
// awaited (it practically always is there).  Returns false (uniformly) if the run was aborted; ends with a barrier.
__device__ __forceinline__ bool blk_chain_next(const BlockParams& b, const long long seq) {
  __shared__ int s_ok;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    int ok = 1;
    flag_store(b.flags + 1, seq);                      // blocks < seq are complete
    const long long xg0 = flag_load(b.flags + 0), ab0 = flag_load(b.flags + 2);
    if (ab0 != 0) ok = 0;
    if (ok && xg0 < seq) {
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      while (flag_load(b.flags + 0) < seq) {
        __builtin_amdgcn_s_sleep(4);
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > HANDOFF_MAX_TICKS || flag_load(b.flags + 2) != 0) { ok = 0; break; }
      }
      if (!ok) { flag_store(b.flags + 2, 1); if (b.sp.st->err == 0) b.sp.st->err = -7; }
    }
    s_ok = ok;
  }
  __syncthreads();
  __builtin_amdgcn_s_dcache_inv();      // the scalar cache does not see this kernel's own vector stores (DevState fields)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return s_ok != 0;
}

// Coefficients the apply kernel (other XCDs, released by a device flag instead of a kernel boundary when blocks are
// chained) reads: agent-scope stores go through to where every XCD sees them.  The cross-Gram is read the same way.
__device__ __forceinline__ void coef_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double xg_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// K of a pipelined block from the previous block's quantities (see BlockParams):
//   staging: Aprev (RB x r) -> sA image, XG[0:RB, 0:nb] -> sKA image reused as a (RB x nb') strip per pass
// Outputs the full symmetric sK.  Called by all NTH threads of the workgroup; ends with a barrier.
template <int NTH>
__device__ __forceinline__ void assemble_K(const BlockParams& b, double* sK, double* sA, double* sKA, const int r, const int tid) {
  const int nb = b.nb;
  const DevState* st = b.sp.st;
  for (int idx = tid; idx < RB * RB; idx += NTH) sK[idx] = 0.0;
  for (int idx = tid; idx < RB * r; idx += NTH) { const int m = idx / r, c = idx - m * r; sA[m * RS + c] = b.Aprev[idx]; }
  __syncthreads();
  // G block and the series block
  for (int idx = tid; idx < r * r; idx += NTH) { const int i = idx / r, c = idx - i * r; sK[i * RB + c] = st->G[idx]; }
  for (int idx = tid; idx < nb * nb; idx += NTH) { const int q = idx / nb, q2 = idx - q * nb; sK[(r + q) * RB + r + q2] = b.XG[(size_t)(RB + q) * XGB + q2]; }
  // cross block K[i][r+q] = sum_m Aprev[m][i] XG[m][q].  The top RB rows of the cross-Gram go through LDS, 32
  // columns at a time (sKA is free until the caller fills it): one coalesced round trip instead of RB
  // dependent L2 reads per output.
  for (int q0 = 0; q0 < nb; q0 += 32) {
    for (int idx = tid; idx < RB * 32; idx += NTH) {
      const int m = idx >> 5, q = idx & 31;
      if (q0 + q < nb) sKA[m * RS + q] = b.XG[(size_t)m * XGB + q0 + q];
    }
    __syncthreads();
    const int nq = nb - q0 < 32 ? nb - q0 : 32;
    for (int idx = tid; idx < r * nq; idx += NTH) {
      const int q = idx / r, i = idx - q * r;          // consecutive threads -> consecutive i (conflict-free sA reads, sKA broadcast)
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 8
      for (int m = 0; m < RB; m += 2) {
        acc0 += sA[m * RS + i] * sKA[m * RS + q];
        acc1 += sA[(m + 1) * RS + i] * sKA[(m + 1) * RS + q];
      }
      const double acc = acc0 + acc1;
      sK[i * RB + r + q0 + q] = acc;
      sK[(r + q0 + q) * RB + i] = acc;
    }
    __syncthreads();
  }
}

}  // namespace psmf
