// The kernels of the filter3 family (filter3 / 3s / 4 / 4s / 5): one body over the programs of psmf_blk3.hip and psmf_blk4.hip,
// and its five __global__ instances.  Included by one translation unit (psmf_filter34.hip).
#pragma once
#include "psmf_blk3.hip"
#include "psmf_blk4.hip"      // filter4: the same skeleton for diagonal-Jacobian dynamics (sequential inversions)

namespace psmf {

// SMALL = true: the r <= 16 instantiation, a kernel of its own -- compiled into the same kernel as the two r > 16 programs it
// cost the r = 32 path 2 % (register allocation over the larger kernel: 111 spilled registers against 96; measured A / B on one box)
// KIND 0: filter3 (random walk, two parallel inversions); KIND 1: filter4, KIND 2: filter5 (simplified hooks) (psmf_blk4.hip)
template <bool SMALL, int KIND = 0>
__device__ __forceinline__ void blk_filter3_body(const BlockParams& b0) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sm = reinterpret_cast<double*>(smem_raw);
  const StepParams& p = b0.sp;
  DevState* st = p.st;
  const int r = p.r, tid0 = threadIdx.x;
  const int r2 = r + (r & 1);
  // ---- LDS carve ----
  // Everything a step touches sits in STATIC LDS: its addresses are compile-time constants that fold into the ds
  // instructions' immediate offsets.  (Off the dynamic-LDS base the compiler formed (lane part + constant) + base for
  // every row / column it reads and kept each sum in a VGPR of its own across the loop: 136 spilled registers.)
  __shared__ __attribute__((aligned(16))) double hot[2 * 4 * 8 * 64 + 3 * RM + 2 * RB + F3_NSC + 12 + 6 + 8 * 32];
  __shared__ __attribute__((aligned(16))) float hotP[2 * 4 * 2 * 64 * 4];
  __shared__ __attribute__((aligned(16))) float hotS[2 * 128];
  F3Lds L;
  L.sK = sm;
  L.sA = L.sK + RB * RB;
  L.sKA = L.sA + RB * F3_AS;
  L.img = L.sKA + RB * F3_AS;
  L.rowbufX = L.img + 2 * 32 * F3_S;
  L.rowbufY = L.rowbufX + 4 * RM;
  L.errflag = reinterpret_cast<int*>(L.rowbufY + 4 * RM);
  L.dump = hot;
  L.dumpP = hotP;
  L.mub = L.dump + 2 * 4 * 8 * 64;
  L.w = L.mub + RM;
  L.h = L.w + RM;
  L.a = L.h + RM;
  L.Ka = L.a + RB;
  L.sc = L.Ka + RB;
  L.nrm = L.sc + F3_NSC;
  L.hv = L.nrm + 12;
  L.gp = L.hv + 2;
  L.tr = L.gp + 2;
  L.sab = L.tr + 2;
  L.sal = L.sab + 128;
  L.sbe = L.sal + 64;
  L.s32 = hotS;
  __shared__ long long s_tick[2];
  L.tick = s_tick;
  __shared__ long long s_acc[F3A_N];
  __shared__ long long s_hand[2];
  L.acc = s_acc;
  L.hand = s_hand;
  __shared__ __attribute__((aligned(16))) double hot4[KIND >= 1 ? 5 * RM + 2 * 48 + F4_NKC : 2];
  F4Lds D;
  D.fd = hot4; D.mu = D.fd + RM; D.tp = D.mu + RM; D.th = D.tp + RM; D.rs = D.th + 2 * RM; D.qs = D.rs + 48; D.kc = D.qs + 48;
  if (tid0 == 0) { L.nrm[8] = p.ns_tol2; L.nrm[9] = p.ns_far2; L.nrm[10] = 0.25 * p.ns_tol2; }   // (read behind the barriers of the block set-up)

  // ---- one launch = `chain` consecutive blocks (1 when the blocks are launched one by one) ----
  // Chained, the blocks of a run pay the kernel launch, the cold instruction cache and the hand-off round trips once
  // instead of once per block; the state travels from block to block through LDS (chain carry) or the f3_* dump (this CU's L1 / L2).
  // Chain carry (KIND 0): between the blocks of one launch the state stays on chip (F3Carry); DevState gets it where the launch ends.
  const int nchain = b0.chain > 1 ? b0.chain : 1;
  const bool carry = KIND == 0 && b0.chain > 1 && b0.carry != 0;
  // WIDE: psmf_blk_filter3 itself.  What shortens the boundary between two carried blocks (F3Carry in 16-byte pieces, one barrier
  // behind the assembly, the diagnostics one lane per word, A_B staged and stored early) is compiled into this kernel alone.
  constexpr bool WIDE = KIND == 0 && !SMALL;
  const bool acc_lds = b0.chain > 1;      // the diagnostics of a chained launch are summed in LDS (f3_acc_flush)
  if (tid0 == 0) {
#pragma unroll
    for (int i = 0; i < F3A_N; ++i) s_acc[i] = 0;
    if (acc_lds) s_acc[F3A_TEND] = st->cnt[6];      // end of the filter kernel before this launch
    s_hand[1] = 0;
  }
  for (int j = 0; j < nchain; ++j) {
  // (the thread index is made opaque per block: otherwise everything the programs' prologues derive from it -- lane masks,
  //  LDS addresses, layouts -- is loop-invariant, gets hoisted out of this loop and stays live across it: 3.3 KB of spills)
  int tid = tid0;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int role = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the role branches are scalar branches
  const BlockParams& b = b0;
  F3Blk k;
  k.k0 = b0.k0; k.nb = b0.nb; k.last = b0.last; k.Acoef = b0.Acoef; k.Bcoef = b0.Bcoef; k.XG = b0.XG; k.Aprev = b0.Aprev;
  k.from_lds = (carry && j > 0) ? 1 : 0;
  k.to_lds = (carry && j < nchain - 1) ? 1 : 0;
  int assemble = b0.assemble;
  long long seq = b0.seq;
  if (b0.chain > 1) {
    const int slot = j & 1;
    k.k0 = b0.k0 + (long long)j * b0.chain_B;
    const long long left = b0.chain_kend - k.k0;
    k.nb = (int)(left < b0.chain_B ? left : b0.chain_B);
    k.Acoef = b0.Acoef0 + (size_t)slot * RB * RM;
    k.Bcoef = b0.Bcoef0 + (size_t)slot * RB * RB;
    seq = b0.seq + j;
    k.last = (j == nchain - 1) ? b0.last : 0;
    if (j > 0) {
      assemble = 1;
      k.XG = b0.XG0 + (size_t)slot * (RB + XGB) * XGB;
      k.Aprev = nullptr;                                               // left in sA by the block that just ended
    }
  }
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();      // 100 MHz: in-situ duration / gap diagnostics
  F3XG xg = {};     // (defined on every path: nothing of it crosses the chain loop)
  bool ahead = false;
  if (j > 0) {
    if (carry && b0.xg_ahead) ahead = f3_xg_ahead(k, L, xg, tid);
    if (!(carry ? f3_chain_next(b0, L, seq) : blk_chain_next(b0, seq))) {
      if (k.from_lds) f3_carry_flush<WIDE>(b0, L, k.k0, tid);                // the blocks completed, as they would have left DevState
      if (tid == 0) f3_acc_flush(st, L.acc);
      return;
    }
  } else {
    // Touch what the start-up will read -- the cross-Gram, the previous block's coefficients, the carried register dump --
    // while the hand-off flags are in flight: one memory round trip for the three instead of three in a row.  (A cross-Gram
    // that is not there yet is re-read after the poll's acquire fence.)
    double pf = 0.0;
    if (b.flags) {
      if (assemble) {
        pf = k.XG[(size_t)tid * 16];                                   // (RB + XGB) x XGB doubles = 512 lines of 128 bytes
        if (tid < RB * RM / 16) pf += k.Aprev[tid * 16];
      }
      constexpr int kDumpLines = (int)((sizeof(st->f3_G) + sizeof(st->f3_W) + sizeof(st->f3_Xc) + sizeof(st->f3_V) + sizeof(st->f3_Xa)) / 128);
      static_assert(kDumpLines <= F3_NT, "one line per thread");
      if (tid < kDumpLines) pf += st->f3_G[tid * 16];                  // the dump is contiguous from f3_G
    }
    if (!blk_handoff_begin(b)) return;
    if (pf == 1.2345e300) hot[0] = pf;                                 // (keeps the loads; never true)
  }
  const long long t_h = (long long)__builtin_amdgcn_s_memrealtime();
  // psmf_blk_filter3: a block that arrives through LDS (chain carry, j > 0) has ONE barrier between the hand-off and the prologues: the assembly
  // leaves its closing barrier to the one behind the LDS set-up below.  The set-up then runs beside the assembly, behind the
  // hand-off's barrier only, so every word it writes must have been read for the last time IN FRONT of that barrier:
  //   errflag           read by the sweeps (inside a step) and by wave 4 at the block end, in front of its drain;
  //   hand[0]           read by wave 6 in phase 2 of the last timestep;
  //   acc[F3A_BLK..]    read by wave 0 behind its block end, in front of the hand-off;
  //   w, h, sc          read inside the steps; sc[F3_PSCALE], sc[F3_IOM] once more by waves 0-4 between the barrier of the block
  //                     end and the hand-off;
  //   the K image       read inside the steps (wave 6) and nowhere behind them.
  // hand[1] is the exception: every wave reads it BEHIND the hand-off's barrier (f3_chain_next), so it is not reset here -- and
  // need not be.  It is 0 already unless the hand-off was the fast one; a block that hands on rewrites it in its last timestep
  // (wave 6's poll, ordered by BF and the barrier of the block end) before f3_xg_ahead / f3_chain_next read it again; behind the
  // last block of a launch nobody reads it, and the next launch starts from 0.
  const bool one_barrier = WIDE && k.from_lds != 0;
  if (!assemble) {
    for (int idx = tid; idx < RB * RB; idx += F3_NT) L.sK[idx] = b.K[idx];
  } else {
    f3_assemble_K<WIDE>(b, k, L, r, tid, xg, ahead, !one_barrier);
  }
  if (tid == 0) {
    *L.errflag = 0; L.hand[0] = seq + 1;
    if (!one_barrier) L.hand[1] = 0;
    L.acc[F3A_BLK] = 0; L.acc[F3A_BLK + 1] = 0; L.acc[F3A_BLK + 2] = 0; L.acc[F3A_BLK + 3] = 0;
  }
  // filter4, a block that follows another one in the same launch: h, w, ee, N, kappa and (a, b) of that block's last step stay
  // where they are in LDS -- the first step's start predictor uses them
  const bool warm = KIND == 1 && j > 0;      // (filter5 has no start to predict)
  if (tid < RM) {
    if (!k.from_lds) L.mub[tid] = (tid < r && KIND == 0) ? st->mu[tid] : 0.0;      // (chain carry: mu_bar is where the last step left it)
    if (!warm) { L.w[tid] = 0.0; L.h[tid] = 0.0; }
  }
  if (tid < F3_NSC && !warm) L.sc[tid] = 0.0;
  if (KIND >= 1) {
    // filter4 / filter5: mu_{k0}, theta and the block's share of the R_k / Q_k schedules into LDS (mu_bar, F of the first step: X pair's prologue)
    if (tid < RM) { D.mu[tid] = (tid < r) ? st->mu[tid] : 0.0; D.fd[tid] = 0.0; D.tp[tid] = 0.0; }
    if (tid >= 64 && tid < 64 + 2 * RM) {
      const int i = tid - 64, j = i & (RM - 1), hi = i >> 6;       // [0, RM): frequencies b (theta of cos-phase) | [RM, 2 RM): gains c
      const bool phased = p.dyn_kind == DYN_SINUSOID && (p.dyn_flags & 2);
      const bool have = p.n_theta > 0 && j < r && (hi == 0 || phased);
      const double tv = p.theta[have ? hi * r + j : 0];
      D.th[i] = have ? tv : 0.0;
    }
    if (tid >= 320 && tid < 320 + F4_NKC) f4_fill_trig_constants(D.kc, tid - 320);
    if (tid >= 256 && tid < 256 + 48) {
      const int jb_ = tid - 256;
      const long long ks = min((long long)(k.k0 + jb_ + 1), (long long)(k.k0 + k.nb)) - p.series_t0;
      if (p.rho_sched) D.rs[jb_] = p.rho_sched[ks];
      if (p.q_sched) D.qs[jb_] = p.q_sched[ks];
    }
  }
  // the previous block (or run) left the f3_* register dump behind -- or, chain carry, the state itself in LDS
  const bool carried = k.from_lds ? true : st->ns_valid == (KIND == 2 ? 5 : (KIND == 1 ? 4 : 3));
  f3_barrier();               // (what was loaded from global memory above sits in LDS writes, which wait for it themselves)
  const long long t_a = (long long)__builtin_amdgcn_s_memrealtime();
  if (!carried && KIND == 0) {
    // Lbar_1 = (P + q I)^-1 by the direct sweep: both halves run it in lockstep on their own image
    const int lt = tid & (WG - 1), c32 = lt & 31, rg = lt >> 5;
    double* im = tid < WG ? L.img : L.img + 32 * F3_S;
    const double q0 = st->Q[0];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int i = rg + 8 * m;
      const bool in = (i < r) && (c32 < r);
      const double pv = st->P[in ? i * r + c32 : 0];
      im[i * F3_S + c32] = in ? pv + (i == c32 ? q0 : 0.0) : (i == c32 ? 1.0 : 0.0);
    }
    __syncthreads();
    f3_sweep_images(L, r2, tid);          // image X now holds Lbar_1 (ends with a barrier)
  }
  if (KIND == 2) {
    // filter5 (psmf_blk4.hip): the simplified hooks -- the vector program alone; waves 0-3 keep the barrier count
    if (role < 4) f5_idle_program(k);
    else if (role == 4) f5_v_program<4>(b, k, L, D, lane, carried);
    else if (role == 5) f5_v_program<5>(b, k, L, D, lane, carried);
    else if (role == 6) f5_v_program<6>(b, k, L, D, lane, carried);
    else f5_v_program<7>(b, k, L, D, lane, carried);
  } else if (KIND == 1) {
    // filter4 (psmf_blk4.hip): waves 0-1 the X pair (P+), 2-3 the Y pair (Lbar), 4-7 the vector waves
    const int md = SMALL ? 2 : (r == 32 ? 0 : 1);
    if (role < 2) {
      if (md == 2) { if (role & 1) f4_x_program<1, 2>(b, k, L, D, role, lane, carried, warm && carried); else f4_x_program<0, 2>(b, k, L, D, role, lane, carried, warm && carried); }
      else if (md == 0) { if (role & 1) f4_x_program<1, 0>(b, k, L, D, role, lane, carried, warm && carried); else f4_x_program<0, 0>(b, k, L, D, role, lane, carried, warm && carried); }
      else { if (role & 1) f4_x_program<1, 1>(b, k, L, D, role, lane, carried, warm && carried); else f4_x_program<0, 1>(b, k, L, D, role, lane, carried, warm && carried); }
    } else if (role < 4) {
      if (md == 2) { if (role & 1) f4_y_program<1, 2>(b, k, L, D, role, lane, carried, warm && carried); else f4_y_program<0, 2>(b, k, L, D, role, lane, carried, warm && carried); }
      else if (md == 0) { if (role & 1) f4_y_program<1, 0>(b, k, L, D, role, lane, carried, warm && carried); else f4_y_program<0, 0>(b, k, L, D, role, lane, carried, warm && carried); }
      else { if (role & 1) f4_y_program<1, 1>(b, k, L, D, role, lane, carried, warm && carried); else f4_y_program<0, 1>(b, k, L, D, role, lane, carried, warm && carried); }
    } else {
      if (role == 4) f4_v_program<4>(b, k, L, D, lane, carried, warm && carried);
      else if (role == 5) f4_v_program<5>(b, k, L, D, lane, carried, warm && carried);
      else if (role == 6) f4_v_program<6>(b, k, L, D, lane, carried, warm && carried);
      else f4_v_program<7>(b, k, L, D, lane, carried, warm && carried);
    }
  } else if (role < 4) {
    const int inv = role >> 1;
    if (SMALL) {
      if (role & 1) f3_ns_program<1, 2>(b, k, L, inv, role, lane, carried);
      else f3_ns_program<0, 2>(b, k, L, inv, role, lane, carried);
    } else if (r == 32) {
      if (role & 1) f3_ns_program<1, 0>(b, k, L, inv, role, lane, carried);
      else f3_ns_program<0, 0>(b, k, L, inv, role, lane, carried);
    } else if (r > 16) {       // (always true here; the test keeps the code placement of the build this kernel was tuned at: +-1.5 %)
      if (role & 1) f3_ns_program<1, 1>(b, k, L, inv, role, lane, carried);
      else f3_ns_program<0, 1>(b, k, L, inv, role, lane, carried);
    }
  } else {
    if (role == 4) f3_v_program<4, WIDE>(b, k, L, lane, carried);
    else if (role == 5) f3_v_program<5, WIDE>(b, k, L, lane, carried);
    else if (role == 6) f3_v_program<6, WIDE>(b, k, L, lane, carried);
    else f3_v_program<7, WIDE>(b, k, L, lane, carried);
  }
  if (WIDE && acc_lds) {
    // psmf_blk_filter3, chained: the sums of F3Lds::acc, ONE LANE PER WORD.  (Thread 0 alone made fourteen dependent LDS read-modify-writes here,
    // between two blocks, with seven waves waiting at the hand-off's barrier.)  Wave 0 holds the block's stamps in scalar
    // registers; every lane reads the two ticks of the step loop, the end of the block before and its own word in one group,
    // forms what its word gains and writes it once.  64-bit integers throughout: the sums are what thread 0 formed.
    if (role == 0) {
      static_assert(F3A_CNT == 0 && F3A_DUR == 4 && F3A_GAP == 5 && F3A_TEND == 6 && F3A_BLOCKS == 7 && F3A_DBG == 8 && F3A_BLK == 13, "one lane per word of F3Lds::acc");
      const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
      long long* a = L.acc;
      const int wd = lane < F3A_BLK ? lane : 0;
      const long long tk0 = L.tick[0], tk1 = L.tick[1], tend0 = a[F3A_TEND], old = a[wd], blk = a[F3A_BLK + (lane & 3)];
      long long add = blk;                                                      // F3A_CNT + i: this block's counters
      if (wd == F3A_DUR) add = t_end - t_begin;
      if (wd == F3A_GAP) add = tend0 != 0 ? t_begin - tend0 : 0;                // (the first block of a handle's life has no gap)
      if (wd == F3A_TEND) add = t_end - old;                                    // (the word becomes t_end)
      if (wd == F3A_BLOCKS) add = 1;
      if (wd == F3A_DBG) add = t_h - t_begin;
      if (wd == F3A_DBG + 1) add = t_a - t_h;
      if (wd == F3A_DBG + 2) add = tk0 - t_a;
      if (wd == F3A_DBG + 3) add = tk1 - tk0;
      if (wd == F3A_DBG + 4) add = t_end - tk1;
      if (lane < F3A_BLK) a[wd] = old + add;
    }
  } else if (tid == 0) {
    // cnt[4]: sum of in-kernel durations, cnt[5]: sum of the gaps to the previous filter kernel, cnt[7]: launches (10 ns ticks)
    const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
    const long long dt[5] = {t_h - t_begin, t_a - t_h, L.tick[0] - t_a, L.tick[1] - L.tick[0], t_end - L.tick[1]};
    if (acc_lds) {            // (the other kernels of the family, chained: the same sums by thread 0, as they were)
      long long* a = L.acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) a[F3A_CNT + i] += a[F3A_BLK + i];
#pragma unroll
      for (int i = 0; i < 5; ++i) a[F3A_DBG + i] += dt[i];
      a[F3A_DUR] += t_end - t_begin;
      if (a[F3A_TEND] != 0) a[F3A_GAP] += t_begin - a[F3A_TEND];
      a[F3A_TEND] = t_end;
      a[F3A_BLOCKS] += 1;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) st->cnt[i] += L.acc[F3A_BLK + i];
#pragma unroll
      for (int i = 0; i < 5; ++i) st->dbg[i] += dt[i];
      st->cnt[4] += t_end - t_begin;
      if (st->cnt[6] != 0) st->cnt[5] += t_begin - st->cnt[6];
      st->cnt[6] = t_end;
      st->cnt[7] += 1;
      if (j == 0) st->dbg[5] += 1;            // kernel launches
    }
  }
  }   // chained blocks
  if (b0.chain > 1) {
    // the last block of the chain: complete, announced (the apply kernel of the bulk stream is waiting for it)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid0 == 0) {
      flag_store(b0.flags + 1, b0.seq + nchain);
      f3_acc_flush(st, s_acc);
    }
  }
}

__global__ __launch_bounds__(F3_NT) void psmf_blk_filter3(BlockParams b0) { blk_filter3_body<false>(b0); }     // 16 < r <= 32
__global__ __launch_bounds__(F3_NT) void psmf_blk_filter3s(BlockParams b0) { blk_filter3_body<true>(b0); }     // r <= 16
// diagonal-Jacobian dynamics / per-step schedules (psmf_blk4.hip)
__global__ __launch_bounds__(F3_NT) void psmf_blk_filter4(BlockParams b0) { blk_filter3_body<false, 1>(b0); }   // 16 < r <= 32
__global__ __launch_bounds__(F3_NT) void psmf_blk_filter4s(BlockParams b0) { blk_filter3_body<true, 1>(b0); }   // r <= 16
// simplified hooks (ExperimentSynthetic), diagonal-Jacobian dynamics, any r <= 32 (psmf_blk4.hip)
__global__ __launch_bounds__(F3_NT) void psmf_blk_filter5(BlockParams b0) { blk_filter3_body<false, 2>(b0); }

}  // namespace psmf
