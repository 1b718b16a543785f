// Blocked engine, host side and kernels (all but the filter3 family, psmf_filter34.hip): which kernel advances a block, the launches,
// the pipelined driver of a run, the engine's share of psmf_create and of psmf_time_kernel.
#include "psmf_host.h"
#include "psmf_block.hip"
#include "psmf_blk16.hip"
#include "psmf_blk32.hip"
#include "psmf_bulk.hip"

#include <cstdio>
#include <cstring>

namespace {

// one block of nb steps of the blocked engine: Gram, reduction, (all-reduce), coefficient-space filter, apply
void fill_block_params(psmf_filter* h, psmf::BlockParams& b, int64_t k0, int nb, int slot = 0) {
  memset(&b, 0, sizeof(b));
  b.last = 1;            // standalone block; the pipelined loop clears it for all but a run's last block
  b.sp = h->sp;
  b.Kpart = h->Kpart; b.K = h->Kmat;
  b.Acoef = h->Acoef + (size_t)slot * psmf::RB * psmf::RM;
  b.Bcoef = h->Bcoef + (size_t)slot * psmf::RB * psmf::RB;
  b.XGpart = h->XGpart;
  b.k0 = k0; b.nb = nb;
  b.gram_rows = (h->cfg.d_local + psmf::BLK_GRAM_WG - 1) / psmf::BLK_GRAM_WG;
}

void launch_blk_gram(psmf_filter* h, const psmf::BlockParams& b, hipStream_t stream = nullptr) {
  if (!stream) stream = h->stream;
  by_storage(h, [&](auto t) { hipLaunchKernelGGL(psmf::psmf_blk_gram_mfma<decltype(t)>, dim3(psmf::BLK_GRAM_WG), dim3(psmf::WG), 0, stream, b); });
  hipLaunchKernelGGL(psmf::psmf_blk_reduce, dim3(psmf::RB * psmf::RB / 128), dim3(128), 0, stream, b, (int)psmf::BLK_GRAM_WG);
}

// streaming bulk kernels (psmf_bulk.hip): float32 storage, d_local a multiple of 4, 16 <= r <= 32
bool blk_bulk2_ok(const psmf_filter* h) {
  return h->sw.bulk2 && h->cfg.storage == PSMF_F32 && (h->cfg.d_local % 4) == 0 && h->cfg.r <= 32 && (h->geo.rp % 4) == 0;
}

void launch_blk_xgram(psmf_filter* h, const psmf::BlockParams& x, double* xg, hipStream_t stream) {
  const size_t xg_elems = (size_t)(psmf::RB + psmf::XGB) * psmf::XGB;
  if (blk_bulk2_ok(h)) {
    const int nct = (h->block_steps + 15) / 16;
    const size_t lds = psmf::blk_xgram2_lds_bytes();
    if (nct <= 2) {
      hipLaunchKernelGGL(psmf::psmf_blk_xgram2<2>, dim3(h->bulk_wgs), dim3(psmf::BK_NT), lds, stream, x);
      hipLaunchKernelGGL(psmf::psmf_blk_xreduce2<2>, dim3(6 * 2 * 256 / 32), dim3(256), 0, stream, (const double*)x.XGpart, xg, h->bulk_wgs);
    } else {
      hipLaunchKernelGGL(psmf::psmf_blk_xgram2<3>, dim3(h->bulk_wgs), dim3(psmf::BK_NT), lds, stream, x);
      hipLaunchKernelGGL(psmf::psmf_blk_xreduce2<3>, dim3(7 * 3 * 256 / 32), dim3(256), 0, stream, (const double*)x.XGpart, xg, h->bulk_wgs);
    }
    return;
  }
  by_storage(h, [&](auto t) { hipLaunchKernelGGL(psmf::psmf_blk_xgram_mfma<decltype(t)>, dim3(psmf::BLK_GRAM_WG), dim3(psmf::WG), 0, stream, x); });
  hipLaunchKernelGGL(psmf::psmf_blk_xreduce, dim3((int)(xg_elems / 128)), dim3(128), 0, stream, x, xg, (int)psmf::BLK_GRAM_WG);
}

bool blk_small_dual(const psmf_filter* h);
bool blk_use_filter3(const psmf_filter* h) { return h->sw.filter3 && !blk_small_dual(h); }

bool blk_dual_ok(const psmf_filter* h) {
  // The two-inversion kernels (filter3, filter3s, filter2) read rho and q ONCE per block: per-step R_k / Q_k schedules
  // (psmf_set_schedules; the reference reads R[k], Q[k] every step, psmf.py:115,123,141) go to the general kernel.
  return h->sw.block_dual && h->q_iso && h->cfg.coef_update && h->cfg.pbar_predict && h->cfg.eta_full &&
         h->cfg.dyn_kind == PSMF_DYN_RANDOM_WALK && !h->sp.rho_sched && !h->sp.q_sched;
}

// filter4 (psmf_blk4.hip): the role-specialised kernel for diagonal-Jacobian dynamics -- cos-phase, unscaled sinusoid, and the
// random walk when R_k / Q_k schedules keep it off filter3 -- full filter, Q = q I, r <= 32; the recursive classes included
// filter6 (psmf_blk16.hip): the general block filter for r <= 16, role-specialised -- whatever filter3s / filter5 do not take,
// INCLUDING what filter4s would (measured at r = 10, d = 2e4: cos-phase full filter 117 k timesteps/s on filter4s, 316 k on
// filter6; its recursive form 196 k against 214 k)
bool blk_small_ok(const psmf_filter* h) { return h->sw.filter6 && h->cfg.r <= psmf::F6_RMAX; }

// ... and the default model too (random walk, Q = q I; PSMF_FILTER6_DUAL=0: filter3s), psmf_blk_filter6d
bool blk_small_dual(const psmf_filter* h) { return h->sw.filter6_dual && blk_small_ok(h) && blk_dual_ok(h); }

bool blk_seq_ok(const psmf_filter* h) {
  if (blk_small_ok(h)) return false;
  const int kd = h->cfg.dyn_kind;
  const bool diag_dyn = kd == PSMF_DYN_RANDOM_WALK || kd == PSMF_DYN_COS_PHASE || (kd == PSMF_DYN_SINUSOID && !(h->cfg.dyn_flags & 1));
  return h->sw.filter4 && h->sw.filter3 && h->sw.block_dual && h->q_iso && h->cfg.coef_update && h->cfg.pbar_predict && h->cfg.eta_full && diag_dyn &&
         h->cfg.r <= 32 && h->cfg.recursive != 2;      // (in-loop SGD: the kernels with dyn_adam_step carry it, filter4 / filter5 have an Adam step of their own)
}

// filter5: the simplified hook configuration (no coefficient update, eta = tr(R) / d, P_bar = P) with diagonal-Jacobian dynamics
bool blk_simpl_ok(const psmf_filter* h) {
  const int kd = h->cfg.dyn_kind;
  const bool diag_dyn = kd == PSMF_DYN_RANDOM_WALK || kd == PSMF_DYN_COS_PHASE || (kd == PSMF_DYN_SINUSOID && !(h->cfg.dyn_flags & 1));
  return h->sw.filter4 && h->sw.filter3 && !h->cfg.coef_update && !h->cfg.eta_full && !h->cfg.pbar_predict && diag_dyn && h->cfg.r <= 32 &&
         !h->sp.q_sched && h->cfg.recursive != 2;
}

}  // namespace

FilterKernel select_filter_kernel(const psmf_filter* h) {
  if (h->engine != 2) return pstep_usable(h) ? FK_PSTEP : FK_STEP;
  if (blk_simpl_ok(h)) return FK_FILTER5;
  const bool dual3 = blk_dual_ok(h) && blk_use_filter3(h);
  if (!dual3 && blk_seq_ok(h)) return h->cfg.r > 16 ? FK_FILTER4 : FK_FILTER4S;
  if (blk_small_dual(h)) return FK_FILTER6D;      // random walk, Q = q I at r <= 16: filter6 with the two inversions side by side
  if (dual3) return h->cfg.r > 16 ? FK_FILTER3 : FK_FILTER3S;
  if (blk_dual_ok(h)) return FK_FILTER2;
  if (blk_small_ok(h)) return FK_FILTER6;
  // 17 <= r <= 32, whatever is left (dense Jacobians, a general Q, ...): filter6's design on 2 x 2 tiles (psmf_blk32.hip)
  return (h->sw.filter7 && h->cfg.r > psmf::F6_RMAX && h->cfg.r <= 32) ? FK_FILTER7 : FK_GENERAL;
}

namespace {

void launch_blk_filter(psmf_filter* h, const psmf::BlockParams& b, hipStream_t stream = nullptr) {
  if (!stream) stream = h->stream;
  const size_t lds = psmf::blk_filter_lds_bytes();
  const FilterKernel fk = select_filter_kernel(h);
  switch (fk) {
    case FK_FILTER5: launch_blk_filter34(fk, b, stream); return;
    case FK_FILTER4:
    case FK_FILTER4S: {
      // filter4's fallback is the wave-local sweep (~5 us, five to six iterations' worth; filter3's LDS sweep: 15 us): a start
      // beyond ||R||_F = 0.6 is cheaper swept than iterated (PSMF_NS_FAR4)
      psmf::BlockParams b4 = b;
      if (!h->sw.ns_far_set) b4.sp.ns_far2 = h->sw.ns_far4 * h->sw.ns_far4;
      launch_blk_filter34(fk, b4, stream);
      return;
    }
    case FK_FILTER6D: {
      psmf::BlockParams b2 = b;
      b2.dual6 = 1;
      hipLaunchKernelGGL(psmf::psmf_blk_filter6d, dim3(1), dim3(psmf::WG), lds, stream, b2);
      return;
    }
    case FK_FILTER3:
    case FK_FILTER3S: launch_blk_filter34(fk, b, stream); return;
    case FK_FILTER2: {
      const size_t lds2 = psmf::blk_filter2_lds_bytes();
      switch (h->geo.rpad) {
        case 8: hipLaunchKernelGGL(psmf::psmf_blk_filter2<8>, dim3(1), dim3(2 * psmf::WG), lds2, stream, b); break;
        case 16: hipLaunchKernelGGL(psmf::psmf_blk_filter2<16>, dim3(1), dim3(2 * psmf::WG), lds2, stream, b); break;
        default: hipLaunchKernelGGL(psmf::psmf_blk_filter2<32>, dim3(1), dim3(2 * psmf::WG), lds2, stream, b); break;
      }
      return;
    }
    case FK_FILTER6: hipLaunchKernelGGL(psmf::psmf_blk_filter6, dim3(1), dim3(psmf::WG), lds, stream, b); return;
    case FK_FILTER7: hipLaunchKernelGGL(psmf::psmf_blk_filter7, dim3(1), dim3(psmf::WG), lds, stream, b); return;
    case FK_GENERAL:
    case FK_STEP:
    case FK_PSTEP:
      break;
  }
  switch (h->geo.rpad) {
    case 8: hipLaunchKernelGGL(psmf::psmf_blk_filter<8>, dim3(1), dim3(psmf::WG), lds, stream, b); break;
    case 16: hipLaunchKernelGGL(psmf::psmf_blk_filter<16>, dim3(1), dim3(psmf::WG), lds, stream, b); break;
    default: hipLaunchKernelGGL(psmf::psmf_blk_filter<32>, dim3(1), dim3(psmf::WG), lds, stream, b); break;
  }
}

void launch_blk_apply(psmf_filter* h, const psmf::BlockParams& b, hipStream_t stream = nullptr) {
  if (!stream) stream = h->stream;
  if (blk_bulk2_ok(h)) {
    const int nyc = (h->block_steps + 15) / 16;
    const size_t lds = psmf::blk_apply2_lds_bytes();
    if (nyc <= 2) hipLaunchKernelGGL(psmf::psmf_blk_apply2<2>, dim3(h->bulk_wgs), dim3(psmf::BK_NT), lds, stream, b);
    else hipLaunchKernelGGL(psmf::psmf_blk_apply2<3>, dim3(h->bulk_wgs), dim3(psmf::BK_NT), lds, stream, b);
    return;
  }
  const int nslab = (h->cfg.d_local + 15) / 16;
  int g = (nslab + 3) / 4;
  if (g > 1024) g = 1024;
  const size_t lds = psmf::blk_apply_lds_bytes();
  by_storage(h, [&](auto t) { hipLaunchKernelGGL(psmf::psmf_blk_apply_mfma<decltype(t)>, dim3(g), dim3(psmf::WG), lds, stream, b); });
}

int enqueue_block(psmf_filter* h, int64_t k0, int nb) {
  psmf::BlockParams b;
  fill_block_params(h, b, k0, nb);
  launch_blk_gram(h, b);
  if (h->use_coll) { const int rc = all_reduce_sum(h, h->Kmat, psmf::RB * psmf::RB, h->stream); if (rc) return rc; }
  launch_blk_filter(h, b);
  launch_blk_apply(h, b);
  return PSMF_OK;
}


// Pipelined blocks: the filter kernels chain back to back on the main stream; Gram of the first block,
// cross-Grams (one block ahead) and applies run on the bulk stream, synchronised with events:
//   bulk:  gram(0) | xgram(1) | [filter(0)] apply(0) | xgram(2) | [filter(1)] apply(1) | ...
//   main:  [gram(0)] filter(0) | [xgram(1)] filter(1) | [xgram(2)] filter(2) | ...
// xgram(b+1) reads C before apply(b) rewrites it (stream order on bulk); the ping-pong coefficient
// buffers of block b are rewritten by filter(b+2), which waits for xgram(b+2), enqueued after apply(b).
int enqueue_blocks_pipelined(psmf_filter* h, int64_t k_begin, int64_t k_end) {
  const int B = h->block_steps;
  const double t_enq0 = h->sw.host_timing ? host_now_ms() : 0.0;
  double t_prev = t_enq0, t_worst = 0.0;
  long long worst_blk = -1;
  const int64_t nblk = (k_end - k_begin + B - 1) / B;
  auto k0_of = [&](int64_t b) { return k_begin + b * B; };
  auto nb_of = [&](int64_t b) { const int64_t left = k_end - k0_of(b); return (int)(left < B ? left : B); };
  const size_t xg_elems = (size_t)(psmf::RB + psmf::XGB) * psmf::XGB;
  HIP_TRY(h, hipEventRecord(h->evS, h->stream));            // everything enqueued so far (state uploads) is visible to bulk
  HIP_TRY(h, hipStreamWaitEvent(h->bulk, h->evS, 0));
  hipStream_t fs = h->fstream ? h->fstream : h->stream;    // the filter chain (its own CUs when the mask streams exist)
  if (h->fstream) HIP_TRY(h, hipStreamWaitEvent(fs, h->evS, 0));
  psmf::BlockParams b;
  // hand-off by device flags when the filter chain has a stream (hardware queue) of its own; by events otherwise
  const bool flags_off = !h->sw.block_flags;
  // (a tool that serialises dispatches: events.  A host-mediated communicator synchronises the bulk stream at every exchange
  //  anyway, and several such handles usually share one process and one GPU -- shards of a test -- where kernels that spin on
  //  flags could end up behind each other in a shared hardware queue: events there, too -- unless PSMF_HOST_COMM_FLAGS=1 asks for the
  //  flags, which is how tests/test_hip_multishard.py runs the flag hand-off and the chained launch with more than one shard)
  const bool use_flags = h->fstream != nullptr && h->flags != nullptr && !flags_off && h->streams_concurrent && (!h->host_fn || h->sw.host_comm_flags);
  const long long s0 = h->seq_next;
  h->seq_next += nblk;
  // chain: the filter kernels of the whole run as ONE launch (psmf_blk_filter3; the bulk stream is driven as before)
  const bool chain_off = !h->sw.block_chain;
  const bool chain = use_flags && !chain_off && nblk > 1 && ((blk_dual_ok(h) && blk_use_filter3(h)) || blk_seq_ok(h) || blk_simpl_ok(h));
  // first block: plain Gram of the stored C
  fill_block_params(h, b, k0_of(0), nb_of(0), 0);
  launch_blk_gram(h, b, h->bulk);
  if (h->use_coll) { const int rc = all_reduce_sum(h, h->Kmat, psmf::RB * psmf::RB, h->bulk); if (rc) return rc; }
  if (use_flags) hipLaunchKernelGGL(psmf::psmf_flag_set_k, dim3(1), dim3(1), 0, h->bulk, h->flags + 0, s0);
  else HIP_TRY(h, hipEventRecord(h->evX[0], h->bulk));
  if (chain) {
    psmf::BlockParams c;
    fill_block_params(h, c, k0_of(0), nb_of(0), 0);
    c.flags = h->flags;
    c.seq = s0;
    c.last = 1;
    c.chain = (int)nblk;
    c.chain_B = B;
    c.chain_kend = k_end;
    c.carry = h->sw.chain_carry ? 1 : 0;
    c.xg_ahead = h->sw.xg_ahead ? 1 : 0;
    c.Acoef0 = h->Acoef;
    c.Bcoef0 = h->Bcoef;
    c.XG0 = h->XG;
    const int slot_ev = h->evk_pending < psmf_filter::kTimedRuns ? h->evk_pending : -1;
    if (slot_ev >= 0) HIP_TRY(h, hipEventRecord(h->evK0[slot_ev], fs));
    launch_blk_filter(h, c, fs);
    if (slot_ev >= 0) { HIP_TRY(h, hipEventRecord(h->evK1[slot_ev], fs)); ++h->evk_pending; }
    HIP_TRY(h, hipEventRecord(h->evC, fs));
  }
  for (int64_t bi = 0; bi < nblk; ++bi) {
    const int slot = (int)(bi & 1);
    // bulk: cross-Gram for block bi + 1 (needs C as of the start of block bi)
    if (bi + 1 < nblk) {
      psmf::BlockParams x;
      fill_block_params(h, x, k0_of(bi), nb_of(bi), slot);
      x.k1 = k0_of(bi + 1);
      x.nb1 = nb_of(bi + 1);
      double* xg = h->XG + (size_t)((bi + 1) & 1) * xg_elems;
      launch_blk_xgram(h, x, xg, h->bulk);
      if (h->use_coll) { const int rc = all_reduce_sum(h, xg, xg_elems, h->bulk); if (rc) return rc; }
      if (use_flags) hipLaunchKernelGGL(psmf::psmf_flag_set_k, dim3(1), dim3(1), 0, h->bulk, h->flags + 0, s0 + bi + 1);
      else HIP_TRY(h, hipEventRecord(h->evX[(bi + 1) & 3], h->bulk));
    }
    // filter stream: filter of block bi
    fill_block_params(h, b, k0_of(bi), nb_of(bi), slot);
    if (bi > 0) {
      b.assemble = 1;
      b.XG = h->XG + (size_t)(bi & 1) * xg_elems;
      b.Aprev = h->Acoef + (size_t)(slot ^ 1) * psmf::RB * psmf::RM;
    }
    b.last = (bi + 1 == nblk) ? 1 : 0;
    if (use_flags) {
      b.flags = h->flags;
      b.seq = s0 + bi;
      if (!chain) {
        launch_blk_filter(h, b, fs);
        if (bi + 1 == nblk) hipLaunchKernelGGL(psmf::psmf_flag_set_k, dim3(1), dim3(1), 0, fs, h->flags + 1, s0 + nblk);   // the last block has no successor to announce it
      }
      hipLaunchKernelGGL(psmf::psmf_flag_wait_k, dim3(1), dim3(64), 0, h->bulk, h->flags, s0 + bi + 1, h->st);
    } else {
      HIP_TRY(h, hipStreamWaitEvent(fs, h->evX[bi & 3], 0));
      launch_blk_filter(h, b, fs);
      HIP_TRY(h, hipEventRecord(h->evF[bi & 3], fs));
      HIP_TRY(h, hipStreamWaitEvent(h->bulk, h->evF[bi & 3], 0));
    }
    // bulk: apply of block bi
    launch_blk_apply(h, b, h->bulk);
    HIP_TRY(h, hipEventRecord(h->evA[bi & 3], h->bulk));
    if (h->sw.host_timing) { const double t = host_now_ms(); if (t - t_prev > t_worst) { t_worst = t - t_prev; worst_blk = bi; } t_prev = t; }
  }
  if (h->sw.host_timing) {
    const double t = host_now_ms();
    if (t - t_enq0 > 20.0 || t_worst > 5.0)
      fprintf(stderr, "[psmf host timing] enqueue of %lld blocks took %.1f ms, slowest block's calls %.1f ms (block %lld)\n", (long long)nblk, t - t_enq0, t_worst, worst_blk);
  }
  HIP_TRY(h, hipStreamWaitEvent(h->stream, h->evA[(nblk - 1) & 3], 0));   // the main stream sees the final C / y_hat
  // ... and the r x r state: the chained kernel writes DevState in its tail, after it has released the last apply, so the end of
  // that launch (not the apply alone) is what host reads / the next run's preparation on the main stream have to follow
  if (chain) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->evC, 0));
  HIP_TRY(h, hipGetLastError());
  return PSMF_OK;
}

}  // namespace

// the steps k_begin + 1 .. k_end of a prepared run (run_steps, psmf_capi.hip) on the blocked engine
int run_blocks(psmf_filter* h, int64_t k_begin, int64_t k_end) {
  int rc = PSMF_OK;
  const bool pipe_off = !h->sw.block_pipe;
  if (!pipe_off && k_end - k_begin > h->block_steps) {
    rc = enqueue_blocks_pipelined(h, k_begin, k_end);
    if (rc) return rc;
    h->k_done = k_end;
    return PSMF_OK;
  }
  int64_t k = k_begin;
  while (k < k_end) {
    const int nb = (int)((k_end - k) < h->block_steps ? (k_end - k) : h->block_steps);
    rc = enqueue_block(h, k, nb);
    if (rc) return rc;
    k += nb;
  }
  HIP_TRY(h, hipGetLastError());
  h->k_done = k_end;
  return PSMF_OK;
}

// start of a run (prepare): the abort flag of the device-flag hand-off
void clear_block_abort_flag(psmf_filter* h) { hipLaunchKernelGGL(psmf::psmf_flag_set_k, dim3(1), dim3(1), 0, h->stream, h->flags + 2, 0LL); }

// blocked engine: buffers, CU-masked streams, events, the concurrency probe, the LDS opt-in of its kernels
int init_blocked(psmf_filter* h) {
  const psmf_config* cfg = &h->cfg;
  // B = 64 - r timesteps per block, at most 48: the role-specialised filter kernel and the streaming bulk kernels stage
  // up to three 16-column tiles of a series block (r < 16 would otherwise give blocks of 49..63)
  h->block_steps = psmf::RB - cfg->r < 48 ? psmf::RB - cfg->r : 48;
  ALLOC_TRY(h, h->Kpart.alloc((size_t)psmf::BLK_GRAM_WG * psmf::RB * psmf::RB * sizeof(double)));
  ALLOC_TRY(h, h->Kmat.alloc((size_t)psmf::RB * psmf::RB * sizeof(double)));
  ALLOC_TRY(h, h->Acoef.alloc((size_t)2 * psmf::RB * psmf::RM * sizeof(double)));
  ALLOC_TRY(h, h->Bcoef.alloc((size_t)2 * psmf::RB * psmf::RB * sizeof(double)));
  HIP_TRY(h, hipMemset(h->Bcoef, 0, (size_t)2 * psmf::RB * psmf::RB * sizeof(double)));
  ALLOC_TRY(h, h->XGpart.alloc((size_t)psmf::BLK_GRAM_WG * (psmf::RB + psmf::XGB) * psmf::XGB * sizeof(double)));
  ALLOC_TRY(h, h->XG.alloc((size_t)2 * (psmf::RB + psmf::XGB) * psmf::XGB * sizeof(double)));
  HIP_TRY(h, hipMemset(h->XG, 0, (size_t)2 * (psmf::RB + psmf::XGB) * psmf::XGB * sizeof(double)));   // the all-reduce covers entries no kernel writes
  ALLOC_TRY(h, h->flags.alloc(8 * sizeof(long long)));
  HIP_TRY(h, hipMemset(h->flags, 0, 8 * sizeof(long long)));
  // The filter chain is one workgroup on the critical path; the bulk kernels (cross-Gram, apply) run
  // beside it and would be co-scheduled onto its CU, stretching it by 10-17 % (measured).  Partition the
  // chip with CU masks: the filter's stream owns `nres` CUs, the bulk stream the others.
  const int nres = h->sw.reserved_cus;
  hipDeviceProp_t prop;
  HIP_TRY(h, hipGetDeviceProperties(&prop, cfg->device));
  const int ncu = prop.multiProcessorCount;
  const int words = (ncu + 31) / 32;
  // The split below is written for the unpartitioned MI355X: 256 CUs = 8 XCDs x 4 shader engines x 8 CUs, mask bit =
  // 32 cu + 8 se + xcc (tools/xcc_probe.hip).  On any other device (a CPX / NPS partition, another part) the bit layout and the
  // engine count are not known here: no CU masks, plain streams -- the filter chain then shares CUs with the bulk kernels
  // (10-17 % slower, measured), which is a speed matter only.
  const bool known_layout = ncu == 256;
  if (known_layout && nres > 0 && nres < ncu / 2 && words <= 16) {
    uint32_t mf[16] = {0}, mb[16] = {0};
    for (int i = 0; i < ncu; ++i) (i < nres ? mf : mb)[i >> 5] |= 1u << (i & 31);
    Stream fs, bs;
    if (hipExtStreamCreateWithCUMask(fs.put(), words, mf) == hipSuccess && hipExtStreamCreateWithCUMask(bs.put(), words, mb) == hipSuccess) {
      h->fstream = std::move(fs);
      h->bulk = std::move(bs);
      h->reserved_cus = nres;
      // The streaming kernels hold one 512-thread workgroup per CU (86-131 KB of LDS), and the dispatcher deals workgroups
      // to the 32 shader engines (8 XCDs x 4) in equal shares whatever the mask has left each of them.  The filter's
      // 8 CUs are CU 0 of engine 0 of every XCD (mask bit = 32 cu + 8 se + xcc, tools/xcc_probe.hip): those engines
      // keep 7 CUs, so with more than 7 workgroups per engine one CU gets a second one and the kernel takes two
      // rounds -- 231 / 317 us per block at d = 1e6 with 248 or 256 workgroups against 138 / 193 us with 224
      // (tools/bulk_stream.hip; 124 / 172 us on the unmasked chip).  Hence (CUs per engine - 1) x 32.
      const int n_engines = 32, per_engine = ncu / n_engines - (nres + n_engines - 1) / n_engines;
      h->bulk_wgs = per_engine >= 1 ? per_engine * n_engines : 8;
      if (h->bulk_wgs > 256) h->bulk_wgs = 256;
      { const int v = h->sw.bulk_wgs_env; if (v >= 8 && v <= 256) h->bulk_wgs = (v / 8) * 8; }
    } else {
      (void)hipGetLastError();      // (plain streams below; fs, bs release what was created)
    }
  }
  if (!h->bulk) HIP_TRY(h, hipStreamCreateWithFlags(h->bulk.put(), hipStreamNonBlocking));
  for (int i = 0; i < 4; ++i) {
    HIP_TRY(h, hipEventCreateWithFlags(h->evF[i].put(), hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(h->evA[i].put(), hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(h->evX[i].put(), hipEventDisableTiming));
  }
  HIP_TRY(h, hipEventCreateWithFlags(h->evS.put(), hipEventDisableTiming));
  HIP_TRY(h, hipEventCreateWithFlags(h->evC.put(), hipEventDisableTiming));
  for (int i = 0; i < psmf_filter::kTimedRuns; ++i) { HIP_TRY(h, hipEventCreate(h->evK0[i].put())); HIP_TRY(h, hipEventCreate(h->evK1[i].put())); }
  if (h->fstream && h->flags) {
    // the device-flag hand-off and the chained filter launches need the two streams to run concurrently: probe it (a waiter on the filter stream, then the
    // setter on the bulk stream; the waiter gives up after 50 ms)
    Dev<int> dres;
    ALLOC_TRY(h, dres.alloc(sizeof(int)));
    HIP_TRY(h, hipMemset(dres, 0, sizeof(int)));
    HIP_TRY(h, hipDeviceSynchronize());      // hipMemset is asynchronous on the null stream, the probe's streams are non-blocking: the zeroes (of dres and of h->flags above) first
    hipLaunchKernelGGL(psmf::psmf_probe_wait_k, dim3(1), dim3(1), 0, h->fstream, h->flags + 7, 1LL, 5000000LL, dres);
    hipLaunchKernelGGL(psmf::psmf_flag_set_k, dim3(1), dim3(1), 0, h->bulk, h->flags + 7, 1LL);
    HIP_TRY(h, hipStreamSynchronize(h->fstream));
    HIP_TRY(h, hipStreamSynchronize(h->bulk));
    int res = 0;
    HIP_TRY(h, hipMemcpy(&res, dres, sizeof(int), hipMemcpyDeviceToHost));
    h->streams_concurrent = res == 1;
  }
  // function-local: no namespace-scope initialiser takes kernel addresses before the runtime has registered them
  const size_t flds = psmf::blk_filter_lds_bytes(), flds2 = psmf::blk_filter2_lds_bytes();
  const size_t alds = psmf::blk_apply_lds_bytes(), alds2 = psmf::blk_apply2_lds_bytes(), xlds2 = psmf::blk_xgram2_lds_bytes();
  const struct { const void* fn; size_t bytes; } lds_kernels[] = {
    {(const void*)psmf::psmf_blk_filter6, flds}, {(const void*)psmf::psmf_blk_filter6d, flds}, {(const void*)psmf::psmf_blk_filter7, flds},
    {(const void*)psmf::psmf_blk_filter<8>, flds}, {(const void*)psmf::psmf_blk_filter<16>, flds}, {(const void*)psmf::psmf_blk_filter<32>, flds},
    {(const void*)psmf::psmf_blk_apply_mfma<float>, alds}, {(const void*)psmf::psmf_blk_apply_mfma<double>, alds},
    {(const void*)psmf::psmf_blk_xgram2<2>, xlds2}, {(const void*)psmf::psmf_blk_xgram2<3>, xlds2},
    {(const void*)psmf::psmf_blk_apply2<2>, alds2}, {(const void*)psmf::psmf_blk_apply2<3>, alds2},
    {(const void*)psmf::psmf_blk_filter2<8>, flds2}, {(const void*)psmf::psmf_blk_filter2<16>, flds2}, {(const void*)psmf::psmf_blk_filter2<32>, flds2},
  };
  for (const auto& k : lds_kernels) { const int rc = opt_in_lds(h, k.fn, k.bytes); if (rc) return rc; }
  return opt_in_lds_filter34(h);      // filter3 / 3s / 4 / 4s / 5: in the unit that defines them
}

// psmf_time_kernel on a blocked handle; saved_st: the DevState as it was before the measurement
int time_block_kernels(psmf_filter* h, int which, int iters, int nb, const DevState* saved_st, float* avg_us) {
  psmf::BlockParams b;
  fill_block_params(h, b, h->sp.series_t0, nb);
  launch_blk_gram(h, b);           // a valid K for the filter / apply measurements
  launch_blk_filter(h, b);
  auto one = [&]() {
    if (which == 0) { HIP_TRY(h, hipMemcpyAsync(h->st, saved_st, sizeof(DevState), hipMemcpyDeviceToDevice, h->stream)); launch_blk_filter(h, b); }
    else if (which == 1) {
      // the per-block d-sized contraction: the cross-Gram for the next block (+ reduction) when the series holds
      // two blocks, else the plain block Gram
      if (h->T_cap >= 2 * (int64_t)nb) {
        psmf::BlockParams x = b;
        x.k1 = b.k0 + nb; x.nb1 = nb;
        launch_blk_xgram(h, x, h->XG, h->stream);
      } else {
        launch_blk_gram(h, b);
      }
    }
    else launch_blk_apply(h, b);
    return (int)PSMF_OK;
  };
  int rc;
  for (int i = 0; i < 2; ++i) { rc = one(); if (rc) return rc; }
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < iters; ++i) { rc = one(); if (rc) return rc; }
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *avg_us = ms * 1000.f / iters;
  return PSMF_OK;
}
