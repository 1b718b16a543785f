// Role-specialised coefficient-space filter of the blocked engine ("filter3") for the common
// configuration (full filter, random-walk dynamics, Q = q I, r <= 32; blocks of at most 48 timesteps): same recursion as
// psmf_blk_filter2 (psmf_block.hip), re-laid out around what bounds a step on MI355X.
//
// On gfx950 v_mfma_f64_16x16x4_f64 runs at the float64 VECTOR rate (64 cycles per instruction and SIMD),
// so a step is bound by the 2 x 32 MFMAs of each Newton-Schulz matrix product, by LDS operand traffic
// and by the number of barrier-separated phases -- not by flops elsewhere.  Hence:
//
//   * 8 waves, one ROLE each.  Waves 0-3 (one per SIMD) do nothing but the two r x r inversions of a
//     step (X: P+ = M^-1, Y: W = (M/beta + I/q)^-1, psmf_block.hip), TWO waves per inversion, wave c owning
//     the 16-column tile column c of its iterate.  Every matrix lives in registers in the MFMA OUTPUT
//     layout ("T-layout": tile (ti, tj), register q of lane l  <->  row 16 ti + (l >> 4) + 4 q,
//     column 16 tj + (l & 15)), which is at the same time the B-operand layout of the next product and
//     -- for a symmetric matrix -- the A-operand layout of the transposed tile.  So
//         R_c = I - M X_c            A = M (registers, built once per step), B = own column of X
//         X'_c = X_c + X^T R_c       A = X (own column + the partner's), B = R_c (registers)
//     need NO LDS operand reads; per iteration a wave publishes its new column (8 doubles per lane)
//     and reads its partner's: one barrier per iteration instead of two, 16 MFMAs per product and SIMD.
//     (X^T instead of X: the iterate is symmetric up to round-off and R' = (I - X M)^T R still
//     squares the residual.)
//   * waves 4-7 own the vector work, laid out so that no product needs a cross-lane reduction over
//     more than two lanes: V (lane = column, 16 rows), A by rows, KA by rows, A^T by columns.
//   * G, Lbar, the rank-2 / rank-1 updates and everything else O(r^2) is elementwise in registers and off
//     the critical path, which per step is:  w = V mu_bar, s, kappa (wave 4) | barrier | M, Newton-
//     Schulz iterations (one barrier each) | v = P+ h, mu (waves 0-1) | barrier.
//
// The direct symmetric sweep (psmf_kernels.hip) stays the fallback whenever the previous inverse is
// not a usable start (first step, transients, no convergence); it runs on all 8 waves through LDS images.
// Reference equations: pypsmf/psmf/psmf.py:104-165, rpsmf.py:116-171.
#pragma once
#include "psmf_block.h"
#include "psmf_sweep.h"
#include "psmf_ns.hip"
#include "psmf_dyn.hip"
#include "psmf_wave.h"     // vector typedefs, DPP / permlane sums, f3_barrier

namespace psmf {

constexpr int F3_NT = 512;
constexpr int F3_S = 34;            // row stride of the row-major 32 x 32 LDS images
constexpr int F3_MAXIT = 12;

// Which T-layout elements lie inside the r x r matrix / on the diagonal.  16 < r <= 32: tile (0, 0) is always inside,
// column tile 1 is inside iff (l & 15) < r - 16, row tile 1 iff (l >> 4) + 4 q < r - 16.  r <= 16 (SMALL): only tile (0, 0)
// holds matrix elements -- column (l & 15) < r, row (l >> 4) + 4 q < r -- the rest of the 32 x 32 iterate is identity
// padding (the same kernel, same speed per timestep as r = 32: the r x r work of a step is latency, not throughput).
// Only the tiles (t, t) hold diagonal elements, where (l & 15) == (l >> 4) + 4 q.  Nine lane predicates (SGPR pairs) in all.
template <int MODE>       // 0: r == 32, nothing to mask (five predicates fewer to keep in SGPR pairs); 1: 16 < r < 32; 2: r <= 16
struct F3Mask {
  static constexpr bool full = MODE == 0;
  static constexpr bool small = MODE == 2;
  bool c1, r1[4], dg[4];      // MODE 2: c1 / r1 describe tile 0 (column / row < r)
};
#define F3_VALID(mk, ti, tj, q) ((mk).full || ((mk).small ? ((ti) == 0 && (tj) == 0 && (mk).r1[q] && (mk).c1) \
                                                          : (((ti) == 0 || (mk).r1[q]) && ((tj) == 0 || (mk).c1))))
#define F3_DIAG(mk, ti, tj, q) (((ti) == (tj)) && (mk).dg[q])

// scalar slots
enum { F3_KAPPA = 0, F3_N, F3_INVN, F3_EE, F3_IOM, F3_Q, F3_IQ, F3_PSCALE, F3_NSC = 16 };

struct F3Lds {
  double* sK;       // RB x RB
  double* sA;       // RB x F3_AS  staging of the K assembly (Aprev)
  double* sKA;      // RB x F3_AS  (upper part of XG)
  double* dump;     // [2 parities][4 NS waves][8 registers][64 lanes]
  float* dumpP;     // [2 parities][4 NS waves][2 tiles][64 lane slots][4]: the same columns, float32, P-layout
  double* img;      // [2 inversions][32 x F3_S]
  double* mub;      // RM
  double* w;        // RM
  double* h;        // RM
  double* a;        // RB
  double* Ka;       // RB
  double* sc;       // F3_NSC
  double* nrm;      // [2][4] residual norms by dump parity and NS wave | 8: ns_tol2, 9: ns_far2, 10: ns_tol2 / 4
  double* hv;       // 2
  double* gp;       // 2
  double* tr;       // 2
  // start predictor of the two inversions (f3_ns_program phase 1; Z = P+ / W):
  double* sab;      // [2 inversions][32][2]  (a_j, b_j) = ((Z h)_j, (Z w)_j) of the step that just ended, by the wave that owns column j
  double* sal;      // [2][32]  alpha = T11 a + T12 b (wave 7, phase 0), ROW-PERMUTED: row 16 ti + lrow + 4 q at 8 lrow + 4 ti + q,
  double* sbe;      // [2][32]  beta  = T12 a + T22 b                    so that a lane's eight rows are 64 contiguous bytes
  float* s32;       // [2][128] the same in float32 for the A operands: alpha (32, permuted) | beta (32, permuted) | (a_j, b_j) pairs (64)
  double* rowbufX;  // 4 RM
  double* rowbufY;  // 4 RM
  int* errflag;
  long long* tick;  // 2: loop start / loop end (s_memrealtime), diagnostics
  long long* acc;   // F3A_*: counters and tick sums of a chained launch (wave 0 alone touches them), flushed to DevState where the launch ends
  long long* hand;  // chain carry: [0] sequence number of the next block, [1] 1: wave 6 saw its cross-Gram announced (f3_chain_next)
};

constexpr int F3_AS = 48;           // row stride of the K-assembly staging (16 mod 32: conflict-free MFMA operand reads)

// dynamic part (block Gram, assembly staging, sweep images and row buffers); the per-step vectors are static LDS
inline size_t blk_filter3_lds_bytes() {
  const size_t doubles = (size_t)RB * RB + 2 * (size_t)RB * F3_AS + 2 * 32 * F3_S + 8 * RM + 2;
  return (doubles * 8 + 15) & ~(size_t)15;
}

// K of a pipelined block from the previous block's quantities (BlockParams; same result as assemble_K in
// psmf_block.hip):  K[0:r,0:r] = G (tracked), K[r+q, r+q'] = Y^T Y (lower part of XG), and the cross block
// K[i, r+q] = sum_m Aprev[m, i] XG[m, q] on the float64 matrix cores: Aprev (RB x r) and the upper part of XG
// (RB x nb) staged once in LDS, one 16 x 16 output tile per wave (16 MFMAs).  Ends with a barrier.
// What changes from block to block of a chained launch (uniform scalars; a modified COPY of BlockParams per block sent
// the whole parameter set through VGPRs and scratch: 3.3 KB of spills, every phase 10-50 % slower).
struct F3Blk {
  long long k0;           // first step of the block is k0 + 1
  int nb, last;
  double* Acoef;
  double* Bcoef;
  const double* XG;
  const double* Aprev;    // nullptr: the previous block of the same launch left its coefficients in sA
  int from_lds, to_lds;   // chain carry (F3Carry): the r x r state arrives from / leaves for the next block through LDS, not DevState
};

// Chain carry (BlockParams::carry, filter3 only).  Between two blocks of ONE launch nobody but this workgroup reads the r x r
// state, so it does not travel through the DevState dump (global stores that the hand-off has to drain, an L2 round trip to read
// them back): every wave parks what it holds in LDS that is idle at a block boundary and picks it up in its next prologue.
//   Xc (wave c's column of its iterate)   dump, parity 0, the wave's own slot            [e][lane]           | [e / 2][lane][2]
//   Xa (its float32 A operands)           dumpP, the wave's own slot of both parities    [e >> 3][.][e & 7][lane] | [e >> 3][.][(e >> 2) & 1][lane][4]
//   G (wave 0), W (wave 2)                dump, parity 1: the slots of waves 0-1 / 2-3   [e][lane]           | [e / 2][lane][2]   (one writer each)
//   V (wave 4), the scalars               the sweep images (nothing sweeps at a boundary) [t][lane]          | [t / 2][lane][2]
//   mu_bar                                stays in L.mub
// Two layouts (f3_carry_d, f3_carry_xa).  Left: psmf_blk_filter3s, an element per read and write.  Right (WIDE): psmf_blk_filter3,
// a lane's elements in 16-byte pieces -- parking and pick-up are ds_write_b128 / ds_read_b128, a quarter-wave per 256 bytes and
// no bank conflict, half (doubles) or a quarter (floats) of the instructions.  WIDE is a compile-time property of the kernel:
// everything that shortens the carried boundary (docs/MEASUREMENTS.md) is built into psmf_blk_filter3 alone, and the other four
// kernels of the family compile to the instructions they had before it.
// The dump, the images and dumpP are read for the last time before the barrier of the block end and written next behind the
// first step's B1; the K assembly touches none of them.  DevState gets the state where the launch ends (f3_ns_dump, f3_v0_dump).
enum { F3C_IQW = 0, F3C_IOM, F3C_PSCALE, F3C_Q, F3C_RHO, F3C_LAM, F3C_PHI, F3C_OMEGA, F3C_EE, F3C_S, F3C_ETA, F3C_N };
struct F3Carry {
  double* Xc;       // [4 waves][8][64]
  float* Xa;        // see f3_carry_xa
  double* G;        // [16][64]
  double* W;        // [16][64]
  double* V;        // [16][64]
  double* sc;       // F3C_*
};
__device__ __forceinline__ F3Carry f3_carry(const F3Lds& L) {
  F3Carry c;
  c.Xc = L.dump;
  c.Xa = L.dumpP;
  c.G = L.dump + 4 * 8 * 64;
  c.W = L.dump + 6 * 8 * 64;
  c.V = L.img;
  c.sc = L.img + 16 * 64;
  return c;
}
// element e of a lane's doubles (Xc: within the wave's slot) / of its float32 A operands (within dumpP)
template <bool WIDE>
__device__ __forceinline__ int f3_carry_d(const int e, const int lane) { return WIDE ? (e >> 1) * 128 + 2 * lane + (e & 1) : e * 64 + lane; }
template <bool WIDE>
__device__ __forceinline__ int f3_carry_xa(const int role, const int e, const int lane) {
  return WIDE ? ((((e >> 3) * 4 + role) * 2 + ((e >> 2) & 1)) * 64 + lane) * 4 + (e & 3) : (((e >> 3) * 4 + role) * 8 + (e & 7)) * 64 + lane;
}

// The inversion waves' share of the DevState dump (valid while ns_valid == 3): what a later launch, or the host, starts from
__device__ __forceinline__ void f3_ns_dump(DevState* st, const int role, const int lane, const double (&Xc)[8], const float (&Xa)[16],
                                           const double (&G)[16], const double (&Wf)[16], const double iq_w) {
  // the state for the next block, as held: coalesced rows
#pragma unroll
  for (int e = 0; e < 8; ++e) st->f3_Xc[role][e * 64 + lane] = Xc[e];
#pragma unroll
  for (int e = 0; e < 16; ++e) st->f3_Xa[role][e * 64 + lane] = Xa[e];
  if (role == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st->f3_G[e * 64 + lane] = G[e];
    if (lane == 0) st->f3_sc[0] = iq_w;
  }
  if (role == 2) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st->f3_W[e * 64 + lane] = Wf[e];
  }
}

// Wave 4's share: V, mu and the scalars.  sc: F3C_* (F3C_IQW unused).  last: the row-major V and Q as well (end of a run)
__device__ __forceinline__ void f3_v0_dump(DevState* st, const F3Lds& L, const int r, const int lane, const long long kdone, const bool last,
                                           const double* V, const double* sc) {
  const int j = lane & 31, hf = lane >> 5;
  const double q = sc[F3C_Q];
#pragma unroll
  for (int t = 0; t < 16; ++t) st->f3_V[t * 64 + lane] = V[t];
  if (last) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int i = 16 * hf + t;
      if (i < r && j < r) {
        st->V[i * r + j] = V[t];
        st->Q[i * r + j] = (i == j) ? q : 0.0;
      }
    }
  } else if (hf == 0 && j < r) {
    st->Q[j * r + j] = q;             // Q = q I: the diagonal is what the next block reads (Q[0])
  }
  if (lane < r) st->mu[lane] = L.mub[lane];
  if (lane == 0) {
    st->f3_sc[1] = sc[F3C_IOM]; st->f3_sc[2] = sc[F3C_PSCALE];
    st->k = kdone;
    st->rho = sc[F3C_RHO]; st->lam = sc[F3C_LAM]; st->phi = sc[F3C_PHI]; st->omega = sc[F3C_OMEGA]; st->ee = sc[F3C_EE];
    st->s_done = sc[F3C_S]; st->eta_done = sc[F3C_ETA]; st->N_done = sc[F3C_N];
    st->ns_valid = 3;
  }
}

// A chained launch that ends between two blocks (dead hand-off): the state of the blocks completed, parked in LDS, goes to
// DevState as a block that does not carry would have left it.  Called by the whole workgroup behind a barrier.
template <bool WIDE>
__device__ __forceinline__ void f3_carry_flush(const BlockParams& b, const F3Lds& L, const long long kdone, const int tid) {
  DevState* st = b.sp.st;
  const int role = tid >> 6, lane = tid & 63;
  const F3Carry cy = f3_carry(L);
  if (role < 4) {
    double Xc[8], G[16], Wf[16];
    float Xa[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) Xc[e] = cy.Xc[role * 512 + f3_carry_d<WIDE>(e, lane)];
#pragma unroll
    for (int e = 0; e < 16; ++e) { Xa[e] = cy.Xa[f3_carry_xa<WIDE>(role, e, lane)]; G[e] = cy.G[f3_carry_d<WIDE>(e, lane)]; Wf[e] = cy.W[f3_carry_d<WIDE>(e, lane)]; }
    f3_ns_dump(st, role, lane, Xc, Xa, G, Wf, cy.sc[F3C_IQW]);
  } else if (role == 4) {
    double V[16], sc[12];
#pragma unroll
    for (int t = 0; t < 16; ++t) V[t] = cy.V[f3_carry_d<WIDE>(t, lane)];
#pragma unroll
    for (int i = 0; i < 12; ++i) sc[i] = cy.sc[i];
    f3_v0_dump(st, L, b.sp.r, lane, kdone, false, V, sc);
  }
}

// Diagnostics of a chained launch (F3Lds::acc).  One launch per block adds its counters and tick sums to DevState when the block
// ends; chained, that was five dependent global round trips of one lane between two blocks with all eight waves waiting at the
// hand-off behind it.  The host reads cnt / dbg after a launch has ended, so a chained launch sums in LDS (wave 0 writes and
// reads every word: psmf_blk_filter3 one lane per word, blk_filter3_body) and adds the sums to DevState once: after its last block, or where a dead hand-off ends it.
enum { F3A_CNT = 0, F3A_DUR = 4, F3A_GAP, F3A_TEND, F3A_BLOCKS, F3A_DBG = 8, F3A_BLK = 13, F3A_N = 17 };   // F3A_BLK: this block's cnt[0..3]
__device__ __forceinline__ void f3_acc_flush(DevState* st, const long long* a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) st->cnt[i] += a[F3A_CNT + i];
  st->cnt[4] += a[F3A_DUR];
  st->cnt[5] += a[F3A_GAP];
  st->cnt[6] = a[F3A_TEND];
  st->cnt[7] += a[F3A_BLOCKS];
#pragma unroll
  for (int i = 0; i < 5; ++i) st->dbg[i] += a[F3A_DBG + i];
  st->dbg[5] += 1;                          // kernel launches
}

// Chain carry: between two blocks of one launch.  blk_chain_next with the ACQUIRE taken out of it: whether the next block's
// cross-Gram is there and the run alive was asked by wave 6 during the last timestep of the block that just ended
// (f3_v_program) and waits in L.hand[1]; a "yes" -- all but the first blocks of a pass -- costs one LDS read instead of an
// agent-scope round trip and a second barrier.  The ANNOUNCE stays where it was: every wave drains its stores (the coefficients
// the apply kernel reads), barrier, flag store -- by wave 6, whose step loop never waits on vmcnt, so nobody waits for the
// store's acknowledgement.  Nothing a carried block reads comes from DevState through the scalar cache (no scalar load of it is
// left inside the chain loop), so there is nothing to invalidate.  Anything but "yes" takes blk_chain_next as it is: announce,
// bounded wait, abort flag, error -7.
__device__ __forceinline__ bool f3_chain_next(const BlockParams& b, const F3Lds& L, const long long seq) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f3_barrier();                     // every wave's stores are complete; the block end's LDS traffic | the next block's set-up
  if (__builtin_amdgcn_readfirstlane((int)L.hand[1]) != 0) {
    if (threadIdx.x == 6 * 64) flag_store(b.flags + 1, seq);           // blocks < seq are complete
    return true;
  }
  return blk_chain_next(b, seq);
}

// What one thread reads of a block's cross-Gram for the K assembly, as ONE group of loads: the upper part (RB x nb, staged in
// LDS as the B operand of the cross block) and Y^T Y (rows RB + q, the lower right corner of K).  Written as a loop with the
// LDS store behind each load, the staging compiled to load, s_waitcnt vmcnt(0), ds_write per trip: six dependent L2 round trips.
constexpr int F3_XS_TRIPS = RB * F3_AS / F3_NT;       // 6
constexpr int F3_AP_TRIPS = RB * 32 / F3_NT;          // 4
constexpr int F3_YY_TRIPS = 6;                        // row q = wave + 8 u, column q2 = lane: no division by the run-time nb
static_assert(F3_XS_TRIPS * F3_NT == RB * F3_AS && F3_AP_TRIPS * F3_NT == RB * 32, "whole trips");
static_assert(F3_YY_TRIPS * (F3_NT / 64) >= F3_AS && F3_AS <= 64 && F3_AS <= XGB, "Y^T Y of the longest block");
struct F3XG {
  double xs[F3_XS_TRIPS], yy[F3_YY_TRIPS];
};
__device__ __forceinline__ void f3_xg_fetch(F3XG& x, const double* XG, const int nb, const int tid) {
#pragma unroll
  for (int u = 0; u < F3_YY_TRIPS; ++u) {
    const int q = max(min((tid >> 6) + 8 * u, nb - 1), 0), q2 = max(min(tid & 63, nb - 1), 0);
    x.yy[u] = xg_load(XG + (size_t)(RB + q) * XGB + q2);
  }
#pragma unroll
  for (int u = 0; u < F3_XS_TRIPS; ++u) {
    const int idx = tid + u * F3_NT, m = idx / F3_AS, q = idx - m * F3_AS;
    x.xs[u] = xg_load(XG + (size_t)m * XGB + max(min(q, nb - 1), 0));
  }
}
__device__ __forceinline__ void f3_xg_stage(const F3XG& x, double* sX, const int nb, const int tid) {
#pragma unroll
  for (int u = 0; u < F3_XS_TRIPS; ++u) {
    const int idx = tid + u * F3_NT, m = idx / F3_AS, q = idx - m * F3_AS;
    sX[m * F3_AS + q] = q < nb ? x.xs[u] : 0.0;
  }
}
__device__ __forceinline__ void f3_xg_corner(const F3XG& x, double* sK, const int r, const int nb, const int tid) {
#pragma unroll
  for (int u = 0; u < F3_YY_TRIPS; ++u) {
    const int q = (tid >> 6) + 8 * u, q2 = tid & 63;
    if (q < nb && q2 < nb) sK[(r + q) * RB + r + q2] = x.yy[u];
  }
}

// Chain carry, fast hand-off (BlockParams::xg_ahead, PSMF_XG_AHEAD): the next block's group of cross-Gram loads is issued in FRONT
// of the hand-off's store drain, so its L2 round trip is the one f3_chain_next's s_waitcnt vmcnt(0) waits for anyway, not a second one
// behind the barrier.  The upper part goes straight into sX -- nothing in a filter3 block touches L.sKA between two assemblies --
// and f3_chain_next's barrier orders it for the cross block's MFMAs; Y^T Y stays in registers across that barrier (sK is still
// being read by waves that have not arrived).  Memory order: wave 6 observed the announcement with an agent-scope load and handed
// it on through L.hand[1] and the barriers of the block end; the agent-scope data loads here are issued after that -- the order
// f3_chain_next's "yes" already relies on, only earlier.  A "yes" here is the same word f3_chain_next reads, so it takes the fast
// path too.  Anything else fetches nothing: the assembly loads behind blk_chain_next's wait as before.
__device__ __forceinline__ bool f3_xg_ahead(const F3Blk& k, const F3Lds& L, F3XG& x, const int tid) {
  if (__builtin_amdgcn_readfirstlane((int)L.hand[1]) == 0) return false;
  f3_xg_fetch(x, k.XG, k.nb, tid);
  f3_xg_stage(x, L.sKA, k.nb, tid);
  return true;
}

// ahead (f3_xg_ahead): x was fetched, and its upper part staged in sX, in front of the hand-off's barrier
// WIDE: the layout of the parked G (F3Carry); close = false (WIDE only): the caller has more LDS words to set up and ends the
// assembly with its own barrier (blk_filter3_body)
template <bool WIDE>
__device__ __forceinline__ void f3_assemble_K(const BlockParams& b, const F3Blk& k, const F3Lds& L, const int r, const int tid, F3XG& x,
                                              const bool ahead, const bool close) {
  const int nb = k.nb, lane = tid & 63, w = tid >> 6, lrow = lane >> 4, lcol = lane & 15;
  double* sK = L.sK;
  double* sA = L.sA;
  double* sX = L.sA + RB * F3_AS;
  const DevState* st = b.sp.st;
  // every global load of the assembly is issued before the first barrier (one L2 round trip, not two)
  // (every address is clamped into the block and the value discarded where it is not wanted: the loads are unconditional, the
  //  trip counts compile-time constants, and nothing waits on vmcnt between the first load and the last)
  double gv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)                                                  // tracked G of the previous block (T-layout dump: an
    gv[u] = k.from_lds ? f3_carry(L).G[f3_carry_d<WIDE>(w + 8 * u, lane)]      // assembled block always follows a filter3 block);
                       : st->f3_G[(w + 8 * u) * 64 + lane];                    // chain carry: where wave 0 parked it
  if (!ahead) f3_xg_fetch(x, k.XG, nb, tid);
  double ap[F3_AP_TRIPS];
  if (k.Aprev) {              // (chained blocks: the previous block left its coefficients in sA)
#pragma unroll
    for (int u = 0; u < F3_AP_TRIPS; ++u) {
      const int idx = tid + u * F3_NT, m = idx >> 5, c = idx & 31;
      ap[u] = k.Aprev[m * r + min(c, r - 1)];
    }
  }
  if (r + nb < RB)            // a full block writes every entry of K below
    for (int idx = tid; idx < RB * RB; idx += F3_NT) sK[idx] = 0.0;
  if (k.Aprev) {
#pragma unroll
    for (int u = 0; u < F3_AP_TRIPS; ++u) {
      const int idx = tid + u * F3_NT, m = idx >> 5, c = idx & 31;
      sA[m * F3_AS + c] = c < r ? ap[u] : 0.0;
    }
  }
  if (!ahead) {
    f3_xg_stage(x, sX, nb, tid);
    __syncthreads();
  } else if (r + nb < RB) {
    f3_barrier();             // the zeroes | the corners.  (sA and sX were complete at the hand-off's barrier.)
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = w + 8 * u;
    const int row = 16 * (e >> 3) + lrow + 4 * (e & 3), col = 16 * ((e >> 2) & 1) + lcol;
    if (row < r && col < r) sK[row * RB + col] = gv[u];
  }
  f3_xg_corner(x, sK, r, nb, tid);
  const int nct = (nb + 15) >> 4;
  if (w < 2 * nct) {
    const int ti = w & 1, ct = w >> 1;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < RB / 4; ++kk)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[(4 * kk + lrow) * F3_AS + 16 * ti + lcol], sX[(4 * kk + lrow) * F3_AS + 16 * ct + lcol], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 16 * ti + lrow + 4 * q, c = 16 * ct + lcol;
      if (i < r && c < nb) { sK[i * RB + r + c] = acc[q]; sK[(r + c) * RB + i] = acc[q]; }
    }
  }
  if (!WIDE || close) f3_barrier();    // (LDS order is all that is needed; __syncthreads() would make wave 6 wait for its flag store's acknowledgement)
}

// A_B (RB x r, row-major) from its LDS staging to global memory by the four vector waves, coalesced: thread t of the 256 stores
// the elements t, t + 256, ... in that order.  The staging address of (m, c) = (idx / r, idx mod r) is carried from trip to trip
// instead of divided out in each: the step (256 / r, 256 mod r) is one division of uniform values, and the first pair comes from
// a float32 reciprocal -- with x = (t + 1/2) / r the fractional part of x lies in [1 / 2r, 1 - 1 / 2r], at least 1 / 64 from an
// integer, and the rounding of the reciprocal and of the product moves x < 2^8 by less than 2^-13: the truncation is
// floor(t / r) exactly.
__device__ __forceinline__ void f3_store_Acoef(double* Acoef, const double* sA, const int r, const int t) {
  // (the step is uniform: scalar registers; the staging address m F3_AS + c is carried as one word beside c)
  const float ir = __builtin_amdgcn_rcpf((float)r);
  const int qs = __builtin_amdgcn_readfirstlane(256 / r), cs = 256 - qs * r, as = qs * F3_AS + cs;
  const int m = (int)(((float)t + 0.5f) * ir);
  int c = t - m * r, at = m * F3_AS + c;
  for (int idx = t; idx < RB * r; idx += 256) {
    coef_store(Acoef + idx, sA[at]);
    c += cs; at += as;
    if (c >= r) { c -= r; at += F3_AS - r; }
  }
}

// Knock-out switches for tools/blk3_knock.hip (timing what each piece costs on the critical path; results are wrong
// with any of them set).  0 in the product: every `if` below folds away.
#ifndef F3_KNOCK
#define F3_KNOCK 0
#endif
// 0 compiles the start predictor out (tools/blk3_knock.hip times the fixed two-iteration schedule; with the predictor in,
// some knock-out masks run into a back-end error of this compiler: "Illegal instruction detected ... $src_shared_base")
#ifndef F3_PREDICT
#define F3_PREDICT 1
#endif

// One Newton-Schulz iteration of tile column C:  R = I - M X_c,  Xn = X_c + X^T R  (see the header).
// Mf: the step's matrix, T-layout, tile (kt, ti) at [(kt * 2 + ti) * 4 + kk]; Xc: own column (T-layout, float64).
// The correction X^T R is formed on the FLOAT32 matrix cores (v_mfma_f32_16x16x4_f32: 32 cycles against 64): R is small,
// so rounding X and R to float32 perturbs the new iterate by ~1e-7 ||X|| ||R|| -- 2e-9 after the first iteration, 1e-11
// or less after the last; the residual itself stays float64.  Xa: the A operands, float32, tile (kt, to) at
// [to * 8 + kt * 4 + kk] for output row tile to, in "P-layout" = T-layout with the 16 lanes of a row permuted by
// pi(4 a + v) = a + 4 v: the float32 MFMA returns row 4 (l >> 4) + v in register v where the float64 one returns
// (l >> 4) + 4 v, and feeding it the rows in that order makes its output land in T-layout.
// Returns this lane's share of ||R_c||_F^2.
template <int C, int FULL>
__device__ __forceinline__ double f3_ns_iter(const double (&Mf)[16], const double (&Xc)[8], const float (&Xa)[16], double (&Xn)[8],
                                             const F3Mask<FULL>& mk) {
  // the two 16 x 16 output tiles of a product are independent accumulator chains: alternate them, so that no MFMA
  // waits for the one before it
  f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
        acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(Mf[(kt * 2 + ti) * 4 + kk], Xc[kt * 4 + kk], acc[ti], 0, 0, 0);
  double R[8];
  double nrm = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = (F3_DIAG(mk, ti, C, q) ? 1.0 : 0.0) - acc[ti][q];
      R[ti * 4 + q] = v;
      nrm += v * v;
    }
  f32x4s d2[2] = {f32x4s{0.f, 0.f, 0.f, 0.f}, f32x4s{0.f, 0.f, 0.f, 0.f}};
  float Rf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) Rf[e] = (float)R[e];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int to = 0; to < 2; ++to)
        if (!(F3_KNOCK & 512)) d2[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(Xa[to * 8 + kt * 4 + kk], Rf[kt * 4 + kk], d2[to], 0, 0, 0);
#pragma unroll
  for (int to = 0; to < 2; ++to)
#pragma unroll
    for (int q = 0; q < 4; ++q) Xn[to * 4 + q] = Xc[to * 4 + q] + (double)d2[to][q];
  return nrm;
}

// Uniform bookkeeping of one step's inversion, identical in both programs (same LDS values, same decisions)
struct F3Ctl {
  bool have_prev;
  int ns_skip;
  int c_ns, c_sw, c_it, c_fail;
};

// residual norms of the iteration whose columns sit in dump parity `par` -> done / failed (uniform over the workgroup)
// The decision reads seven words of L.nrm.  Read where each is compared they made a chain of dependent LDS round trips (the four
// norms | wait | the tolerance | wait | compare, and again for the far bound and the quarter tolerance on the other exits); here
// they come in as ONE group of reads -- f3_norms_read, issued with whatever else the phase reads from LDS -- and F3_DECIDE_FROM
// compares registers: same values, same comparisons.
struct F3Nrm {
  f64x2 nx, ny, tf;       // norms of the X pair | of the Y pair | ns_tol2, ns_far2
  double tq;              // ns_tol2 / 4
};
__device__ __forceinline__ F3Nrm f3_norms_read(const double* nrm, const int par) {
  const f64x2* n2 = reinterpret_cast<const f64x2*>(nrm);      // (16-byte aligned: blk_filter3_body's carve)
  F3Nrm nd;
  nd.nx = n2[par * 2];
  nd.ny = n2[par * 2 + 1];
  nd.tf = n2[4];
  nd.tq = nrm[10];
  return nd;
}
#define F3_DECIDE_FROM(nd_)                                                                                \
  do {                                                                                                     \
    const double nx_ = (nd_).nx[0] + (nd_).nx[1];                                                          \
    const double ny_ = (nd_).ny[0] + (nd_).ny[1];                                                          \
    const double worst_ = fmax(nx_, ny_);                                                                  \
    ++ctl.c_it;                                                                                            \
    /* the thresholds are read from LDS beside the norms (L.nrm[8..10]): as kernel arguments they were kept in VGPRs,   */ \
    /* spilled, and reloaded from scratch in front of every one of these comparisons (scratch_load; s_waitcnt vmcnt(0)) */ \
    if (worst_ < (nd_).tf[0]) done = true;        /* ||R|| below the tolerance BEFORE the update just made */ \
    else if (!(worst_ < (nd_).tf[1]) || it == F3_MAXIT - 1) failed = true;   /* start too far or not converging */ \
    /* ||R_next||_F <= (||R||_F + ||M (Xc - Xa)||) ||R||_F: one more iteration is the last, no check needed */   \
    else last = worst_ * worst_ < (nd_).tq;                                                                \
    if (F3_KNOCK & 1) { done = false; failed = false; last = true; }      /* always exactly two iterations */ \
  } while (0)
#define F3_DECIDE()                                                                                        \
  do {                                                                                                     \
    const F3Nrm nd_d_ = f3_norms_read(L.nrm, par);                                                         \
    F3_DECIDE_FROM(nd_d_);                                                                                 \
  } while (0)

// The direct symmetric sweep of both matrices on all 8 waves (half X: image X, half Y: image Y), in place in
// the images.  Called from both programs at the same point; the images were published before the barrier that
// precedes it.
__device__ __forceinline__ void f3_sweep_images(const F3Lds& L, const int r2, const int tid) {
  const int lt = tid & (WG - 1), c32 = lt & 31, rg = lt >> 5;
  const bool halfX = tid < WG;
  double* im = halfX ? L.img : L.img + 32 * F3_S;
  double A1[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) A1[m] = im[(rg + 8 * m) * F3_S + c32];
  sweep_all<32>(A1, r2, c32, rg, halfX ? L.rowbufX : L.rowbufY, L.errflag);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int i = rg + 8 * m;
    if (i < r2 && c32 < r2) im[i * F3_S + c32] = -A1[m];
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------
// Program of the four inversion waves.  INV 0 = X (P+ = M^-1), 1 = Y (W = (M / beta + I / q)^-1); C = own tile column.
// ------------------------------------------------------------------------------------------------------------
template <int C, int FULL>      // FULL: the F3Mask mode
__device__ __forceinline__ void f3_ns_program(const BlockParams& b, const F3Blk& k, const F3Lds& L, const int inv, const int role, const int lane,
                                              const bool carried) {
  const StepParams& p = b.sp;
  DevState* st = p.st;
  const int r = p.r, r2 = r + (r & 1), tid = 64 * role + lane;
  const int lrow = lane >> 4, lcol = lane & 15;
  const bool isX = inv == 0, isY = inv == 1;
  double* imgX = L.img;
  double* imgY = L.img + 32 * F3_S;
  double G[16], Wf[16], Xc[8];
  float Xa[16];                             // float32 A operands of the correction product (see f3_ns_iter)
  const int pcol = (lcol >> 2) + 4 * (lcol & 3);     // pi(lcol)       // Wf: W of the last step (zero outside r x r): Lbar = (I / q - W / q^2) / omega
  const bool from_lds = k.from_lds != 0;     // chain carry (implies carried): nothing below reads DevState
  constexpr bool WIDE = FULL != 2;           // psmf_blk_filter3: F3Carry in 16-byte pieces (filter3s: an element per access)
  const F3Carry cy = f3_carry(L);
  const double q0 = from_lds ? 0.0 : st->Q[0];
  F3Mask<FULL> mk;
  const int rt = FULL == 2 ? r : r - 16;               // extent of the partially filled tile (tile 0 when r <= 16, else tile 1)
  mk.c1 = lcol < rt;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) { mk.r1[qq] = lrow + 4 * qq < rt; mk.dg[qq] = lcol == lrow + 4 * qq; }
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int row = 16 * ti + lrow + 4 * qq, col = 16 * tj + lcol;
        const bool in = row < r && col < r;
        const int e = (ti * 2 + tj) * 4 + qq;
        G[e] = in ? L.sK[row * RB + col] : 0.0;                              // G_0: exact Gram of the stored C / tracked G
        if (from_lds) {
          if (!WIDE) Wf[e] = cy.W[e * 64 + lane];       // (WIDE: picked up below, two elements per read)
        } else if (carried) {
          Wf[e] = st->f3_W[e * 64 + lane];
        } else {
          // the block starts from Lbar itself (just formed by the sweep): as a W, q I - q^2 Lbar
          const double l0 = imgX[row * F3_S + col];
          Wf[e] = in ? ((row == col ? q0 : 0.0) - q0 * q0 * l0) : 0.0;
        }
      }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int row = 16 * (e >> 2) + lrow + 4 * (e & 3);
    if (from_lds) { if (!WIDE) Xc[e] = cy.Xc[role * 512 + e * 64 + lane]; }
    else Xc[e] = carried ? st->f3_Xc[role][e * 64 + lane] : (row == 16 * C + lcol ? 1.0 : 0.0);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = 16 * ((e >> 2) & 1) + lrow + 4 * (e & 3), cp = 16 * (e >> 3) + pcol;
    if (from_lds) { if (!WIDE) Xa[e] = cy.Xa[f3_carry_xa<false>(role, e, lane)]; }
    else Xa[e] = carried ? st->f3_Xa[role][e * 64 + lane] : (row == cp ? 1.f : 0.f);
  }
  if (WIDE && from_lds) {
    // chain carry: W, the own column and its A operands as the block before parked them (F3Carry), 16 bytes per read
    const f64x2* w2 = reinterpret_cast<const f64x2*>(cy.W) + lane;
    const f64x2* x2 = reinterpret_cast<const f64x2*>(cy.Xc + role * 512) + lane;
    const f32x4s* a4 = reinterpret_cast<const f32x4s*>(cy.Xa) + lane;
#pragma unroll
    for (int e = 0; e < 16; e += 2) { const f64x2 v = w2[(e >> 1) * 64]; Wf[e] = v[0]; Wf[e + 1] = v[1]; }
#pragma unroll
    for (int e = 0; e < 8; e += 2) { const f64x2 v = x2[(e >> 1) * 64]; Xc[e] = v[0]; Xc[e + 1] = v[1]; }
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
      const f32x4s v = a4[f3_carry_xa<true>(role, e, 0) >> 2];
      Xa[e] = v[0]; Xa[e + 1] = v[1]; Xa[e + 2] = v[2]; Xa[e + 3] = v[3];
    }
  }
  if (isX) {
    // <G_0, P> and tr G_0 of the own column, for eta of the first step (Pbar_1 = P + q I); carried: P = beta omega P+
    double g1 = 0.0, t1 = 0.0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int row = 16 * ti + lrow + 4 * qq, col = 16 * C + lcol;
        const bool in = row < r && col < r;
        const double g = G[(ti * 2 + C) * 4 + qq];
        double pv;
        if (carried) pv = Xc[ti * 4 + qq];            // wave 4 applies beta omega
        else pv = st->P[in ? row * r + col : 0];
        g1 += in ? g * pv : 0.0;
        t1 += (row == col) ? g : 0.0;
      }
    g1 = wave_sum_f64_dpp(g1);
    t1 = wave_sum_f64_dpp(t1);
    if (lane == 0) { L.gp[C] = g1; L.tr[C] = t1; }
  }
  f3_barrier();                                                       // ---- init barrier

  // After a step's inversion: W (both columns) into Wf, and for the X waves <G_k, P+> and tr G_k of the own column
  // (eta of the next step).  Runs in the next step's phase 0, while wave 4 forms w, s and kappa, and once more after
  // the last step.  Lbar_{k+1} = (I / q - W / q^2) / omega_k is never formed: M is built from W directly (phase 1).
#define F3_W_AND_TRACES()                                                                                  \
  do {                                                                                                     \
    if (!(F3_KNOCK & 4))                                                                                   \
    _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_)                                                    \
      _Pragma("unroll") for (int tj_ = 0; tj_ < 2; ++tj_) {                                                \
        double wv_[4];                                                                                     \
        if (isY && tj_ == C) {                                                                             \
          _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) wv_[q_] = Xc[ti_ * 4 + q_];                     \
        } else if (w_from_img) {                                                                           \
          _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) wv_[q_] = imgY[(16 * ti_ + lrow + 4 * q_) * F3_S + 16 * tj_ + lcol]; \
        } else {                                                                                           \
          const f64x2* d2_ = reinterpret_cast<const f64x2*>(L.dump) + (size_t)((w_par * 4 + 2 + tj_) * 4) * 64 + lane; \
          const f64x2 v0_ = d2_[(ti_ * 2) * 64], v1_ = d2_[(ti_ * 2 + 1) * 64];                            \
          wv_[0] = v0_[0]; wv_[1] = v0_[1]; wv_[2] = v1_[0]; wv_[3] = v1_[1];                               \
        }                                                                                                  \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                                   \
          Wf[(ti_ * 2 + tj_) * 4 + q_] = F3_VALID(mk, ti_, tj_, q_) ? wv_[q_] : 0.0;                       \
      }                                                                                                    \
    BLK_T(6);                                                                                              \
    if (isX && !(F3_KNOCK & 2)) {                                                                          \
      double g1_ = 0.0;                                                                                    \
      _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_)                                                  \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                                   \
          g1_ += G[(ti_ * 2 + C) * 4 + q_] * Xc[ti_ * 4 + q_];     /* G is zero outside r x r */           \
      g1_ = wave_sum_f64_dpp(g1_);                                                                         \
      if (lane == 0) L.gp[C] = g1_;                                                                        \
    } else if (isY && !(F3_KNOCK & 2)) {                                                                   \
      /* tr G of the own column tile: every inversion wave holds all of G, the W waves have the shorter phase 0 */ \
      double t1_ = 0.0;                                                                                    \
      _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) t1_ += F3_DIAG(mk, C, C, q_) ? G[(C * 2 + C) * 4 + q_] : 0.0; \
      t1_ = wave_sum_f64_dpp(t1_);                                                                         \
      if (lane == 0) L.tr[C] = t1_;                                                                        \
    }                                                                                                      \
  } while (0)

  // psmf_blk_filter3 (WIDE): the same fill and the same traces, straight-line.  Above, the source of every tile -- own column,
  // sweep image, dump -- is chosen tile by tile: sixteen scalar branches in phase 0, the flags they test reloaded from spilled
  // SGPRs, the image's addresses from scratch.  Here W always comes from the dump: a step that sweeps has its Y waves publish
  // their columns of the image there, in the layout an iteration leaves (F3_W_PUBLISH in the sweep's exit, ordered by BF like the
  // iterations' own stores), so the refill from the image is a cold block of that exit and phase 0 never asks where W is.  The one
  // run-time choice left, X or Y wave, is made once for the own column and the trace together.  Same words, same values, same
  // order of summation.
#define F3_W_TILE(ti_, tj_)                                                                                \
  do {                                                                                                     \
    const f64x2* d2_ = reinterpret_cast<const f64x2*>(L.dump) + (size_t)((w_par * 4 + 2 + (tj_)) * 4) * 64 + lane; \
    const f64x2 v0_ = d2_[((ti_) * 2) * 64], v1_ = d2_[((ti_) * 2 + 1) * 64];                              \
    const double wv_[4] = {v0_[0], v0_[1], v1_[0], v1_[1]};                                                \
    _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                                       \
      Wf[((ti_) * 2 + (tj_)) * 4 + q_] = F3_VALID(mk, ti_, tj_, q_) ? wv_[q_] : 0.0;                       \
  } while (0)
#define F3_W_AND_TRACES_WIDE()                                                                             \
  do {                                                                                                     \
    if (!(F3_KNOCK & 4))                                                                                   \
    _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_) F3_W_TILE(ti_, 1 - C);                             \
    if (isX) {                                                                                             \
      if (!(F3_KNOCK & 4))                                                                                 \
      _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_) F3_W_TILE(ti_, C);                               \
      BLK_T(6);                                                                                            \
      if (!(F3_KNOCK & 2)) {                                                                               \
        double g1_ = 0.0;                                                                                  \
        _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_)                                                \
          _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                                 \
            g1_ += G[(ti_ * 2 + C) * 4 + q_] * Xc[ti_ * 4 + q_];     /* G is zero outside r x r */         \
        g1_ = wave_sum_f64_dpp(g1_);                                                                       \
        if (lane == 0) L.gp[C] = g1_;                                                                      \
      }                                                                                                    \
    } else {                                                                                               \
      if (!(F3_KNOCK & 4))                                                                                 \
      _Pragma("unroll") for (int ti_ = 0; ti_ < 2; ++ti_)                                                  \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                                   \
          Wf[(ti_ * 2 + C) * 4 + q_] = F3_VALID(mk, ti_, C, q_) ? Xc[ti_ * 4 + q_] : 0.0;                  \
      BLK_T(6);                                                                                            \
      if (!(F3_KNOCK & 2)) {                                                                               \
        double t1_ = 0.0;                                                                                  \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) t1_ += F3_DIAG(mk, C, C, q_) ? G[(C * 2 + C) * 4 + q_] : 0.0; \
        t1_ = wave_sum_f64_dpp(t1_);                                                                       \
        if (lane == 0) L.tr[C] = t1_;                                                                      \
      }                                                                                                    \
    }                                                                                                      \
  } while (0)
  // the sweep's exit: a Y wave's column of W (just read from the image into Xc) into its slot of dump parity `par`
#define F3_W_PUBLISH(parity_out)                                                                           \
  do {                                                                                                     \
    f64x2* dp_ = reinterpret_cast<f64x2*>(L.dump) + (size_t)(((parity_out) * 4 + role) * 4) * 64 + lane;   \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) dp_[e_ * 64] = f64x2{Xc[2 * e_], Xc[2 * e_ + 1]};    \
  } while (0)

#define F3_ITERATE(parity_out)                                                                             \
  do {                                                                                                     \
    const double nr_ = f3_ns_iter<C, FULL>(Mf, Xc, Xa, Xn, mk);                                               \
    const float nw_ = wave_sum_f32_dpp((float)nr_);                                                        \
    f64x2* dp_ = reinterpret_cast<f64x2*>(L.dump) + (size_t)(((parity_out) * 4 + role) * 4) * 64 + lane;   \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) dp_[e_ * 64] = f64x2{Xn[2 * e_], Xn[2 * e_ + 1]};    \
    f32x4s* pp_ = reinterpret_cast<f32x4s*>(L.dumpP) + (size_t)(((parity_out) * 4 + role) * 2) * 64 + 16 * lrow + pcol; \
    _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_)                                                       \
      pp_[t_ * 64] = f32x4s{(float)Xn[t_ * 4], (float)Xn[t_ * 4 + 1], (float)Xn[t_ * 4 + 2], (float)Xn[t_ * 4 + 3]}; \
    if (lane == 0) L.nrm[(parity_out) * 4 + role] = (double)nw_;                                           \
    _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) Xc[e_] = Xn[e_];                                      \
  } while (0)
#define F3_FETCH_PARTNER(parity_in)                                                                        \
  do {   /* both columns of the new iterate as float32 A operands: own tiles -> output tile C, partner's -> 1 - C */ \
    _Pragma("unroll") for (int w_ = 0; w_ < 2; ++w_) {                                                     \
      const int src_ = w_ == 0 ? role : (role ^ 1);                                                        \
      const int to_ = w_ == 0 ? C : 1 - C;                                                                 \
      const f32x4s* pq_ = reinterpret_cast<const f32x4s*>(L.dumpP) + (size_t)(((parity_in) * 4 + src_) * 2) * 64 + lane; \
      _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_) {                                                   \
        const f32x4s v_ = pq_[t_ * 64];                                                                    \
        Xa[to_ * 8 + t_ * 4 + 0] = v_[0]; Xa[to_ * 8 + t_ * 4 + 1] = v_[1];                                 \
        Xa[to_ * 8 + t_ * 4 + 2] = v_[2]; Xa[to_ * 8 + t_ * 4 + 3] = v_[3];                                 \
      }                                                                                                    \
    }                                                                                                      \
  } while (0)
  F3Ctl ctl = {carried, 0, 0, 0, 0, 0};
  int w_par = 0;
  bool w_from_img = false, fetch_late = false;
  double iq_w;                                              // 1 / q that Wf was formed with
  if (from_lds) iq_w = cy.sc[F3C_IQW];
  else iq_w = carried ? st->f3_sc[0] : 1.0 / q0;
  double kap_prev = 1.0;                                    // kappa of the step that just ended (start predictor)
  bool smw_ok = false;                                      // that step left a = Z h, b = Z w behind (not the first step of a block)
  BLK_T0();
  for (int jb = 0; jb < k.nb; ++jb) {
    // phase 0 (wave 4 forms w, s, kappa meanwhile): what the step that just ended left to do off the critical path
    if (fetch_late) F3_FETCH_PARTNER(w_par);     // (after BF: the partner published it in the last phase it ran)
    if (WIDE) {
      if (jb > 0) F3_W_AND_TRACES_WIDE();
    } else if (jb > 0) F3_W_AND_TRACES();
    BLK_T(7);
    f3_barrier();                                                     // ---- B1
    BLK_T(1);
    // =============================== phase 1: M, first iteration ===============================
    const bool try_ns = ctl.have_prev && p.use_ns && ctl.ns_skip == 0;
    if (!try_ns && ctl.ns_skip > 0) --ctl.ns_skip;
    double Mf[16], Xn[8];
    double hrow[8], wrow[8], h_j = 0.0, mub_j = 0.0, kap_k = 0.0;     // operands of phase F, loaded in phase 2
    int par = 0;
    // One group of LDS reads behind B1: the three scalars and the operands of the start predictor (read whether or not it
    // runs: the addresses are always valid).  M is built under the latency of the predictor's operands; read inside the
    // predictor's branch they waited for kappa's round trip first and M for theirs.
    const double kap_in = L.sc[F3_KAPPA], iom_in = L.sc[F3_IOM], iq_in = L.sc[F3_IQ];
    f64x2 ab = {0.0, 0.0}, al64[4], be64[4];
    f32x4s al32[2], be32[2];
    f32x2s abp0, abp1;
    if (F3_PREDICT) {
      ab = *reinterpret_cast<const f64x2*>(L.sab + 2 * (32 * inv + 16 * C + lcol));
      const float* f32b = L.s32 + 128 * inv;
      al32[0] = *reinterpret_cast<const f32x4s*>(f32b + 8 * lrow); al32[1] = *reinterpret_cast<const f32x4s*>(f32b + 8 * lrow + 4);
      be32[0] = *reinterpret_cast<const f32x4s*>(f32b + 32 + 8 * lrow); be32[1] = *reinterpret_cast<const f32x4s*>(f32b + 32 + 8 * lrow + 4);
      abp0 = *reinterpret_cast<const f32x2s*>(f32b + 64 + 2 * pcol); abp1 = *reinterpret_cast<const f32x2s*>(f32b + 64 + 2 * (16 + pcol));
      const f64x2* alp = reinterpret_cast<const f64x2*>(L.sal + 32 * inv + 8 * lrow);
      const f64x2* bep = reinterpret_cast<const f64x2*>(L.sbe + 32 * inv + 8 * lrow);
#pragma unroll
      for (int e = 0; e < 4; ++e) { al64[e] = alp[e]; be64[e] = bep[e]; }
      __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise moves the reads behind the M build, to where they are waited for)
    }
    {
      const double kap = kap_in, iom = iom_in, iq = iq_in;
      kap_k = kap;
      const double ib = isY ? 1.0 / p.beta : 1.0, dq = isY ? iq : 0.0;
      // M = Lbar + kappa G with Lbar = (I / qw - W / qw^2) / omega, qw = the q that W was formed with; Y: M / beta + I / q
      const double c1 = iom * iq_w, c2 = c1 * iq_w;
      iq_w = iq;
      const double kb = kap * ib, cb = c2 * ib, dv = c1 * ib + dq;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int e = (ti * 2 + tj) * 4 + qq;
            const double m = kb * G[e] - cb * Wf[e];                 // zero outside r x r (G and Wf are)
            if (ti == tj) Mf[e] = m + (F3_DIAG(mk, ti, tj, qq) ? (F3_VALID(mk, ti, tj, qq) ? dv : 1.0) : 0.0);
            else Mf[e] = m;
          }
    }
    if (F3_PREDICT) {
      // (M pinned in front of the predictor, the operands in front of its branch: neither sinks behind the other's wait)
#pragma unroll
      for (int e = 0; e < 16; e += 8)
        asm volatile("" : "+v"(Mf[e]), "+v"(Mf[e + 1]), "+v"(Mf[e + 2]), "+v"(Mf[e + 3]), "+v"(Mf[e + 4]), "+v"(Mf[e + 5]), "+v"(Mf[e + 6]), "+v"(Mf[e + 7]));
      asm volatile("" : "+v"(ab), "+v"(al32[0]), "+v"(al32[1]), "+v"(be32[0]), "+v"(be32[1]), "+v"(abp0), "+v"(abp1),
                        "+v"(al64[0]), "+v"(al64[1]), "+v"(al64[2]), "+v"(al64[3]), "+v"(be64[0]), "+v"(be64[1]), "+v"(be64[2]), "+v"(be64[3]));
    }
    if (F3_PREDICT && try_ns && smw_ok && (p.ns_predict & 4)) {
      // Start of the iteration ("start predictor"): M_k differs from M_{k-1} by the rank-2 change of G
      // (h w^T + w h^T) / N + (ee / N^2) w w^T  -- downdated exactly, Sherman-Morrison-Woodbury with a = Z h, b = Z w left by
      // phase F and the 2 x 2 core folded into alpha, beta by wave 7 in phase 0 --  and, to first order, by the factor
      // kappa_k / kappa_{k-1} on everything (kappa G dominates M):  Z_0 = (kappa_{k-1} / kappa_k) (Z - alpha a^T - beta b^T).
      // Leaves ||I - M Z_0|| ~ 1e-4 .. 1e-3 where the plain start Z leaves 1e-2 .. 1e-1 (and > 1 through the first ~400 steps).
      const double sc = kap_prev * fast_rcp(kap_k);
      const double aj = ab[0], bj = ab[1];
      const float scf = (float)sc;
      // (the identity padding of r < 32 keeps its ones: alpha, a vanish there, only the scale has to be kept off it)
      const bool pc0 = FULL == 0 || (FULL == 2 ? pcol < rt : true), pc1 = FULL == 0 || (FULL == 2 ? false : pcol < rt);
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int e = ti * 4 + qq;
          const double al = al64[e >> 1][e & 1], be = be64[e >> 1][e & 1];
          const bool rok = FULL == 0 || (FULL == 2 ? (ti == 0 && mk.r1[qq]) : (ti == 0 || mk.r1[qq]));
          const double xc = sc * fma(-be, bj, fma(-al, aj, Xc[e]));
          Xc[e] = F3_VALID(mk, ti, C, qq) ? xc : Xc[e];
          const float alf = al32[ti][qq], bef = be32[ti][qq];
          const float x0 = scf * fmaf(-bef, abp0[1], fmaf(-alf, abp0[0], Xa[e]));
          const float x1 = scf * fmaf(-bef, abp1[1], fmaf(-alf, abp1[0], Xa[8 + e]));
          Xa[e] = (rok && pc0) ? x0 : Xa[e];
          Xa[8 + e] = (rok && pc1) ? x1 : Xa[8 + e];
        }
    }
    kap_prev = kap_k;
    if (try_ns) F3_ITERATE(0);
    BLK_T(2);
    f3_barrier();                                                     // ---- B2
    BLK_T(1);
    // =============================== phase 2: second iteration, G update ===============================
    bool done = false, failed = !try_ns, last = false;
    int it = 0;
    fetch_late = false;              // converged: the partner's final column is only needed by the NEXT step -> its phase 0
    // One group of LDS reads behind B2: the partner's column, the norms and thresholds of the decision, and the operands of the
    // Gram update and of phase F.  The update runs under their latency and in front of the decision -- which is uniform, and on
    // which nothing in the update depends: G changes exactly once per step whichever exit the decision takes.  (The reads are
    // unconditional: without a start nothing compares the norms, and the sweep path reloads the operands.)
    F3_FETCH_PARTNER(0);
    const F3Nrm nd0 = f3_norms_read(L.nrm, 0);
    {
      // G_k = G_{k-1} + (h w^T + w h^T) / N + ee w w^T / N^2   (tracked Gram)
      //     = G_{k-1} + u w^T + w hn^T,  u = h / N + (ee / N^2) w,  hn = h / N:  two FMAs per element
      const double iN = L.sc[F3_INVN], ee = L.sc[F3_EE];
      const double e2 = ee * iN * iN;
      double hcol[2], wcol[2], hn[2];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) { hcol[tj] = L.h[16 * tj + lcol]; wcol[tj] = L.w[16 * tj + lcol]; }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) { hrow[ti * 4 + qq] = L.h[16 * ti + lrow + 4 * qq]; wrow[ti * 4 + qq] = L.w[16 * ti + lrow + 4 * qq]; }
      mub_j = L.mub[16 * C + lcol];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) hn[tj] = hcol[tj] * iN;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const double hi = hrow[ti * 4 + qq], wi = wrow[ti * 4 + qq];
          const double ui = hi * iN + e2 * wi;
#pragma unroll
          for (int tj = 0; tj < 2; ++tj)
            if (!(F3_KNOCK & 16)) G[(ti * 2 + tj) * 4 + qq] += ui * wcol[tj] + wi * hn[tj];
        }
      h_j = hcol[C];
    }
    // (left to itself the compiler sinks the update behind the stores of phase F, where nothing waits, and the decision's reads
    //  are then all that stands between B2 and the branch: the values are pinned here)
#pragma unroll
    for (int e = 0; e < 16; e += 8)
      asm volatile("" : "+v"(G[e]), "+v"(G[e + 1]), "+v"(G[e + 2]), "+v"(G[e + 3]), "+v"(G[e + 4]), "+v"(G[e + 5]), "+v"(G[e + 6]), "+v"(G[e + 7]));
    if (try_ns) {
      F3_DECIDE_FROM(nd0);
      if (!done && !failed) {
        if (!(F3_KNOCK & 256)) F3_ITERATE(1);
        par = 1;
        it = 1;
        if (last) { done = true; fetch_late = true; ++ctl.c_it; }
      }
    }
    BLK_T(3);
    // =============================== further iterations (only when the outcome is not known yet) ===============================
    if (!done) {
      f3_barrier();                                                   // ---- B3
      BLK_T(1);
      while (try_ns && !done && !failed) {
        F3_DECIDE();
        if (done) fetch_late = true;
        if (done || failed) break;
        F3_FETCH_PARTNER(par);
        F3_ITERATE(par ^ 1);
        par ^= 1;
        ++it;
        if (last) { done = true; fetch_late = true; ++ctl.c_it; break; }
        f3_barrier();
      }
    }
    BLK_T(4);
    // `par` = parity of the dump that holds the columns published by the last iteration that ran
    const bool from_img = !done;
    if (!done) {
      if (try_ns) { ++ctl.c_fail; ctl.ns_skip = p.ns_skip_n; }
      ++ctl.c_sw;
      double* im = isX ? imgX : imgY;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) im[(16 * ti + lrow + 4 * qq) * F3_S + 16 * C + lcol] = Mf[(ti * 2 + C) * 4 + qq];
      f3_barrier();
      f3_sweep_images(L, r2, tid);
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int row = 16 * ti + lrow + 4 * qq;
          Xc[ti * 4 + qq] = im[row * F3_S + 16 * C + lcol];
#pragma unroll
          for (int to = 0; to < 2; ++to) Xa[to * 8 + ti * 4 + qq] = (float)im[row * F3_S + 16 * to + pcol];
        }
      if (WIDE && isY) F3_W_PUBLISH(par);        // (the next phase 0 finds W where an iteration would have left it)
    } else {
      ++ctl.c_ns;
    }
    ctl.have_prev = true;
    // =============================== phase F: v = P+ h, mu (the only work between the inversion and the next step) ===============================
    w_par = par;
    w_from_img = from_img;
    if (!(F3_KNOCK & 8)) {
      // a = Z h, b = Z w of the own column (by symmetry) for the next step's start predictor; X waves: a is v = P+ h,
      // mu_k = mu_bar + kappa v (psmf.py:155-159); h.v for omega (rPSMF only)
      double vp0 = 0.0, vp1 = 0.0, vq0 = 0.0, vq1 = 0.0;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        vp0 += Xc[qq] * hrow[qq]; vp1 += Xc[4 + qq] * hrow[4 + qq];
        vq0 += Xc[qq] * wrow[qq]; vq1 += Xc[4 + qq] * wrow[4 + qq];
      }
      const double vp = xor32_sum_f64(xor16_sum_f64(vp0 + vp1));
      // (the lane index made opaque here: the LDS / global addresses and the lane predicate of the stores below are then formed
      //  on the spot -- three integer instructions -- instead of being hoisted out of the step loop, spilled, and reloaded from
      //  scratch right in front of the barrier that ends the step: scratch_load; s_waitcnt vmcnt(0); ds_write, three times per step)
      int lane_f = lane;
      asm volatile("" : "+v"(lane_f));
      const int lcol = lane_f & 15, lrow = lane_f >> 4;
      const int j = 16 * C + lcol;
      if (isX) {
        const double mu_new = mub_j + kap_k * vp;
        if (lrow == 0 && j < r) {
          L.mub[j] = mu_new;                    // random walk: mu_bar_{k+1} = mu_k
          if (p.mu_hist) p.mu_hist[(size_t)(k.k0 + jb + 1 - p.series_t0) * r + j] = mu_new;
        }
        if (p.robust) {
          const double hvp = wave_sum_f64_dpp((lrow == 0) ? h_j * vp : 0.0);
          if (lane == 0) L.hv[C] = hvp;
        }
      }
      if (F3_PREDICT && (p.ns_predict & 1)) {
        const double vq = xor32_sum_f64(xor16_sum_f64(vq0 + vq1));
        if (lrow == 0) *reinterpret_cast<f64x2*>(L.sab + 2 * (32 * inv + j)) = f64x2{vp, vq};
      }
      smw_ok = true;
    }
    BLK_T(5);
    f3_barrier();                                                     // ---- BF
    BLK_T(1);
  }
  BLK_TOUT();
  // ---- block end ----
  if (fetch_late) F3_FETCH_PARTNER(w_par);
  if (WIDE) {
    if (k.nb > 0) F3_W_AND_TRACES_WIDE();
  } else if (k.nb > 0) F3_W_AND_TRACES();
  f3_barrier();                       // wave 4 has published pscale and 1 / omega of the last step
  const double ps = L.sc[F3_PSCALE], iom = L.sc[F3_IOM];
  if (k.to_lds) {
    // chain carry: the next block of this launch picks the state up from LDS (every reader of the dump is behind the barrier above)
    if (WIDE) {
      f64x2* x2 = reinterpret_cast<f64x2*>(cy.Xc + role * 512) + lane;
      f32x4s* a4 = reinterpret_cast<f32x4s*>(cy.Xa) + lane;
#pragma unroll
      for (int e = 0; e < 8; e += 2) x2[(e >> 1) * 64] = f64x2{Xc[e], Xc[e + 1]};
#pragma unroll
      for (int e = 0; e < 16; e += 4) a4[f3_carry_xa<true>(role, e, 0) >> 2] = f32x4s{Xa[e], Xa[e + 1], Xa[e + 2], Xa[e + 3]};
      if (role == 0) {
        f64x2* g2 = reinterpret_cast<f64x2*>(cy.G) + lane;
#pragma unroll
        for (int e = 0; e < 16; e += 2) g2[(e >> 1) * 64] = f64x2{G[e], G[e + 1]};
        if (lane == 0) cy.sc[F3C_IQW] = iq_w;
      }
      if (role == 2) {
        f64x2* w2 = reinterpret_cast<f64x2*>(cy.W) + lane;
#pragma unroll
        for (int e = 0; e < 16; e += 2) w2[(e >> 1) * 64] = f64x2{Wf[e], Wf[e + 1]};
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) cy.Xc[role * 512 + e * 64 + lane] = Xc[e];
#pragma unroll
      for (int e = 0; e < 16; ++e) cy.Xa[f3_carry_xa<false>(role, e, lane)] = Xa[e];
      if (role == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) cy.G[e * 64 + lane] = G[e];
        if (lane == 0) cy.sc[F3C_IQW] = iq_w;
      }
      if (role == 2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) cy.W[e * 64 + lane] = Wf[e];
      }
    }
  } else {
    f3_ns_dump(st, role, lane, Xc, Xa, G, Wf, iq_w);
  }
  if (k.last) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int row = 16 * ti + lrow + 4 * qq, col = 16 * C + lcol;
        if (row < r && col < r) {
          const int idx = row * r + col;
          if (isX) {
            st->XpX[idx] = Xc[ti * 4 + qq];
            st->P[idx] = ps * Xc[ti * 4 + qq];
            st->G[idx] = G[(ti * 2 + C) * 4 + qq];
          } else {
            st->XpY[idx] = Xc[ti * 4 + qq];
            st->Lbar[idx] = ((row == col ? iq_w : 0.0) - Wf[(ti * 2 + C) * 4 + qq] * iq_w * iq_w) * iom;
          }
        }
      }
  }
  // (thread 0: blk_filter3_body adds them to DevState, or to the sums of a chained launch)
  if (role == 0 && lane == 0) { L.acc[F3A_BLK] = ctl.c_ns; L.acc[F3A_BLK + 1] = ctl.c_sw; L.acc[F3A_BLK + 2] = ctl.c_it; L.acc[F3A_BLK + 3] = ctl.c_fail; }
#undef F3_ITERATE
#undef F3_FETCH_PARTNER
#undef F3_W_AND_TRACES
#undef F3_W_AND_TRACES_WIDE
#undef F3_W_TILE
#undef F3_W_PUBLISH
}

// ------------------------------------------------------------------------------------------------------------
// Program of the four vector waves: 4 = V and every scalar, 5 = A by rows, 6 = KA by rows, 7 = A^T by columns.
// ------------------------------------------------------------------------------------------------------------
template <int ROLE, bool WIDE>       // WIDE: psmf_blk_filter3 (see F3Carry)
__device__ __forceinline__ void f3_v_program(const BlockParams& b, const F3Blk& k, const F3Lds& L, const int lane, const bool carried) {
  const StepParams& p = b.sp;
  DevState* st = p.st;
  constexpr int role = ROLE;
  const int r = p.r, r2 = r + (r & 1), tid = 64 * role + lane;
  const double dd = (double)p.d, idd = 1.0 / dd;
  constexpr bool isV0 = ROLE == 4, isV1 = ROLE == 5, isV2 = ROLE == 6, isV3 = ROLE == 7;
  // Each vector wave shares its SIMD with an inversion wave.  At equal priority its ~60 VALU instructions per phase were
  // issued about one per MFMA (64 cycles) and the barrier waited for THEM (3.7k cycles against 3.1k, stamps); with
  // priority they issue back to back and cost the MFMA stream a few hundred cycles instead.
  __builtin_amdgcn_s_setprio(3);
  // persistent registers:  V0: [0,16) V[16 hf + t][j]   V1: A[m][c]   V2: KA[m][c]   V3: A[32 hf + t][c]
  double pr[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) pr[i] = 0.0;
  // wave 4's running scalars (every lane holds the same values)
  double kappa = 0.0, Nk = 0.0, invN = 0.0, s_k = 0.0, eta_k = 0.0, ee_k = 0.0, phi = 1.0, omega = 1.0, pscale = 1.0, wj = 0.0;
  const bool from_lds = k.from_lds != 0;       // chain carry (implies carried): nothing below reads DevState
  const F3Carry cy = f3_carry(L);
  double q, rho, lam;
  if (from_lds) { q = cy.sc[F3C_Q]; rho = cy.sc[F3C_RHO]; lam = cy.sc[F3C_LAM]; }
  else { q = st->Q[0]; rho = st->rho; lam = st->lam; }      // Q = q I (checked by the host)
  double iom0 = 1.0;                    // 1 / omega of the last step of the previous block (carried W is not yet divided by it)
  double kap7 = 1.0;                    // wave 7: kappa of the step that just ended
  if (isV0) {
    const int j = lane & 31, hf = lane >> 5;
    if (from_lds) {
#pragma unroll
      for (int t = 0; t < 16; t += 2) {
        if (WIDE) { const f64x2 v = reinterpret_cast<const f64x2*>(cy.V)[(t >> 1) * 64 + lane]; pr[t] = v[0]; pr[t + 1] = v[1]; }
        else { pr[t] = cy.V[t * 64 + lane]; pr[t + 1] = cy.V[(t + 1) * 64 + lane]; }
      }
      iom0 = cy.sc[F3C_IOM];
      pscale = cy.sc[F3C_PSCALE];
    } else if (carried) {
#pragma unroll
      for (int t = 0; t < 16; ++t) pr[t] = st->f3_V[t * 64 + lane];
      iom0 = st->f3_sc[1];
      pscale = st->f3_sc[2];
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = 16 * hf + t;
        const bool in = i < r && j < r;
        const double v = st->V[in ? i * r + j : 0];
        pr[t] = in ? v : 0.0;
      }
    }
  } else if (isV1) {
#pragma unroll
    for (int c = 0; c < 32; ++c) pr[c] = (lane == c && c < r) ? 1.0 : 0.0;
  } else if (isV2) {
#pragma unroll
    for (int c = 0; c < 32; ++c) pr[c] = (c < r) ? L.sK[lane * RB + c] : 0.0;
  } else {
    const int c = lane & 31, hf = lane >> 5;
#pragma unroll
    for (int t = 0; t < 32; ++t) pr[t] = (32 * hf + t == c && c < r) ? 1.0 : 0.0;
  }
  f3_barrier();                                                       // ---- init barrier

  // scalars of the step that just ended (omega needs v = P+ h): rpsmf.py:155-171
#define F3_V0_FINISH_PREV()                                               \
  do {                                                                    \
    omega = 1.0;                                                          \
    pscale = 1.0;                                                         \
    if (p.robust) {                                                       \
      const double hPh_ = L.hv[0] + L.hv[1];                              \
      const double quad_ = kappa * ee_k - kappa * kappa * hPh_;           \
      omega = (lam + quad_) * fast_rcp(lam + dd);                         \
      pscale = p.beta * omega;                                            \
      rho *= omega;                                                       \
      q *= omega;                                                         \
      if (!p.fixed_lambda) lam += dd;                                     \
    }                                                                     \
  } while (0)

  F3Ctl ctl = {carried, 0, 0, 0, 0, 0};
  if (role == 4 && lane == 0) L.tick[0] = (long long)__builtin_amdgcn_s_memrealtime();
  BLK_T0();
  for (int jb = 0; jb < k.nb; ++jb) {
    // =============================== phase 0 ===============================
    // chain carry, last timestep of a block that hands on (wave 6, which has the shortest phases): is the next block's cross-Gram
    // announced, is the run alive?  Asked here, answered into L.hand[1] in phase 2: f3_chain_next finds it there
    const bool poll = isV2 && k.to_lds && jb == k.nb - 1;
    long long poll_xg = 0, poll_ab = 1;
    if (poll) { poll_xg = flag_load(b.flags + 0); poll_ab = flag_load(b.flags + 2); }
    double cm = 0.0;                       // V1: a_m, V2: (K a)_m  (kept for the rank-1 update of phase 2)
    if (isV0 && !(F3_KNOCK & 1024)) {
      const int j = lane & 31, hf = lane >> 5;
      double iom = iom0;
      if (jb > 0) { F3_V0_FINISH_PREV(); iom = fast_rcp(omega); }
      double part0 = 0.0, part1 = 0.0;
#pragma unroll
      for (int t = 0; t < 16; t += 2) {
        part0 += pr[t] * L.mub[16 * hf + t];
        part1 += pr[t + 1] * L.mub[16 * hf + t + 1];
      }
      const double part = part0 + part1;
      s_k = wave_sum_f64_dpp(part * L.mub[j]);                          // s = mu_bar^T V mu_bar: both halves hold their 16 rows' share
      kappa = fast_rcp(rho + s_k);
      if (lane == 0) { L.sc[F3_KAPPA] = kappa; L.sc[F3_IOM] = iom; L.sc[F3_Q] = q; L.sc[F3_IQ] = fast_rcp(q); }
      wj = part;                                                        // this half's share of w_j; completed in phase 1
    } else if ((isV1 || isV2) && !(F3_KNOCK & 32)) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      // psmf_blk_filter3 (WIDE): the compiler already reads mu_bar sixteen bytes at a time, but three or four reads per group into
      // the same registers, each group waited for before the next is issued: five LDS round trips in a row in the phase these two
      // waves arrive last in.  All sixteen reads as ONE group, pinned in front of the products (64 more live registers, which
      // the vector waves have).  Same words, same products, same four sums.
      if (WIDE) {
        double mb[32];
        const f64x2* m2 = reinterpret_cast<const f64x2*>(L.mub);        // (16-byte aligned: blk_filter3_body's carve)
#pragma unroll
        for (int c = 0; c < 32; c += 2) { const f64x2 v = m2[c >> 1]; mb[c] = v[0]; mb[c + 1] = v[1]; }
#pragma unroll
        for (int c = 0; c < 32; c += 16)
          asm volatile("" : "+v"(mb[c]), "+v"(mb[c + 1]), "+v"(mb[c + 2]), "+v"(mb[c + 3]), "+v"(mb[c + 4]), "+v"(mb[c + 5]), "+v"(mb[c + 6]), "+v"(mb[c + 7]),
                            "+v"(mb[c + 8]), "+v"(mb[c + 9]), "+v"(mb[c + 10]), "+v"(mb[c + 11]), "+v"(mb[c + 12]), "+v"(mb[c + 13]), "+v"(mb[c + 14]), "+v"(mb[c + 15]));
#pragma unroll
        for (int c = 0; c < 32; c += 4) {
          a0 += pr[c] * mb[c];
          a1 += pr[c + 1] * mb[c + 1];
          a2 += pr[c + 2] * mb[c + 2];
          a3 += pr[c + 3] * mb[c + 3];
        }
      } else {
#pragma unroll
      for (int c = 0; c < 32; c += 4) {
        a0 += pr[c] * L.mub[c];
        a1 += pr[c + 1] * L.mub[c + 1];
        a2 += pr[c + 2] * L.mub[c + 2];
        a3 += pr[c + 3] * L.mub[c + 3];
      }
      }
      const double dot = (a0 + a1) + (a2 + a3);
      if (isV1) {
        cm = (lane == r + jb ? 1.0 : 0.0) - dot;                        // a_j = u_{r+j} - A mu_bar
        L.a[lane] = cm;
        coef_store(k.Bcoef + (size_t)jb * RB + lane, dot);              // y_hat_j = Z b_j
      } else {
        cm = L.sK[lane * RB + r + jb] - dot;                            // K a_j
        L.Ka[lane] = cm;
      }
    }
    else if (F3_PREDICT && isV3 && (p.ns_predict & 2)) {
      // Start predictor of the two inversions (f3_ns_program, phase 1): the 2 x 2 core of the rank-2 downdate.  With a = Z h,
      // b = Z w (left by the inversion waves in phase F), U = [h w] and G_k - G_{k-1} = U K U^T, K = [[0, 1/N], [1/N, ee/N^2]]:
      //   (M + kappa U K U^T)^-1 = Z - [a b] T [a b]^T,   T = ((kappa K)^-1 + U^T Z U)^-1,   (kappa K)^-1 = [[-ee, N], [N, 0]] / kappa
      // (W: M / beta, so kappa / beta).  Published as alpha = T11 a + T12 b, beta = T12 a + T22 b; lanes 0-31: P+, 32-63: W.
      const int j = lane & 31, hf = lane >> 5;
      double al = 0.0, be = 0.0;
      f64x2 ab7 = {0.0, 0.0};
      if (jb > 0) {
        ab7 = *reinterpret_cast<const f64x2*>(L.sab + 2 * lane);
        const double a = ab7[0], bb = ab7[1], hj = L.h[j], wv = L.w[j];
        const double ha = xor16_sum_f64(row_sum_f64_dpp(hj * a)), hb = xor16_sum_f64(row_sum_f64_dpp(hj * bb));
        const double wb = xor16_sum_f64(row_sum_f64_dpp(wv * bb));
        const double ik = (hf ? p.beta : 1.0) * fast_rcp(kap7);
        const double s11 = ha - L.sc[F3_EE] * ik, s12 = hb + L.sc[F3_N] * ik;
        const double idet = fast_rcp(s11 * wb - s12 * s12);
        const double t11 = wb * idet, t12 = -s12 * idet, t22 = s11 * idet;
        al = t11 * a + t12 * bb;
        be = t12 * a + t22 * bb;
      }
      const int pj = 32 * hf + 8 * (j & 3) + 4 * (j >> 4) + ((j >> 2) & 3);
      L.sal[pj] = al;
      L.sbe[pj] = be;
      float* f32b = L.s32 + 128 * hf;
      f32b[pj - 32 * hf] = (float)al;
      f32b[32 + pj - 32 * hf] = (float)be;
      *reinterpret_cast<f32x2s*>(f32b + 64 + 2 * j) = f32x2s{(float)ab7[0], (float)ab7[1]};
    }
    BLK_T(0);
    f3_barrier();                                                     // ---- B1
    BLK_T(1);
    // =============================== phase 1 ===============================
    const bool try_ns = ctl.have_prev && p.use_ns && ctl.ns_skip == 0;
    if (!try_ns && ctl.ns_skip > 0) --ctl.ns_skip;
    int par = 0;
    if (isV3) kap7 = L.sc[F3_KAPPA];                                    // (stable from B1 to the next step's phase 0)
    if (isV3 && !(F3_KNOCK & 64)) {
      const int c = lane & 31, hf = lane >> 5;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int t = 0; t < 32; t += 4) {
        a0 += pr[t] * L.Ka[32 * hf + t];
        a1 += pr[t + 1] * L.Ka[32 * hf + t + 1];
        a2 += pr[t + 2] * L.Ka[32 * hf + t + 2];
        a3 += pr[t + 3] * L.Ka[32 * hf + t + 3];
      }
      const double part = (a0 + a1) + (a2 + a3);
      const double hc = xor32_sum_f64(part);                            // h = A^T K a
      if (hf == 0) L.h[c] = hc;
    } else if (isV1) {
      // ee = a . K a: wave 5 is idle in this phase, wave 7's product above is the one the barrier waits for
      const double e1 = wave_sum_f64_dpp(cm * L.Ka[lane]);
      if (lane == 0) L.sc[F3_EE] = e1;
    } else if (isV0) {
      wj = xor32_sum_f64(wj);                                           // w = V mu_bar
      if (lane < 32) L.w[lane] = wj;
      // eta, N (psmf.py:121-128): <G, Pbar> and tr G were left by the X waves in phase 0
      const double gpv = pscale * (L.gp[0] + L.gp[1]) + q * (L.tr[0] + L.tr[1]);
      eta_k = rho + gpv * idd;
      Nk = s_k + eta_k;
      invN = fast_rcp(Nk);
      if (lane == 0) { L.sc[F3_N] = Nk; L.sc[F3_INVN] = invN; }
    }
    BLK_T(2);
    f3_barrier();                                                     // ---- B2
    BLK_T(1);
    // =============================== phase 2 ===============================
    bool done = false, failed = !try_ns, last = false;
    int it = 0;
    // as in f3_ns_program: the decision's words are read with the operands of the rank-1 update, the update runs, then the decision
    const F3Nrm nd0 = f3_norms_read(L.nrm, 0);
    if (F3_KNOCK & 128) {
    } else if (isV3) {
      const int c = lane & 31, hf = lane >> 5;
      const double wn = L.w[c] * L.sc[F3_INVN];
#pragma unroll
      for (int t = 0; t < 32; ++t) pr[t] += L.a[32 * hf + t] * wn;
    } else if (isV1 || isV2) {
      // rank-1 updates of A (rows) and KA (rows): psmf.py:130-133 in coefficient space
      const double cn = cm * L.sc[F3_INVN];
#pragma unroll
      for (int c = 0; c < 32; ++c) pr[c] += cn * L.w[c];
    } else if (isV0) {
      const int hf = lane >> 5;
      ee_k = L.sc[F3_EE];
      phi = 1.0;
      double vscale = 1.0;
      if (p.robust) {
        phi = (lam + ee_k * invN) * fast_rcp(lam + dd);                 // rpsmf.py:133-138
        vscale = p.alpha * phi;
      }
      const double wjn = wj * invN;
#pragma unroll
      for (int t = 0; t < 16; ++t) pr[t] = vscale * (pr[t] - L.w[16 * hf + t] * wjn);   // psmf.py:135-138
    }
#pragma unroll
    for (int t = 0; t < (isV0 ? 16 : 32); t += 8)       // (pinned in front of the decision, see f3_ns_program)
      asm volatile("" : "+v"(pr[t]), "+v"(pr[t + 1]), "+v"(pr[t + 2]), "+v"(pr[t + 3]), "+v"(pr[t + 4]), "+v"(pr[t + 5]), "+v"(pr[t + 6]), "+v"(pr[t + 7]));
    if (try_ns) {
      F3_DECIDE_FROM(nd0);
      if (!done && !failed) {
        par = 1;
        it = 1;
        if (last) done = true;
      }
    }
    if (poll && lane == 0) L.hand[1] = (poll_ab == 0 && poll_xg >= L.hand[0]) ? 1 : 0;
    // A_B: wave 5's rows are final here in the block's last timestep, and nothing inside a step reads sA (the assembly is done
    // with it before the first one).  Staged now, BF orders the rows for the four vector waves, whose coefficient stores then
    // leave in FRONT of the barrier of the block end and drain beside the inversion waves' last W and traces.
    if (WIDE && isV1 && jb == k.nb - 1) {
#pragma unroll
      for (int c = 0; c < 32; ++c) L.sA[lane * F3_AS + c] = pr[c];       // (a strided global store per column took ~4 us)
    }
    BLK_T(3);
    if (!done) {
      f3_barrier();                                                   // ---- B3
      while (try_ns && !done && !failed) {
        F3_DECIDE();
        if (done || failed) break;
        par ^= 1;
        ++it;
        if (last) { done = true; break; }
        f3_barrier();
      }
    }
    if (!done) {
      if (try_ns) { ++ctl.c_fail; ctl.ns_skip = p.ns_skip_n; }
      ++ctl.c_sw;
      f3_barrier();
      f3_sweep_images(L, r2, tid);
    } else {
      ++ctl.c_ns;
    }
    ctl.have_prev = true;
    BLK_T(4);
    f3_barrier();                                                     // ---- BF
    BLK_T(1);
  }
  BLK_TOUT();
  if (role == 4 && lane == 0) L.tick[1] = (long long)__builtin_amdgcn_s_memrealtime();

  // ---- block end ----
  // A_B (wave 5's rows) leaves through LDS: all four vector waves store it, coalesced.  WIDE: staged in the last timestep
  // (phase 2; a block has at least one: the host cuts a run into ceil(steps / B) blocks), stored in front of the barrier
  if (WIDE) f3_store_Acoef(k.Acoef, L.sA, r, tid - 256);
  if (isV0) {
    if (k.nb > 0) F3_V0_FINISH_PREV();
    if (lane == 0) { L.sc[F3_PSCALE] = pscale; L.sc[F3_IOM] = fast_rcp(omega); L.sc[F3_Q] = q; }
  } else if (!WIDE && isV1) {
#pragma unroll
    for (int c = 0; c < 32; ++c) L.sA[lane * F3_AS + c] = pr[c];       // (a strided global store per column took ~4 us)
  }
  f3_barrier();
  if (isV0) {
    double sc[12];
    sc[F3C_IQW] = 0.0; sc[F3C_IOM] = L.sc[F3_IOM]; sc[F3C_PSCALE] = pscale; sc[F3C_Q] = q; sc[F3C_RHO] = rho; sc[F3C_LAM] = lam;
    sc[F3C_PHI] = phi; sc[F3C_OMEGA] = omega; sc[F3C_EE] = ee_k; sc[F3C_S] = s_k; sc[F3C_ETA] = eta_k; sc[F3C_N] = Nk;
    if (k.to_lds) {
      // chain carry: V and the scalars wait in the sweep images (mu_bar stays in L.mub); sc[F3C_IQW] is wave 0's
#pragma unroll
      for (int t = 0; t < 16; t += 2) {
        if (WIDE) reinterpret_cast<f64x2*>(cy.V)[(t >> 1) * 64 + lane] = f64x2{pr[t], pr[t + 1]};
        else { cy.V[t * 64 + lane] = pr[t]; cy.V[(t + 1) * 64 + lane] = pr[t + 1]; }
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 1; i < 12; ++i) cy.sc[i] = sc[i];
      }
    } else {
      f3_v0_dump(st, L, r, lane, k.k0 + k.nb, k.last != 0, pr, sc);
    }
    if (lane == 0 && *L.errflag && st->err == 0) st->err = (int)(k.k0 + 1);
  }
  // (filter3s: A_B left through LDS before the barrier above)
  if (!WIDE) for (int idx = tid - 256; idx < RB * r; idx += 256) { const int m = idx / r, c = idx - m * r; coef_store(k.Acoef + idx, L.sA[m * F3_AS + c]); }
#undef F3_V0_FINISH_PREV
}

}  // namespace psmf
