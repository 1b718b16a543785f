// The series buffers of a handle (Y, y_hat, observation mask, the mean and (s, eta) histories): allocation, uploads, downloads and
// the reductions over stored rows -- one body each for a resident handle (the whole series on the device, row = step) and for a
// series ring (psmf_series_ring, DESIGN section 3a: n_slots windows of `chunk` rows, fed chunk by chunk).  The two differ in which
// device row a step lives in and in which stream a read sits behind; both answers come from series_span / mu_hist_row / upload_span,
// and the entry points are loops over the pieces they return.  A resident handle is the degenerate case: one piece, row = step, the
// compute stream, after psmf_sync.
#include "psmf_host.h"
#include "psmf_series_kernels.hip"       // psmf_cast_rows, psmf_sq_error_k, psmf_masked_metrics_k

#include <string>
#include <vector>

namespace {

// ---- addressing ----------------------------------------------------------------------------------------------------------------
// Ring: chunk c of the stream lives in slot c % ring_slots; step t (0-based) of it in row slot * ring_chunk + t % ring_chunk of the
// series buffers, which is row t - series_t0 with series_t0 = (c - slot) * ring_chunk: what the kernels index by.
int64_t ring_t0(const psmf_filter* h, int64_t c) { return (c - c % h->ring_slots) * h->ring_chunk; }

// The histories a step writes one row AHEAD of the series row it reads -- the posterior mean of step k in row k, the persistent
// kernel's (s, eta) of the next step -- get chunk + 1 rows per slot, so that a slot's last row is not the first row of its
// neighbour (which may hold a chunk that has not been read back yet): the slot's base is moved by `slot` rows.
void ring_point(const psmf_filter* h, StepParams& sp, int64_t c) {
  const int64_t slot = c % h->ring_slots;
  sp.series_t0 = ring_t0(h, c);
  sp.mu_hist = h->mu_hist + (size_t)slot * h->cfg.r;
  if (h->sc_hist) sp.sc_hist = h->sc_hist + 2 * (size_t)slot;
}

// is row `off` (0-based, within its chunk) of chunk c on the device?  mask: of the observation mask instead of the series
bool ring_has(const psmf_filter* h, int64_t c, int64_t off, bool mask = false) {
  const psmf_filter::RingSlot& s = h->ring[(size_t)(c % h->ring_slots)];
  return s.chunk == c && off < (mask ? s.mrows : s.rows);
}

// The steps [t0, t0 + nt) of a caller's range as the device holds them: a resident handle has one piece, a ring one per chunk.
struct SeriesPiece {
  int64_t t0, nt;        // steps of the caller's range
  size_t row;            // row of step t0 in Y / YP / mask
  size_t hist_row;       // row of step t0 in mu_hist / sc_hist (a ring: chunk + 1 of them per slot, ring_point)
  int64_t c; int slot;   // ring: the chunk and its slot (resident: 0, 0)
};
struct SeriesSpan { hipStream_t stream; std::vector<SeriesPiece> pieces; };

// the parameter block a kernel reads a piece with: rows are indexed by step - series_t0
StepParams piece_params(const psmf_filter* h, const SeriesPiece& pc) {
  StepParams sp = h->sp;
  if (h->ring_slots) ring_point(h, sp, pc.c);
  return sp;
}

// resident: do rows up to `end` lie outside the buffers?  (a ring has no end: residency is checked piece by piece)
bool beyond_cap(const psmf_filter* h, int64_t end) { return !h->ring_slots && end > h->T_cap; }

// the steps [t0, t0 + nt) cut at the chunk boundaries; every piece must be resident (PSMF_ERR_STATE names the first step that is not)
int ring_pieces(psmf_filter* h, const char* who, int64_t t0, int64_t nt, bool need_mask, std::vector<SeriesPiece>& out) {
  out.clear();
  for (int64_t t = t0; t < t0 + nt;) {
    const int64_t c = t / h->ring_chunk, end = (c + 1) * h->ring_chunk < t0 + nt ? (c + 1) * h->ring_chunk : t0 + nt;
    const int64_t slot = c % h->ring_slots;
    for (int pass = 0; pass < (need_mask ? 2 : 1); ++pass) {
      const psmf_filter::RingSlot& s = h->ring[(size_t)slot];
      const int64_t have = s.chunk == c ? (pass ? s.mrows : s.rows) : 0;
      if (have < end - c * h->ring_chunk) {
        const int64_t miss = s.chunk == c && c * h->ring_chunk + have > t ? c * h->ring_chunk + have : t;
        const bool evicted = s.chunk > c;
        return fail(h, PSMF_ERR_STATE, std::string(who) + ": step " + std::to_string(miss + 1) + (evicted ? " is no longer resident" : " is not resident") +
                                       (pass ? " (observation mask)" : "") + " in the series ring");
      }
    }
    const size_t row = (size_t)(t - ring_t0(h, c));
    out.push_back({t, end - t, row, row + (size_t)slot, c, (int)slot});
    t = end;
  }
  return PSMF_OK;
}

// What a read of the series buffers waits for, and the stream it then sits on.  Resident: psmf_sync, the compute stream.  Ring: the
// copy stream behind the runs that touched the marked slots and behind nothing else (live_c: behind the whole compute stream too).
int series_wait(psmf_filter* h, const std::vector<char>& slots, bool live_c, hipStream_t& stream) {
  stream = h->ring_slots ? h->cstream : h->stream;
  if (!h->ring_slots || live_c) { const int rc = psmf_sync(h); if (rc) return rc; }
  for (size_t i = 0; i < h->ring.size(); ++i)
    if (slots[i] && h->ring[i].run_set) HIP_TRY(h, hipStreamWaitEvent(h->cstream, h->ring[i].run, 0));
  return PSMF_OK;
}

struct RangeError { int code; const char* msg; };      // what a resident handle answers to a range beyond its buffers
constexpr unsigned kSpanMask = 1, kSpanLiveC = 2;      // the mask rows must be resident too; the read needs the C behind every queued run

int series_span(psmf_filter* h, const char* who, int64_t t0, int64_t nt, unsigned flags, RangeError range, SeriesSpan& out) {
  int rc = set_device(h);
  if (rc) return rc;
  out.pieces.clear();
  if (beyond_cap(h, t0 + nt)) return fail(h, range.code, range.msg);
  if (h->ring_slots) rc = ring_pieces(h, who, t0, nt, (flags & kSpanMask) != 0, out.pieces);
  else out.pieces.push_back({t0, nt, (size_t)t0, (size_t)t0, 0, 0});
  if (rc) return rc;
  std::vector<char> slots(h->ring.size(), 0);
  for (const SeriesPiece& pc : out.pieces) if (h->ring_slots) slots[(size_t)pc.slot] = 1;
  return series_wait(h, slots, (flags & kSpanLiveC) != 0, out.stream);
}

// The history row of mean k (the state after step k), or -1 where it is not resident.  Ring: row k is kept with the chunk of step
// k; the mean a chunk starts from is also the first row of the chunk's own slot, and is read from there where the predecessor has
// left the ring.  *slot: the ring slot whose runs write the row.
int64_t mu_hist_row(const psmf_filter* h, int64_t k, int* slot) {
  *slot = 0;
  if (!h->ring_slots) return k;
  int64_t c = (k > 0 ? k - 1 : 0) / h->ring_chunk;
  if (!ring_has(h, c, k > 0 ? k - 1 - c * h->ring_chunk : 0)) {
    c = k / h->ring_chunk;
    if (k != c * h->ring_chunk || !ring_has(h, c, 0)) return -1;
  }
  *slot = (int)(c % h->ring_slots);
  return k - ring_t0(h, c) + *slot;      // (chunk + 1 rows per slot: ring_point)
}

// ---- copies --------------------------------------------------------------------------------------------------------------------
// n elements src -> dst with a change of element type on the copy stream (head: psmf_cast_rows)
template <typename TS, typename TD>
void launch_cast(psmf_filter* h, const TS* src, TD* dst, size_t n, int head) {
  size_t grid = (n / 4 + psmf::CAST_NT - 1) / psmf::CAST_NT;
  if (grid < 1) grid = 1;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((psmf::psmf_cast_rows<TS, TD>), dim3((unsigned)grid), dim3(psmf::CAST_NT), 0, h->cstream, src, dst, n, head);
}

// ring: through the one-chunk device staging buffer, converted by psmf_cast_rows on the copy stream
int cast_on_device(psmf_filter* h, void* host, void* dev, size_t n, bool upload) {
  const size_t es = h->elem(), hs = 12 - es;
  // one chunk of float64, and room to shift it to the rows' alignment: only streams of the other type pay for it
  ALLOC_TRY(h, h->ring_stage.reserve((size_t)h->ring_chunk * h->cfg.d_local * 8 + 16));
  const int head = psmf::cast_head(dev, es);
  char* stage = h->ring_stage.as<char>() + (size_t)psmf::cast_shift(head, hs) * hs;
  if (upload) {
    HIP_TRY(h, hipMemcpyAsync(stage, host, n * hs, hipMemcpyHostToDevice, h->cstream));
    if (es == 4) launch_cast(h, (const double*)stage, (float*)dev, n, head);
    else launch_cast(h, (const float*)stage, (double*)dev, n, head);
    HIP_TRY(h, hipGetLastError());
  } else {
    if (es == 4) launch_cast(h, (const float*)dev, (double*)stage, n, head);
    else launch_cast(h, (const double*)dev, (float*)stage, n, head);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(host, stage, n * hs, hipMemcpyDeviceToHost, h->cstream));
  }
  return PSMF_OK;
}

// resident: converted on the host, in blocks (TH: the caller's element type, TD: the storage type)
template <typename TH, typename TD>
int cast_on_host(psmf_filter* h, hipStream_t s, TH* host, TD* dev, size_t n, bool upload) {
  const size_t blk = (size_t)1 << 24;
  std::vector<TD> buf(n < blk ? n : blk);
  for (size_t a = 0; a < n; a += blk) {
    const size_t m = n - a < blk ? n - a : blk;
    if (upload) for (size_t i = 0; i < m; ++i) buf[i] = (TD)host[a + i];
    HIP_TRY(h, upload ? hipMemcpyAsync(dev + a, buf.data(), m * sizeof(TD), hipMemcpyHostToDevice, s)
                      : hipMemcpyAsync(buf.data(), dev + a, m * sizeof(TD), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, spin_stream(s));        // the block buffer serves the next block
    if (!upload) for (size_t i = 0; i < m; ++i) host[a + i] = (TH)buf[i];
  }
  return PSMF_OK;
}

// n elements of the caller (host, element type dtype) -> dev (storage type), or back, on the stream of a span; the caller spins
// on it.  Where the types differ a resident handle converts on the host and a ring on the device (its copies overlap the runs).
int copy_rows(psmf_filter* h, hipStream_t s, void* host, int dtype, void* dev, size_t n, bool upload) {
  const size_t es = h->elem(), hs = dtype == PSMF_F64 ? 8 : 4;
  if (n == 0) return PSMF_OK;
  if (hs == es) {
    if (upload) HIP_TRY(h, hipMemcpyAsync(dev, host, n * es, hipMemcpyHostToDevice, s));
    else HIP_TRY(h, hipMemcpyAsync(host, dev, n * es, hipMemcpyDeviceToHost, s));
    return PSMF_OK;
  }
  if (h->ring_slots) return cast_on_device(h, host, dev, n, upload);
  return es == 4 ? cast_on_host(h, s, (double*)host, (float*)dev, n, upload) : cast_on_host(h, s, (float*)host, (double*)dev, n, upload);
}

// ---- allocation ----------------------------------------------------------------------------------------------------------------
void series_free(psmf_filter* h) {
  h->Y.reset(); h->YP.reset(); h->mask.reset(); h->sc_hist.reset(); h->mu_hist.reset();
  h->sp.Y = h->sp.YP = nullptr; h->sp.mask = nullptr; h->sp.sc_hist = nullptr; h->sp.mu_hist = nullptr;
  h->have_mask = false;
  h->mask_hi = 0;
}

// Y, YP, the mask, sc_hist and mu_hist for `rows` series rows, and the StepParams fields that point at them.  What a step touches
// one row ahead of the series row it reads gets more: the histories (written: the mean of step k in row k, the (s, eta) of the next
// step) hist_extra rows, the mask (read: the Gram of the next step) mask_extra rows.  (s, eta) start at zero.  The one function that
// sets these fields; on an error the caller clears them again (series_free).
int series_alloc(psmf_filter* h, size_t rows, size_t hist_extra, size_t mask_extra) {
  const size_t dl = h->cfg.d_local, es = h->elem(), r = h->cfg.r;
  if (h->cfg.masked) {
    ALLOC_TRY(h, h->mask.alloc((rows + mask_extra) * dl));
    ALLOC_TRY(h, h->sc_hist.alloc((rows + hist_extra) * 2 * sizeof(double)));
    HIP_TRY(h, hipMemsetAsync(h->sc_hist, 0, (rows + hist_extra) * 2 * sizeof(double), h->stream));
    h->sp.mask = h->mask;
    h->sp.mg = h->mg;
    h->sp.mg_tr = h->mg + (r * r + 1) + 1;
    h->sp.mg_ntr = (int)((r * r + 1 + 63) / 64);
    h->sp.sc_hist = h->sc_hist;
    h->sp.mask_rows = (int)(rows + mask_extra);
  }
  ALLOC_TRY(h, h->Y.alloc(rows * dl * es));
  if (h->cfg.store_y_pred) ALLOC_TRY(h, h->YP.alloc(rows * dl * es));
  ALLOC_TRY(h, h->mu_hist.alloc((rows + hist_extra) * r * sizeof(double)));
  h->sp.mu_hist = h->mu_hist;
  h->sp.Y = h->Y;
  h->sp.YP = h->YP;
  h->sp.store_yp = h->cfg.store_y_pred ? 1 : 0;
  h->sp.series_t0 = 0;
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // the zero-fill
  return PSMF_OK;
}

// resident: the buffers are sized by T_total, on the first upload or when a series that starts over is longer
int resident_reserve(psmf_filter* h, int64_t t0, int64_t nt, int64_t T_total) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (T_total < t0 + nt) T_total = t0 + nt;
  if (h->Y && T_total <= h->T_cap) return PSMF_OK;
  if (h->Y && t0 != 0) return fail(h, PSMF_ERR_STATE, "psmf_upload_series: buffer would grow mid-series; pass T_total on the first block");
  destroy_graph(h);   // graph nodes hold the old buffer addresses
  series_free(h);
  const int rc = series_alloc(h, (size_t)T_total, 1, 0);
  if (rc) return rc;
  h->T_cap = T_total;
  return PSMF_OK;
}

// the buffers, the copy stream and the events of a ring; on an error the caller releases what exists (psmf_series_ring)
int ring_alloc(psmf_filter* h, int64_t chunk, int n_slots) {
  const size_t dl = h->cfg.d_local, rows = (size_t)n_slots * chunk;
  // the mask gets one row behind the last slot, a copy of slot 0's first; the histories chunk + 1 rows per slot (ring_point)
  int rc = series_alloc(h, rows, (size_t)n_slots, 1);
  if (rc) return rc;
  if (h->mask) HIP_TRY(h, hipMemsetAsync(h->mask, 0, (rows + 1) * dl, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->Y, 0, rows * dl * h->elem(), h->stream));
  HIP_TRY(h, hipStreamCreateWithFlags(h->cstream.put(), hipStreamNonBlocking));
  h->ring = std::vector<psmf_filter::RingSlot>((size_t)n_slots);
  for (auto& s : h->ring) {
    HIP_TRY(h, hipEventCreateWithFlags(s.up.put(), hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(s.run.put(), hipEventDisableTiming));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));      // the zero-fills
  return PSMF_OK;
}

// ---- uploads -------------------------------------------------------------------------------------------------------------------
// Where the rows [t0, t0 + nt) of an upload go, and the stream that takes them.  Resident: any range within the buffers, on the
// compute stream once it is idle.  Ring: rows of ONE chunk, in order, into its slot on the copy stream, behind the last run that
// touched the slot's previous occupant -- the compute stream is not synchronised; nt = 0 gives no piece.
int upload_span(psmf_filter* h, const char* who, bool mask, int64_t t0, int64_t nt, SeriesSpan& out) {
  out.pieces.clear();
  if (!h->ring_slots) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    out.stream = h->stream;
    out.pieces.push_back({t0, nt, (size_t)t0, (size_t)t0, 0, 0});
    return PSMF_OK;
  }
  out.stream = h->cstream;
  if (nt == 0) return PSMF_OK;
  const int64_t c = t0 / h->ring_chunk, off = t0 - c * h->ring_chunk;
  if ((t0 + nt - 1) / h->ring_chunk != c)
    return fail(h, PSMF_ERR_ARG, std::string(who) + ": the rows cross a chunk boundary of the series ring (one chunk of " + std::to_string(h->ring_chunk) + " rows per call)");
  const int slot = (int)(c % h->ring_slots);
  const psmf_filter::RingSlot& s = h->ring[(size_t)slot];
  if (mask && (s.chunk != c || s.rows < off + nt)) return fail(h, PSMF_ERR_STATE, std::string(who) + ": upload the series rows of the chunk first");
  const int64_t have = s.chunk == c ? (mask ? s.mrows : s.rows) : 0;
  if (off > have) return fail(h, PSMF_ERR_ARG, std::string(who) + ": the rows of a chunk are uploaded in order (rows " + std::to_string(have) + " .. " + std::to_string(off) + " of the chunk are missing)");
  if (s.run_set) HIP_TRY(h, hipStreamWaitEvent(h->cstream, s.run, 0));      // the previous occupant's last reader / writer
  const size_t row = (size_t)slot * h->ring_chunk + off;
  out.pieces.push_back({t0, nt, row, row + (size_t)slot, c, slot});
  return PSMF_OK;
}

// ring: the slot now holds these rows of its chunk; runs wait for the upload event
int ring_uploaded(psmf_filter* h, const SeriesPiece& pc, bool mask) {
  psmf_filter::RingSlot& s = h->ring[(size_t)pc.slot];
  const int64_t end = pc.t0 + pc.nt - pc.c * h->ring_chunk;
  HIP_TRY(h, hipEventRecord(s.up, h->cstream));
  s.up_set = true;
  if (s.chunk != pc.c) { s.chunk = pc.c; s.rows = 0; s.mrows = 0; }
  if (mask) { if (end > s.mrows) s.mrows = end; }
  else if (end > s.rows) s.rows = end;
  return PSMF_OK;
}

// psmf_upload_series / psmf_upload_mask (mask: src is uint8, dtype plays no part).  Returns when the caller's array has been read.
int series_upload(psmf_filter* h, const char* who, const void* src, int dtype, bool mask, int64_t t0, int64_t nt) {
  SeriesSpan sp;
  int rc = upload_span(h, who, mask, t0, nt, sp);
  if (rc || sp.pieces.empty()) return rc;
  const SeriesPiece& pc = sp.pieces[0];
  const size_t dl = h->cfg.d_local, es = h->elem(), n = (size_t)nt * dl;
  char* dst = h->Y.as<char>() + pc.row * dl * es;
  if (mask) {
    HIP_TRY(h, hipMemcpyAsync(h->mask + pc.row * dl, src, n, hipMemcpyHostToDevice, sp.stream));
    // ring: the masked Gram is formed one step ahead: the last step of the last slot reads the row behind it, which is this one
    if (pc.row == 0 && nt > 0 && (int64_t)h->sp.mask_rows > h->T_cap)
      HIP_TRY(h, hipMemcpyAsync(h->mask + (size_t)h->T_cap * dl, src, dl, hipMemcpyHostToDevice, sp.stream));
  } else {
    rc = copy_rows(h, sp.stream, const_cast<void*>(src), dtype, dst, n, true);
    if (rc) return rc;
  }
  HIP_TRY(h, spin_stream(sp.stream));
  if (h->ring_slots) { rc = ring_uploaded(h, pc, mask); if (rc) return rc; }
  if (!mask && h->rotU && n) {           // non-diagonal R: the handle keeps the rows y^T U (resident only: a ring refuses the rotation)
    rc = ensure_rot_tmp(h, n * es);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->rot_tmp, dst, n * es, hipMemcpyDeviceToDevice, h->stream));
    rc = rot_rows(h, h->rot_tmp, dst, nt, true);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (mask) h->have_mask = true;
  if (mask && !h->ring_slots) {
    if (t0 <= h->mask_hi && t0 + nt > h->mask_hi) h->mask_hi = t0 + nt;      // (rows behind a gap do not count)
    // the masked Gram is formed one step ahead: the run that ended at k_done has formed the Gram of step k_done + 1 from mask row
    // k_done.  When that row arrives (or changes) now, the next run must prepare again and form it from what was uploaded.
    if (nt > 0 && t0 <= h->k_done && h->k_done < t0 + nt) h->need_prep = true;
  }
  return PSMF_OK;
}

// the sums of psmf_masked_metrics over the steps t0+1 .. t0+nt, read at t - sp.series_t0, on `stream`; waits for it
int masked_metrics_rows(psmf_filter* h, const StepParams& sp, hipStream_t stream, const uint8_t* Mmiss, int64_t t0, int64_t nt, double sig, double* out4) {
  const size_t dl = h->cfg.d_local, nb = (size_t)nt * dl;
  ALLOC_TRY(h, h->mmiss.reserve(nb));
  HIP_TRY(h, hipMemcpy(h->mmiss, Mmiss, nb, hipMemcpyHostToDevice));
  const int gx = (int)((dl + psmf::WG - 1) / psmf::WG);
  int gy = (int)((2048 + gx - 1) / gx);                  // ~2 k workgroups in all
  if (gy > nt) gy = (int)nt;
  if (gy < 1) gy = 1;
  const int chunk = (int)((nt + gy - 1) / gy);
  gy = (int)((nt + chunk - 1) / chunk);
  int rc = ensure_scratch(h, (size_t)gx * gy * 4 * sizeof(double));
  if (rc) return rc;
  const size_t lds = (size_t)32 * h->cfg.r * sizeof(double);
  by_storage(h, [&](auto t) {
    hipLaunchKernelGGL(psmf::psmf_masked_metrics_k<decltype(t)>, dim3(gx, gy), dim3(psmf::WG), lds, stream, sp, (const uint8_t*)h->mask,
                       (const uint8_t*)h->mmiss, (const double*)sp.sc_hist, (long long)t0, (int)nt, chunk, sig, h->cfg.robust, h->scratch);
  });
  HIP_TRY(h, hipGetLastError());
  std::vector<double> part((size_t)gx * gy * 4);
  HIP_TRY(h, hipMemcpyAsync(part.data(), h->scratch, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(h, spin_stream(stream));
  for (int q = 0; q < 4; ++q) out4[q] = 0.0;
  for (size_t b = 0; b < (size_t)gx * gy; ++b)
    for (int q = 0; q < 4; ++q) out4[q] += part[b * 4 + q];       // fixed order
  return PSMF_OK;
}

}  // namespace

// *acc += sum (yp[i] - y[i])^2, i < n (device arrays of the element type `storage`): psmf_sq_error_k on `stream` into the kSqErrorParts
// doubles at part_d, read back and added to *acc in order; waits for the stream
int sq_error_sum(psmf_filter* h, hipStream_t stream, int storage, const void* yp, const void* y, size_t n, double* part_d, double* acc) {
  if (storage == PSMF_F64) hipLaunchKernelGGL(psmf::psmf_sq_error_k<double>, dim3(kSqErrorParts), dim3(psmf::WG), 0, stream, (const double*)yp, (const double*)y, n, part_d);
  else hipLaunchKernelGGL(psmf::psmf_sq_error_k<float>, dim3(kSqErrorParts), dim3(psmf::WG), 0, stream, (const float*)yp, (const float*)y, n, part_d);
  HIP_TRY(h, hipGetLastError());
  std::vector<double> part(kSqErrorParts);
  HIP_TRY(h, hipMemcpyAsync(part.data(), part_d, kSqErrorParts * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(h, spin_stream(stream));
  for (int q = 0; q < kSqErrorParts; ++q) *acc += part[q];
  return PSMF_OK;
}

// psmf_run on a ring handle: cut at the chunk boundaries, every piece with the series_t0 of its slot.  Nothing is launched unless
// every piece is resident.  Across a boundary the run simply goes on (k_done == k_begin: no prepare()); the posterior mean is copied
// into the slot's start row as prepare() does, which is what makes the wrap from the last slot to slot 0 right.
int ring_run(psmf_filter* h, int64_t k_begin, int64_t k_end) {
  std::vector<SeriesPiece> pcs;
  int rc = ring_pieces(h, "psmf_run", k_begin, k_end - k_begin, h->cfg.masked != 0, pcs);
  if (rc) return rc;
  const int r = h->cfg.r;
  for (const SeriesPiece& pc : pcs) {
    psmf_filter::RingSlot& s = h->ring[(size_t)pc.slot];
    const int64_t t0 = ring_t0(h, pc.c), pe = pc.t0 + pc.nt;
    if (pc.c != h->ring_cur) {
      ring_point(h, h->sp, pc.c);
      h->ring_cur = pc.c;
      // The captured launches carry the parameter block: capture again.  A replay of the old graph may still be running (runs are
      // queued without a sync), and an executable graph is not destroyed under a replay: wait for it first.  Only a launched
      // handle with pieces of 256 steps and more has one, and the slot this piece reads was uploaded behind that replay anyway.
      if (h->gexec) HIP_TRY(h, spin_stream(h->stream));
      destroy_graph(h);
    }
    if (s.up_set) HIP_TRY(h, hipStreamWaitEvent(h->stream, s.up, 0));
    bool ahead = true;         // masked: is the mask row of step pe + 1, whose Gram the piece's last step forms, where the kernel reads it?
    if (h->cfg.masked) {
      const int64_t cn = pe / h->ring_chunk;
      ahead = ring_has(h, cn, pe - cn * h->ring_chunk, true);
      const psmf_filter::RingSlot& sn = h->ring[(size_t)(cn % h->ring_slots)];
      if (ahead && sn.up_set) HIP_TRY(h, hipStreamWaitEvent(h->stream, sn.up, 0));
    }
    if (h->ring_mg_stale && h->k_done == pc.t0) h->need_prep = true;      // that Gram was formed from a row not uploaded yet: start over here
    if (!h->need_prep && h->k_done == pc.t0 && pc.t0 == pc.c * h->ring_chunk && h->mu_hist)
      HIP_TRY(h, hipMemcpyAsync(h->sp.mu_hist + (size_t)(pc.t0 - t0) * r, h->st->mu, r * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    rc = run_steps(h, pc.t0, pe);
    if (rc) return rc;
    h->ring_mg_stale = !ahead;
    HIP_TRY(h, hipEventRecord(s.run, h->stream));
    s.run_set = true;
  }
  return PSMF_OK;
}

extern "C" {

int psmf_upload_series(psmf_handle h, const void* Y, int dtype, int64_t t0, int64_t nt, int64_t T_total) {
  if (!h || !Y || nt < 0 || t0 < 0) return fail(h, PSMF_ERR_ARG, "psmf_upload_series: bad argument");
  if (dtype != PSMF_F32 && dtype != PSMF_F64) return fail(h, PSMF_ERR_ARG, "psmf_upload_series: dtype");
  int rc = set_device(h);
  if (rc) return rc;
  if (!h->ring_slots) {      // (the buffers of a ring were sized by psmf_series_ring: T_total plays no part)
    rc = resident_reserve(h, t0, nt, T_total);
    if (rc) return rc;
  }
  return series_upload(h, "psmf_upload_series", Y, dtype, false, t0, nt);
}

int psmf_upload_mask(psmf_handle h, const uint8_t* M, int64_t t0, int64_t nt) {
  if (!h || !M || t0 < 0 || nt < 0) return fail(h, PSMF_ERR_ARG, "psmf_upload_mask: bad argument");
  if (!h->cfg.masked) return fail(h, PSMF_ERR_STATE, "psmf_upload_mask: the handle was created with masked = 0");
  if (!h->mask || beyond_cap(h, t0 + nt)) return fail(h, PSMF_ERR_STATE, "psmf_upload_mask: upload the series first (it sizes the mask buffer)");
  int rc = set_device(h);
  if (rc) return rc;
  return series_upload(h, "psmf_upload_mask", M, 0, true, t0, nt);
}

int psmf_series_ring(psmf_handle h, int64_t chunk, int n_slots) {
  if (!h || chunk < 1 || n_slots < 2 || chunk > (int64_t)1 << 30 || (int64_t)n_slots * chunk > (int64_t)1 << 30)
    return fail(h, PSMF_ERR_ARG, "psmf_series_ring: need chunk >= 1, n_slots >= 2 and n_slots * chunk <= 2^30 rows");
  if (h->Y) return fail(h, PSMF_ERR_STATE, "psmf_series_ring: call it before the first psmf_upload_series (the series buffers exist already)");
  if (h->cfg.dyn_kind == PSMF_DYN_HOST) return fail(h, PSMF_ERR_STATE, std::string("host-stepped dynamics (PSMF_DYN_HOST, psmf_step_host)") + kRingRefused);
  if (h->sched) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_schedules") + kRingRefused + ": the schedules are not windowed");
  if (h->qmat) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_q_matrix_schedule") + kRingRefused + ": the schedule is not windowed");
  if (h->rotU) return fail(h, PSMF_ERR_STATE, std::string("psmf_set_noise_rotation") + kRingRefused + ": the rotation of the rows would have to run on the copy stream");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  destroy_graph(h);
  rc = ring_alloc(h, chunk, n_slots);
  if (rc) {      // leave the handle as it was: without series buffers, so that the call can be made again
    series_free(h);
    h->ring.clear();      // (the slots' events)
    h->cstream.reset();
    return rc;
  }
  h->T_cap = (int64_t)n_slots * chunk;
  h->ring_chunk = chunk;
  h->ring_slots = n_slots;
  h->need_prep = true;
  return PSMF_OK;
}

int psmf_series_ring_info(psmf_handle h, int64_t* out) {
  if (!h || !out) return PSMF_ERR_ARG;
  out[0] = h->ring_chunk;
  out[1] = h->ring_slots;
  for (int i = 0; i < h->ring_slots; ++i) out[2 + i] = h->ring[(size_t)i].chunk;
  return PSMF_OK;
}

int psmf_download_y_pred(psmf_handle h, void* out, int dtype, int64_t t0, int64_t nt) {
  if (!h || !out) return PSMF_ERR_ARG;
  if (!h->YP) return fail(h, PSMF_ERR_STATE, "psmf_download_y_pred: handle was created with store_y_pred = 0");
  const RangeError range = {PSMF_ERR_ARG, "psmf_download_y_pred: range"};
  if (t0 < 0 || nt < 0) return fail(h, range.code, range.msg);
  if (dtype != PSMF_F32 && dtype != PSMF_F64) return fail(h, PSMF_ERR_ARG, "psmf_download_y_pred: dtype");
  SeriesSpan sp;
  int rc = series_span(h, "psmf_download_y_pred", t0, nt, 0, range, sp);
  if (rc) return rc;
  const size_t dl = h->cfg.d_local, es = h->elem(), hs = dtype == PSMF_F64 ? 8 : 4;
  for (const SeriesPiece& pc : sp.pieces) {
    const size_t n = (size_t)pc.nt * dl;
    char* src = h->YP.as<char>() + pc.row * dl * es;
    if (h->rotU && n) {                    // non-diagonal R: y_hat = U (U^T y_hat) (resident only: a ring refuses the rotation)
      rc = ensure_rot_tmp(h, n * es);
      if (rc) return rc;
      rc = rot_rows(h, src, h->rot_tmp, pc.nt, false);
      if (rc) return rc;
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      src = h->rot_tmp.as<char>();
    }
    rc = copy_rows(h, sp.stream, (char*)out + (size_t)(pc.t0 - t0) * dl * hs, dtype, src, n, false);
    if (rc) return rc;
    HIP_TRY(h, spin_stream(sp.stream));      // (a ring's staging buffer serves the next piece)
  }
  return PSMF_OK;
}

int psmf_download_mu(psmf_handle h, double* out, int64_t k0, int64_t nk) {
  if (!h || !out) return PSMF_ERR_ARG;
  if (!h->mu_hist) return fail(h, PSMF_ERR_STATE, "psmf_download_mu: no series uploaded yet");
  if (k0 < 0 || nk < 0 || beyond_cap(h, k0 + nk - 1)) return fail(h, PSMF_ERR_ARG, "psmf_download_mu: range");
  int rc = set_device(h);
  if (rc) return rc;
  const int r = h->cfg.r;
  std::vector<int64_t> rows((size_t)nk);
  std::vector<char> slots(h->ring.size(), 0);
  for (int64_t k = k0; k < k0 + nk; ++k) {
    int slot;
    const int64_t row = mu_hist_row(h, k, &slot);
    if (row < 0) return fail(h, PSMF_ERR_STATE, "psmf_download_mu: step " + std::to_string(k) + " is no longer resident in the series ring");
    rows[(size_t)(k - k0)] = row;
    if (h->ring_slots) slots[(size_t)slot] = 1;
  }
  hipStream_t stream;
  rc = series_wait(h, slots, false, stream);
  if (rc) return rc;
  for (int64_t a = 0; a < nk;) {        // contiguous rows in one copy
    int64_t b = a + 1;
    while (b < nk && rows[(size_t)b] == rows[(size_t)b - 1] + 1) ++b;
    HIP_TRY(h, hipMemcpyAsync(out + (size_t)a * r, h->mu_hist + (size_t)rows[(size_t)a] * r, (size_t)(b - a) * r * sizeof(double), hipMemcpyDeviceToHost, stream));
    a = b;
  }
  HIP_TRY(h, spin_stream(stream));
  return PSMF_OK;
}

int psmf_sq_error(psmf_handle h, int64_t t0, int64_t nt, double* out) {
  if (!h || !out) return PSMF_ERR_ARG;
  if (!h->YP || !h->Y) return fail(h, PSMF_ERR_STATE, "psmf_sq_error: needs store_y_pred and an uploaded series");
  const RangeError range = {PSMF_ERR_ARG, "psmf_sq_error: range"};
  if (t0 < 0 || nt < 0) return fail(h, range.code, range.msg);
  SeriesSpan sp;
  int rc = series_span(h, "psmf_sq_error", t0, nt, 0, range, sp);
  if (rc) return rc;
  rc = ensure_scratch(h, kSqErrorParts * sizeof(double));      // (only reductions the host waits for use it: none is in flight)
  if (rc) return rc;
  const size_t dl = h->cfg.d_local, es = h->elem();
  double a = 0.0;
  for (const SeriesPiece& pc : sp.pieces) {
    const size_t off = pc.row * dl * es;
    rc = sq_error_sum(h, sp.stream, h->cfg.storage, h->YP.as<char>() + off, h->Y.as<char>() + off, (size_t)pc.nt * dl, h->scratch, &a);
    if (rc) return rc;
  }
  *out = a;
  return PSMF_OK;
}

int psmf_masked_metrics(psmf_handle h, const uint8_t* Mmiss, int64_t t0, int64_t nt, double sig, double* out4) {
  if (!h || !Mmiss || !out4 || t0 < 0 || nt < 1) return fail(h, PSMF_ERR_ARG, "psmf_masked_metrics: bad argument");
  const RangeError range = {PSMF_ERR_STATE, "psmf_masked_metrics: needs a masked handle that has run over these steps"};
  if (!h->cfg.masked || !h->have_mask || !h->YP) return fail(h, range.code, range.msg);
  // The second sum reads the live C, which every queued run rewrites: unlike the downloads, this entry point waits for the
  // compute stream on a ring too -- C is the C behind every run queued before the call, as on a resident handle.
  SeriesSpan sp;
  int rc = series_span(h, "psmf_masked_metrics", t0, nt, kSpanMask | kSpanLiveC, range, sp);
  if (rc) return rc;
  for (int q = 0; q < 4; ++q) out4[q] = 0.0;
  for (const SeriesPiece& pc : sp.pieces) {      // a ring: chunk by chunk, each with its slot's series_t0
    double o4[4];
    rc = masked_metrics_rows(h, piece_params(h, pc), sp.stream, Mmiss + (size_t)(pc.t0 - t0) * h->cfg.d_local, pc.t0, pc.nt, sig, o4);
    if (rc) return rc;
    for (int q = 0; q < 4; ++q) out4[q] += o4[q];
  }
  return PSMF_OK;
}

int psmf_download_step_scalars(psmf_handle h, double* out, int64_t t0, int64_t nt) {
  if (!h || !out || t0 < 0 || nt < 0) return fail(h, PSMF_ERR_ARG, "psmf_download_step_scalars: bad argument");
  const RangeError range = {PSMF_ERR_STATE, "psmf_download_step_scalars: needs a masked handle with an uploaded series"};
  if (!h->cfg.masked || !h->sc_hist) return fail(h, range.code, range.msg);
  SeriesSpan sp;
  int rc = series_span(h, "psmf_download_step_scalars", t0, nt, 0, range, sp);
  if (rc) return rc;
  for (const SeriesPiece& pc : sp.pieces)
    HIP_TRY(h, hipMemcpyAsync(out + 2 * (size_t)(pc.t0 - t0), h->sc_hist + 2 * pc.hist_row, (size_t)pc.nt * 2 * sizeof(double), hipMemcpyDeviceToHost, sp.stream));
  HIP_TRY(h, spin_stream(sp.stream));
  return PSMF_OK;
}

}  // extern "C"
