// Host-only check of the scaffold of the entry points without a handle, rpsmf_amd/csrc/psmf_batch.h: the transfer helpers, the per-item
// slots and the chunk plan instantiated over memcpy, memset, counting host allocators and a made-up memory query in the place of the
// HIP functions, EntryFail, all_finite and replica_status as they are.
// tests/test_native_batch.py compiles this file as host code with the address and undefined-behaviour sanitizers and runs it; it
// touches no device.  Exit status 0 and "batch_check OK" when every check holds.
#include "../../rpsmf_amd/csrc/psmf_batch.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

thread_local std::string g_create_error;      // (the library's lives in psmf_capi.hip, the C ABI unit)

static int g_live = 0, g_failed = 0;
static size_t g_alloc_bytes = 0, g_copy_bytes = 0;     // of the last allocation / copy
static std::vector<size_t> g_copies;                   // the bytes of every copy since it was cleared
static bool g_fail_alloc = false, g_fail_copy = false;
static int g_fail_alloc_in = -1;                      // >= 0: the allocation after that many more fails

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "batch_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); ++g_failed; } } while (0)

static hipError_t host_alloc(void** p, size_t n) {
  if (g_fail_alloc || (g_fail_alloc_in >= 0 && g_fail_alloc_in-- == 0)) { g_fail_alloc = false; return hipErrorOutOfMemory; }
  *p = std::malloc(n);          // exactly n bytes: the sanitizer watches every copy against it
  ++g_live; g_alloc_bytes = n;
  return hipSuccess;
}
static hipError_t host_free(void* p) { std::free(p); --g_live; return hipSuccess; }
static hipError_t host_copy(void* dst, const void* src, size_t n, hipMemcpyKind) {
  if (g_fail_copy) { g_fail_copy = false; return hipErrorInvalidValue; }
  std::memcpy(dst, src, n);
  g_copy_bytes = n;
  g_copies.push_back(n);
  return hipSuccess;
}
static size_t g_zero_bytes = 0;                       // of the last clearing
static hipError_t host_zero(void* dst, int value, size_t n) {
  std::memset(dst, value, n);
  g_zero_bytes = n;
  return hipSuccess;
}
static size_t g_free = 0;                             // what the made-up device reports as free
static bool g_fail_query = false;
static hipError_t host_mem_info(size_t* free_b, size_t* total_b) {
  if (g_fail_query) return hipErrorInvalidDevice;
  *free_b = g_free; *total_b = 2 * g_free;
  return hipSuccess;
}
template <typename T>
struct HostDev : Buf<host_alloc, host_free> {      // what Dev<T> is to DevBuf
  T* get() const { return as<T>(); }
};

static const EntryFail fail{"batch_check"};
static bool starts_with_who() { return g_create_error.rfind("batch_check: ", 0) == 0; }

// bytes allocated and moved = count * sizeof(T), in and out
template <typename T>
static void check_sizes(size_t count) {
  std::vector<T> src(count), back(count, T(0));
  std::iota(src.begin(), src.end(), T(1));
  HostDev<T> buf;
  CHECK(alloc_n(fail, buf, count) == PSMF_OK && g_alloc_bytes == count * sizeof(T) && buf.bytes() == count * sizeof(T));
  CHECK(copy_in<host_copy>(fail, buf, src.data(), count) == PSMF_OK && g_copy_bytes == count * sizeof(T));
  g_copy_bytes = 0;
  CHECK(copy_out<host_copy>(fail, back.data(), buf, count) == PSMF_OK && g_copy_bytes == count * sizeof(T));
  CHECK(back == src);
  HostDev<T> both;
  CHECK(alloc_copy_in<host_copy>(fail, both, src.data(), count) == PSMF_OK && g_alloc_bytes == count * sizeof(T) && g_copy_bytes == count * sizeof(T));
  CHECK(std::memcmp(both.get(), src.data(), count * sizeof(T)) == 0);
  CHECK(copy_in<host_copy>(fail, buf, src.data(), count + 1) == PSMF_ERR_HIP && starts_with_who());      // larger than the buffer: refused, not made
  CHECK(copy_out<host_copy>(fail, back.data(), buf, count + 1) == PSMF_ERR_HIP);
}

// a batch of 5 through a buffer of 2 (the host loop of psmf_bocpd_run): in at an element offset, out at the same one
static void check_chunks() {
  const size_t B = 5, chunk = 2, per = 3;
  std::vector<double> X(B * per), Y(B * per, -1.0);
  std::iota(X.begin(), X.end(), 0.5);
  HostDev<double> buf;
  CHECK(alloc_n(fail, buf, chunk * per) == PSMF_OK);
  int chunks = 0;
  for (size_t s0 = 0; s0 < B; s0 += chunk, ++chunks) {
    const size_t ns = B - s0 < chunk ? B - s0 : chunk;
    CHECK(copy_in<host_copy>(fail, buf, X.data(), ns * per, s0 * per) == PSMF_OK && g_copy_bytes == ns * per * sizeof(double));
    CHECK(buf.get()[0] == X[s0 * per]);
    CHECK(copy_out<host_copy>(fail, Y.data(), buf, ns * per, s0 * per) == PSMF_OK);
  }
  CHECK(chunks == 3 && Y == X);
}

// a tuple of slots: allocated, filled and read back in the order written; count 0 and null pointers are skipped
static void check_slots() {
  std::vector<double> a = {1, 2, 3}, a_out(3, 0.0);
  std::vector<int32_t> e_out(2, -1);
  std::vector<uint8_t> m = {1, 0, 1, 1};
  HostDev<double> da, dskip;
  HostDev<int32_t> de;
  HostDev<uint8_t> dm;
  {
    const auto io = std::make_tuple(slot(da, a.data(), a_out.data(), 3), slot(dm, m.data(), nullptr, 4), slot(de, nullptr, e_out.data(), 2),
                                    slot(dskip, a.data(), a_out.data(), 0));
    CHECK(alloc_all(fail, io) == PSMF_OK && g_live == 3 && !dskip && g_alloc_bytes == 2 * sizeof(int32_t));
    CHECK(copy_in_all<host_copy>(fail, io) == PSMF_OK && g_copy_bytes == 4 && da.get()[2] == 3.0 && dm.get()[3] == 1);
    de.get()[0] = 7; de.get()[1] = 9;
    CHECK(copy_out_all<host_copy>(fail, io) == PSMF_OK && a_out == a && e_out[0] == 7 && e_out[1] == 9);
  }
  // the second allocation fails: the code comes back through EntryFail, nothing after it is allocated
  HostDev<double> d2, d3;
  g_create_error.clear();
  g_fail_alloc = true;
  CHECK(alloc_all(fail, std::make_tuple(slot(d2, a.data(), nullptr, 3), slot(d3, a.data(), nullptr, 3))) == PSMF_ERR_HIP);
  CHECK(starts_with_who() && g_create_error.find("out of memory") != std::string::npos && !d2 && !d3);
}

// the chunk plan: budget = min(free / 2, 16 GiB); shared + one item have to fit; min(B, max_items, (budget - shared) / per item); a
// switch > 0 only lowers
static int plan(size_t free_b, int B, size_t shared, size_t per_item, int max_items, int switch_value) {
  g_free = free_b;
  int chunk = -1;
  const int rc = plan_chunk<host_mem_info>(fail, B, shared, per_item, max_items, switch_value, "replica", &chunk);
  return rc == PSMF_OK ? chunk : rc;
}
static void check_plan() {
  CHECK(plan(1000, 10, 100, 150, kNoItemCap, 0) == 2);
  CHECK(plan(1000, 10, 100, 150, kNoItemCap, 1) == 1);
  CHECK(plan(1000, 10, 100, 150, kNoItemCap, 5) == 2);      // a switch never raises it
  CHECK(plan(1000, 10, 100, 150, 1, 0) == 1);
  CHECK(plan(1000, 1, 100, 150, kNoItemCap, 0) == 1);
  g_create_error.clear();
  CHECK(plan(1000, 10, 100, 401, kNoItemCap, 0) == PSMF_ERR_HIP && starts_with_who());
  CHECK(g_create_error == "batch_check: one replica needs 501 bytes of device memory, more than is free");
  CHECK(plan(1000, 10, 100, 400, kNoItemCap, 0) == 1);      // exactly the budget
  CHECK(plan((size_t)1 << 36, 100, 0, (size_t)1 << 30, kNoItemCap, 0) == 16);      // the 16 GiB cap
  g_create_error.clear();
  g_fail_query = true;
  CHECK(plan(1000, 10, 100, 150, kNoItemCap, 0) == PSMF_ERR_HIP && starts_with_who() && g_create_error.find("hipMemGetInfo") != std::string::npos);
  g_fail_query = false;
}

// per-item slots: three buffers of different element types and per-item counts, a batch of 5 through a chunk of 2.  The buffers hold
// exactly `chunk` items, so the sanitizer sees any transfer or clearing that passes their end.
static void check_items() {
  const size_t B = 5, chunk = 2, pa = 3, pe = 1, pm = 5;
  std::vector<double> a(B * pa), a_out(B * pa, -1.0);
  std::vector<int32_t> e(B * pe), e_out(B * pe, -1);
  std::vector<uint8_t> m(B * pm), m_out(B * pm, 0xff);
  std::iota(a.begin(), a.end(), 0.5);
  std::iota(e.begin(), e.end(), 100);
  std::iota(m.begin(), m.end(), uint8_t(1));
  const int live = g_live;
  {
    HostDev<double> da, dz, dskip;
    HostDev<int32_t> de, dx;
    HostDev<uint8_t> dm;
    const auto items = std::make_tuple(item_slot(da, a.data(), a_out.data(), pa), item_slot(de, e.data(), e_out.data(), pe),
                                       item_slot(dm, m.data(), m_out.data(), pm), item_slot(dz, nullptr, nullptr, pa, true),
                                       item_slot(dx, nullptr, nullptr, 0, true, 1), item_slot(dskip, a.data(), a_out.data(), 0));
    CHECK(alloc_items(fail, items, chunk) == PSMF_OK && g_live == live + 5 && !dskip);      // a count of 0: never allocated
    CHECK(da.bytes() == chunk * pa * sizeof(double) && de.bytes() == chunk * pe * sizeof(int32_t) && dm.bytes() == chunk * pm);
    CHECK(dx.bytes() == sizeof(int32_t));      // no elements an item and one extra: a buffer of one element
    int chunks = 0;
    for (size_t s0 = 0; s0 < B; s0 += chunk, ++chunks) {
      const size_t ns = B - s0 < chunk ? B - s0 : chunk;
      for (size_t i = 0; i < chunk * pa; ++i) dz.get()[i] = 7.0;
      dx.get()[0] = 7;
      const std::vector<size_t> moved = {ns * pa * sizeof(double), ns * pe * sizeof(int32_t), ns * pm * sizeof(uint8_t)};
      g_copies.clear();
      g_zero_bytes = 0;
      CHECK((fill_items<host_copy, host_zero>(fail, items, s0, ns)) == PSMF_OK);
      CHECK(g_copies == moved && g_zero_bytes == sizeof(int32_t));      // (the last slot that is cleared: one extra element)
      CHECK(da.get()[0] == a[s0 * pa] && de.get()[0] == e[s0 * pe] && dm.get()[0] == m[s0 * pm]);
      CHECK(std::memcmp(da.get(), a.data() + s0 * pa, ns * pa * sizeof(double)) == 0 && std::memcmp(de.get(), e.data() + s0 * pe, ns * pe * sizeof(int32_t)) == 0 &&
            std::memcmp(dm.get(), m.data() + s0 * pm, ns * pm) == 0);
      for (size_t i = 0; i < chunk * pa; ++i) CHECK(dz.get()[i] == (i < ns * pa ? 0.0 : 7.0));      // cleared over the chunk's items, untouched beyond
      CHECK(dx.get()[0] == 0);
      g_copies.clear();
      CHECK(read_items<host_copy>(fail, items, s0, ns) == PSMF_OK && g_copies == moved);
    }
    CHECK(chunks == 3 && a_out == a && e_out == e && m_out == m);      // the host arrays, reassembled
    g_create_error.clear();
    CHECK(read_items<host_copy>(fail, items, 0, chunk + 1) == PSMF_ERR_HIP && starts_with_who());      // more items than the chunk: refused, not made
  }
  CHECK(g_live == live);
  // the allocation in the middle of the tuple fails: the code comes back through EntryFail, nothing after it is allocated, and what
  // came before it goes with its owner
  {
    HostDev<double> d1, d2, d3;
    const auto items = std::make_tuple(item_slot(d1, a.data(), nullptr, pa), item_slot(d2, a.data(), nullptr, pa), item_slot(d3, a.data(), nullptr, pa));
    g_create_error.clear();
    g_fail_alloc_in = 1;
    CHECK(alloc_items(fail, items, chunk) == PSMF_ERR_HIP && starts_with_who() && g_create_error.find("out of memory") != std::string::npos);
    CHECK(d1 && !d2 && !d3 && g_live == live + 1 && g_fail_alloc_in < 0);
  }
  CHECK(g_live == live);
}

static void check_all_finite() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double ok[3] = {1.0, -2.5, 0.0}, nan_last[3] = {1.0, 2.0, nan}, inf_first[3] = {-inf, 1.0, 2.0};
  CHECK(all_finite(nullptr, 0) && all_finite(ok, 0));
  CHECK(all_finite(ok, 3) && !all_finite(nan_last, 3) && all_finite(nan_last, 2) && !all_finite(inf_first, 3) && !all_finite(inf_first, 1));
}

// a failing allocation or copy inside a function shaped like an entry point: the code and "who: " come back, no buffer stays alive
static int entry(bool fail_alloc, bool fail_copy) {
  std::vector<double> x(8, 1.0);
  HostDev<double> a, b;
  PSMF_TRY(alloc_n(fail, a, 8));
  g_fail_alloc = fail_alloc;
  PSMF_TRY(alloc_n(fail, b, 8));
  g_fail_copy = fail_copy;
  PSMF_TRY(copy_in<host_copy>(fail, a, x.data(), 8));
  return copy_out<host_copy>(fail, x.data(), a, 8);
}
static void check_failures() {
  const int live = g_live;
  g_create_error.clear();
  CHECK(entry(true, false) == PSMF_ERR_HIP && starts_with_who() && g_create_error.find(kAllocCall) != std::string::npos && g_live == live);
  g_create_error.clear();
  CHECK(entry(false, true) == PSMF_ERR_HIP && starts_with_who() && g_create_error.find("hipMemcpy") != std::string::npos && g_live == live);
  CHECK(entry(false, false) == PSMF_OK && g_live == live);
  CHECK(fail(nullptr, PSMF_ERR_ARG, "three") == PSMF_ERR_ARG && g_create_error == "batch_check: three");      // the form HIP_TRY calls
}

static void check_status() {
  const bool bad[4] = {false, true, false, true};
  int asked = 0;
  const auto is_bad = [&](int b) { ++asked; return bad[b]; };
  const auto message = [](int b) { return "bad replica " + std::to_string(b); };
  int32_t status[4] = {9, 9, 9, 9};
  CHECK(replica_status(fail, 4, status, is_bad, message) == PSMF_OK && asked == 4);
  CHECK(status[0] == PSMF_OK && status[1] == PSMF_ERR_NUMERIC && status[2] == PSMF_OK && status[3] == PSMF_ERR_NUMERIC);
  asked = 0;
  CHECK(replica_status(fail, 4, nullptr, is_bad, message) == PSMF_ERR_NUMERIC && asked == 2);      // stops at the first bad replica
  CHECK(g_create_error == "batch_check: bad replica 1");
  CHECK(replica_status(fail, 1, nullptr, is_bad, message) == PSMF_OK);
}

int main() {
  check_sizes<double>(7);
  check_sizes<int32_t>(7);
  check_sizes<uint8_t>(7);
  check_chunks();
  check_slots();
  check_plan();
  check_items();
  check_all_finite();
  check_failures();
  check_status();
  CHECK(g_live == 0);                           // everything released
  if (g_failed) { std::fprintf(stderr, "batch_check: %d checks failed\n", g_failed); return 1; }
  std::puts("batch_check OK");
  return 0;
}
