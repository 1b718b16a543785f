// Host-only check of the scaffold of the entry points without a handle, rpsmf_amd/csrc/psmf_batch.h: the transfer helpers instantiated
// over memcpy and counting host allocators in the place of the HIP functions, EntryFail and replica_status as they are.
// tests/test_native_batch.py compiles this file as host code with the address and undefined-behaviour sanitizers and runs it; it
// touches no device.  Exit status 0 and "batch_check OK" when every check holds.
#include "../../rpsmf_amd/csrc/psmf_batch.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

thread_local std::string g_create_error;      // (the library's lives in psmf_capi.hip)

static int g_live = 0, g_failed = 0;
static size_t g_alloc_bytes = 0, g_copy_bytes = 0;     // of the last allocation / copy
static bool g_fail_alloc = false, g_fail_copy = false;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "batch_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); ++g_failed; } } while (0)

static hipError_t host_alloc(void** p, size_t n) {
  if (g_fail_alloc) { g_fail_alloc = false; return hipErrorOutOfMemory; }
  *p = std::malloc(n);          // exactly n bytes: the sanitizer watches every copy against it
  ++g_live; g_alloc_bytes = n;
  return hipSuccess;
}
static hipError_t host_free(void* p) { std::free(p); --g_live; return hipSuccess; }
static hipError_t host_copy(void* dst, const void* src, size_t n, hipMemcpyKind) {
  if (g_fail_copy) { g_fail_copy = false; return hipErrorInvalidValue; }
  std::memcpy(dst, src, n);
  g_copy_bytes = n;
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
  check_failures();
  check_status();
  CHECK(g_live == 0);                           // everything released
  if (g_failed) { std::fprintf(stderr, "batch_check: %d checks failed\n", g_failed); return 1; }
  std::puts("batch_check OK");
  return 0;
}
