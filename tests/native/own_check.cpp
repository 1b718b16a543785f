// Host-only check of the owning types of rpsmf_amd/csrc/psmf_own.h: the class templates instantiated with counting host allocators in
// the place of the HIP functions.  tests/test_native_ownership.py compiles this file as host code with the address and
// undefined-behaviour sanitizers and runs it; it touches no device.  Exit status 0 and "own_check OK" when every check holds.
#include "../../rpsmf_amd/csrc/psmf_own.h"

#include <cstdio>
#include <cstdlib>

static int g_live = 0;          // allocations / handles alive
static int g_allocs = 0, g_frees = 0;
static bool g_fail_next = false;
static int g_failed = 0;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "own_check.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); ++g_failed; } } while (0)

static hipError_t host_alloc(void** p, size_t n) {
  if (g_fail_next) { g_fail_next = false; *p = reinterpret_cast<void*>(0x1);  return hipErrorOutOfMemory; }      // (a failed call may leave garbage)
  *p = std::malloc(n ? n : 1);
  ++g_live; ++g_allocs;
  return hipSuccess;
}
static hipError_t host_free(void* p) { std::free(p); --g_live; ++g_frees; return hipSuccess; }
using HostBuf = Buf<host_alloc, host_free>;

// a "handle": a heap int
static hipError_t make_handle(int** out) { *out = new int(7); ++g_live; return hipSuccess; }
static hipError_t drop_handle(int* h) { delete h; --g_live; ++g_frees; return hipSuccess; }
using Handle = Owned<int*, drop_handle>;

static void check_owned() {
  Handle a;
  CHECK(!a && a.get() == nullptr);
  CHECK(make_handle(a.put()) == hipSuccess);
  CHECK(a && g_live == 1);
  int* first = a.get();
  Handle b(std::move(a));                       // move-construct: exactly one owner
  CHECK(!a && b.get() == first && g_live == 1);
  Handle c;
  c = std::move(b);                             // move-assign
  CHECK(!b && c.get() == first && g_live == 1);
  Handle d;
  CHECK(make_handle(d.put()) == hipSuccess && g_live == 2);
  d = std::move(c);                             // move-assign over an occupied object releases its handle
  CHECK(!c && d.get() == first && g_live == 1);
  const int frees = g_frees;
  CHECK(make_handle(d.put()) == hipSuccess);    // put() on an occupied object releases first
  CHECK(g_frees == frees + 1 && g_live == 1 && d);
  int* raw = d;                                 // reads as the handle
  CHECK(raw == d.get() && *raw == 7);
  d.reset();
  CHECK(!d && g_live == 0);
  d.reset();                                    // idempotent
  CHECK(g_live == 0);
  { Handle e; CHECK(make_handle(e.put()) == hipSuccess); }      // the destructor releases
  CHECK(g_live == 0);
}

static void check_buf() {
  HostBuf a;
  CHECK(!a && a.bytes() == 0 && a.as<char>() == nullptr);
  CHECK(a.alloc(100) == hipSuccess && a && a.bytes() == 100 && g_live == 1);
  a.as<char>()[99] = 1;                         // (the sanitizer watches the bounds)
  void* p = a.as<void>();
  CHECK(a.reserve(40) == hipSuccess && a.as<void>() == p && a.bytes() == 100);       // smaller: keeps the pointer
  CHECK(a.reserve(100) == hipSuccess && a.as<void>() == p);
  int allocs = g_allocs, frees = g_frees;
  CHECK(a.reserve(101) == hipSuccess && a.bytes() == 101);                           // larger: releases, then allocates
  CHECK(g_allocs == allocs + 1 && g_frees == frees + 1 && g_live == 1);
  a.as<char>()[100] = 2;
  CHECK(a.alloc(8) == hipSuccess && a.bytes() == 8 && g_live == 1);                  // alloc: exact size, releases first
  HostBuf b(std::move(a));
  CHECK(!a && a.bytes() == 0 && b && b.bytes() == 8 && g_live == 1);
  HostBuf c;
  CHECK(c.alloc(16) == hipSuccess && g_live == 2);
  c = std::move(b);
  CHECK(!b && b.bytes() == 0 && c.bytes() == 8 && g_live == 1);
  g_fail_next = true;
  CHECK(c.reserve(1000) == hipErrorOutOfMemory);                                     // a failing allocator: empty, capacity 0
  CHECK(!c && c.bytes() == 0 && c.as<void>() == nullptr && g_live == 0);
  g_fail_next = true;
  CHECK(c.alloc(4) == hipErrorOutOfMemory && !c && c.bytes() == 0);
  CHECK(c.reserve(4) == hipSuccess && c.bytes() == 4 && g_live == 1);                // and usable again
  { HostBuf d; CHECK(d.alloc(32) == hipSuccess && g_live == 2); }
  CHECK(g_live == 1);
}

int main() {
  check_owned();
  check_buf();
  CHECK(g_live == 0);                           // everything released at exit
  if (g_failed) { std::fprintf(stderr, "own_check: %d checks failed\n", g_failed); return 1; }
  std::puts("own_check OK");
  return 0;
}
