// alloc_probe.cpp -- stand-alone program around the product's allocation registry (photobundle_amd/csrc/pba_alloc.h) over a malloc-backed
// backend that counts its calls.  tests/test_alloc_cpu.py builds it with AddressSanitizer + UBSan and runs `alloc_probe <case>` as a
// child process: exit status 0 and "ok", or the failed check on stderr.  Every case frees what it allocated, so the leak checker at
// exit speaks for the registry.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../../photobundle_amd/csrc/pba_alloc.h"

using pba::Allocations;
using pba::MemKind;

#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

namespace {

struct Block {
  MemKind kind;
  size_t bytes;
  void* view;   // mapped: the token handed out as the block's device address
};

struct MallocBackend final : pba::MemBackend {
  std::map<void*, Block> live;
  int allocs = 0, frees = 0, views = 0;
  size_t last_bytes = 0;
  int fail_alloc_in = 0, fail_view_in = 0;   // k > 0: the k-th call from now fails with kError
  static constexpr int kError = 2;

  int alloc(MemKind kind, size_t bytes, void** out) override {
    ++allocs;
    last_bytes = bytes;
    if (fail_alloc_in && --fail_alloc_in == 0) return kError;
    void* p = malloc(bytes);
    memset(p, 0xA5, bytes);      // the sanitizer sees every byte the registry asked for
    live[p] = Block{kind, bytes, nullptr};
    *out = p;
    return 0;
  }
  void free(MemKind kind, void* p) override {
    ++frees;
    auto it = live.find(p);
    CHECK(it != live.end());          // never a block the backend does not own, never twice
    CHECK(it->second.kind == kind);   // ... and through the call of its kind
    ::free(it->second.view);
    ::free(p);
    live.erase(it);
  }
  int device_view(void* host, void** out) override {
    ++views;
    auto it = live.find(host);
    CHECK(it != live.end() && it->second.kind == MemKind::mapped && !it->second.view);
    if (fail_view_in && --fail_view_in == 0) return kError;
    it->second.view = malloc(1);
    *out = it->second.view;
    return 0;
  }
};

void first_reserve() {
  MallocBackend b;
  Allocations a(&b);
  double* d = nullptr;
  CHECK(a.reserve(&d, MemKind::device, 100) == 0);
  CHECK(d && b.allocs == 1 && b.frees == 0 && a.count() == 1);
  CHECK(b.live.at(d).bytes == 800 + 100 && b.live.at(d).kind == MemKind::device);
  char* h = nullptr;
  CHECK(a.reserve(&h, MemKind::pinned, 64) == 0);
  CHECK(h && b.live.at(h).bytes == 64 + 8 && b.live.at(h).kind == MemKind::pinned && a.count() == 2);
  a.release_all();
  CHECK(!d && !h && b.live.empty() && b.frees == 2 && a.count() == 0);
}

void zero_elements() {
  MallocBackend b;
  Allocations a(&b);
  int* p = nullptr;
  CHECK(a.reserve(&p, MemKind::device, 0) == 0);
  CHECK(p && b.live.at(p).bytes == sizeof(int));      // n == 0 counts as 1; 4 / 8 == 0 bytes of headroom
  int* q = p;
  CHECK(a.reserve(&p, MemKind::device, 1) == 0 && p == q && b.allocs == 1);
  a.release_all();
  CHECK(b.live.empty());
}

void smaller_keeps() {
  MallocBackend b;
  Allocations a(&b);
  float* p = nullptr;
  CHECK(a.reserve(&p, MemKind::device, 1000) == 0);
  float* q = p;
  CHECK(a.reserve(&p, MemKind::device, 10) == 0 && p == q);
  CHECK(a.reserve(&p, MemKind::device, 1000) == 0 && p == q);
  CHECK(a.reserve(&p, MemKind::device, 1125) == 0 && p == q);      // the headroom of the first request: 4000 + 500 bytes
  CHECK(b.allocs == 1 && b.frees == 0);
  a.release_all();
  CHECK(b.live.empty());
}

void larger_regrows() {
  MallocBackend b;
  Allocations a(&b);
  double* p = nullptr;
  CHECK(a.reserve(&p, MemKind::device, 16) == 0);
  CHECK(a.reserve(&p, MemKind::device, 1000) == 0);
  CHECK(b.allocs == 2 && b.frees == 1 && b.live.size() == 1);      // the old block freed once (the backend refuses a second free)
  CHECK(b.last_bytes == 8000 + 1000 && b.live.at(p).bytes == 9000 && a.count() == 1);
  p[1124] = 1.0;      // the last element of the headroom is the block's
  a.release(&p);
  CHECK(!p && b.frees == 2 && b.live.empty() && a.count() == 0);
  a.release(&p);      // an entry the registry does not hold: nothing happens
  CHECK(b.frees == 2);
}

void mapped_view() {
  MallocBackend b;
  Allocations a(&b);
  double *h = nullptr, *dev = nullptr;
  CHECK(a.reserve(&h, MemKind::mapped, 8, &dev) == 0);
  CHECK(h && dev && dev == b.live.at(h).view && b.views == 1);
  CHECK(a.reserve(&h, MemKind::mapped, 8, &dev) == 0 && b.views == 1 && b.allocs == 1);
  CHECK(a.reserve(&h, MemKind::mapped, 800, &dev) == 0);
  CHECK(b.allocs == 2 && b.frees == 1 && b.views == 2 && b.live.size() == 1);
  CHECK(dev && dev == b.live.at(h).view);      // the view of the NEW block (the old one's token went with it)
  a.release(&h);
  CHECK(!h && !dev && b.live.empty());
}

void failure_mid_growth() {
  MallocBackend b;
  Allocations a(&b);
  double *h = nullptr, *dev = nullptr;
  float* d = nullptr;
  CHECK(a.reserve(&d, MemKind::device, 10) == 0 && a.reserve(&h, MemKind::mapped, 10, &dev) == 0);
  b.fail_alloc_in = 1;
  CHECK(a.reserve(&d, MemKind::device, 1000) == MallocBackend::kError);
  CHECK(!d && a.count() == 1 && b.live.size() == 1 && b.frees == 1);      // the old block went, nothing stale stays behind
  CHECK(a.reserve(&d, MemKind::device, 5) == 0 && d && a.count() == 2);    // a later reserve starts afresh
  CHECK(b.live.at(d).bytes == 20 + 2);
  b.fail_view_in = 1;      // the block is allocated, its device view refused: the block goes back
  CHECK(a.reserve(&h, MemKind::mapped, 1000, &dev) == MallocBackend::kError);
  CHECK(!h && !dev && a.count() == 1 && b.live.size() == 1);
  CHECK(a.reserve(&h, MemKind::mapped, 1000, &dev) == 0 && h && dev == b.live.at(h).view && a.count() == 2);
  a.release_all();
  CHECK(b.live.empty() && b.allocs == b.frees + 1);      // (one alloc call failed before it allocated)
}

void release_all_reuse() {
  MallocBackend b;
  Allocations a(&b);
  int* p[4] = {};
  for (int round = 0; round < 3; ++round) {
    for (int k = 0; k < 4; ++k) CHECK(a.reserve(&p[k], k % 2 ? MemKind::pinned : MemKind::device, 10 * (k + 1)) == 0 && p[k]);
    CHECK(a.count() == 4 && b.live.size() == 4);
    a.release_all();
    for (int k = 0; k < 4; ++k) CHECK(!p[k]);
    CHECK(a.count() == 0 && b.live.empty() && b.allocs == 4 * (round + 1) && b.frees == b.allocs);
  }
  a.release_all();      // empty: nothing happens
  CHECK(b.frees == 12);
}

void abandon_frees_nothing() {
  MallocBackend b;
  Allocations a(&b);
  double *h = nullptr, *dev = nullptr;
  int* d = nullptr;
  CHECK(a.reserve(&d, MemKind::device, 10) == 0 && a.reserve(&h, MemKind::mapped, 10, &dev) == 0);
  void *keep_d = d, *keep_h = h;
  a.abandon();
  CHECK(b.frees == 0 && b.live.size() == 2 && a.count() == 0 && d == keep_d && h == keep_h && dev);
  a.release_all();
  a.release(&d);
  CHECK(b.frees == 0 && b.live.size() == 2);
  // the abandoned blocks are this program's to free, so that the leak checker stays meaningful for every other case
  b.free(MemKind::device, keep_d);
  b.free(MemKind::mapped, keep_h);
  CHECK(b.live.empty());
}

const struct { const char* name; void (*run)(); } kCases[] = {
    {"first_reserve", first_reserve},   {"zero_elements", zero_elements},           {"smaller_keeps", smaller_keeps},
    {"larger_regrows", larger_regrows}, {"mapped_view", mapped_view},               {"failure_mid_growth", failure_mid_growth},
    {"release_all_reuse", release_all_reuse}, {"abandon_frees_nothing", abandon_frees_nothing},
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    for (const auto& c : kCases) printf("%s\n", c.name);
    return 2;
  }
  for (const auto& c : kCases)
    if (!strcmp(argv[1], c.name)) {
      c.run();
      printf("ok %s\n", c.name);
      return 0;
    }
  fprintf(stderr, "unknown case %s\n", argv[1]);
  return 2;
}
