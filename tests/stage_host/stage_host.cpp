// stage_host.cpp -- the staged block (csrc/bpsw_stage.h) on the HOST, stand-alone: StageLayout, StageIn and StageOut over two stand-in
// buffer types and a hipMemcpyAsync that is a memcpy.  tests/test_stage_host.py builds it with -fsanitize=address,undefined and
// runs it.  Test infrastructure: every buffer is allocated at exactly the size asked for, so that a byte past a block's total() is
// a byte past an allocation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <vector>

namespace bpsw {
struct FakeBuffer {
  void* ptr = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {  // grow-only, as the library's
    if (bytes <= cap) return hipSuccess;
    free(ptr);
    ptr = malloc(bytes);
    cap = ptr ? bytes : 0;
    if (ptr) memset(ptr, 0xA5, bytes);
    return ptr ? hipSuccess : hipErrorOutOfMemory;
  }
  void fill() { if (ptr) memset(ptr, 0xA5, cap); }
  ~FakeBuffer() { free(ptr); }
};
struct PinnedBuffer : FakeBuffer {};
struct DeviceBuffer : FakeBuffer {};
}  // namespace bpsw

#include "bpsw_stage.h"

static int g_copies = 0;
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  if (n) memcpy(d, s, n);
  ++g_copies;
  return hipSuccess;
}

using namespace bpsw;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); }   \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((g_rng >> 33) % n);
}

struct Spec { size_t bytes, align; bool null_src; };

// the definition the kernels index by: o_0 = 0, o_k = align_k(o_{k-1} + size_{k-1}), total = align_16(o_last + size_last)
static size_t closed_form(const std::vector<Spec>& p, std::vector<size_t>* at) {
  size_t end = 0;
  at->clear();
  for (const Spec& s : p) {
    const size_t o = (end + s.align - 1) / s.align * s.align;
    at->push_back(o);
    end = o + s.bytes;
  }
  return (end + 15) / 16 * 16;
}

static uint8_t pattern(size_t part, size_t i) { return (uint8_t)(1 + (i * 7 + part * 13) % 0xA0); }  // never 0xA5

static void check_layout(const std::vector<Spec>& p) {
  std::vector<size_t> want;
  const size_t total = closed_form(p, &want);
  StageLayout lay;
  size_t prev_end = 0;
  for (size_t k = 0; k < p.size(); ++k) {
    const size_t at = lay.add(p[k].bytes, p[k].align);
    CHECK(at == want[k]);
    CHECK(at % p[k].align == 0);
    CHECK(at >= prev_end);  // no overlap with the part before (and so with none)
    prev_end = at + p[k].bytes;
    CHECK(prev_end <= total);
  }
  CHECK(lay.total() == total && total % 16 == 0 && total >= prev_end && total < prev_end + 16);
}

// stages p through (pinned, dev), which the caller has filled with 0xA5, and checks what arrived
static void check_in(const std::vector<Spec>& p, PinnedBuffer& pinned, DeviceBuffer& dev) {
  std::vector<size_t> want;
  const size_t total = closed_form(p, &want);
  std::vector<std::vector<uint8_t> > src(p.size());
  StageIn in;
  for (size_t k = 0; k < p.size(); ++k) {
    src[k].resize(p[k].bytes);
    for (size_t i = 0; i < p[k].bytes; ++i) src[k][i] = pattern(k, i);
    // (a zero-size part with a source keeps its pointer: the vector's data() of an empty vector, possibly null)
    const int id = in.add(p[k].null_src ? nullptr : src[k].data(), p[k].bytes, p[k].align);
    CHECK(id == (int)k);
  }
  CHECK(in.total() == total);
  const int copies = g_copies;
  CHECK(in.stage(pinned, dev, nullptr) == hipSuccess);
  CHECK(g_copies == copies + 1);  // one H2D copy for the block
  CHECK(pinned.cap >= total && dev.cap >= total);
  for (size_t k = 0; k < p.size(); ++k) {
    const uint8_t* d = in.dev<uint8_t>((int)k);
    CHECK(d == (const uint8_t*)dev.ptr + want[k] && in.host<uint8_t>((int)k) == (uint8_t*)pinned.ptr + want[k]);
    for (size_t i = 0; i < p[k].bytes; ++i) CHECK(d[i] == (p[k].null_src ? 0xA5 : pattern(k, i)));  // live: every byte written; skipped: none
    // the padding up to the next part is nobody's
    const size_t next = k + 1 < p.size() ? want[k + 1] : total;
    for (size_t i = want[k] + p[k].bytes; i < next; ++i) CHECK(((const uint8_t*)dev.ptr)[i] == 0xA5);
  }
}

static void check_out(const std::vector<Spec>& p) {
  std::vector<size_t> want;
  const size_t total = closed_form(p, &want);
  PinnedBuffer pinned;
  DeviceBuffer dev;
  StageOut out;
  for (size_t k = 0; k < p.size(); ++k) CHECK(out.add(p[k].bytes, p[k].align) == (int)k);
  CHECK(out.total() == total);
  CHECK(out.reserve(pinned, dev) == hipSuccess);
  for (size_t k = 0; k < p.size(); ++k) {
    uint8_t* d = out.dev<uint8_t>((int)k);
    CHECK(d == (uint8_t*)dev.ptr + want[k]);
    for (size_t i = 0; i < p[k].bytes; ++i) d[i] = pattern(k, i);
  }
  const int copies = g_copies;
  CHECK(out.fetch(nullptr) == hipSuccess);
  CHECK(g_copies == copies + 1);
  for (size_t k = 0; k < p.size(); ++k) {
    const uint8_t* h = out.host<uint8_t>((int)k);
    CHECK(h == (const uint8_t*)pinned.ptr + want[k]);
    for (size_t i = 0; i < p[k].bytes; ++i) CHECK(h[i] == pattern(k, i));
  }
}

int main() {
  std::vector<size_t> sizes = {0, 1, 3, 4, 15, 16, 17};
  for (size_t n = 1; n <= 5; ++n) { sizes.push_back(4 * n); sizes.push_back(8 * n); }
  long cases = 0;
  for (int count = 0; count <= kStageMaxParts; ++count)
    for (int rep = 0; rep < (count == 0 ? 1 : 400); ++rep) {
      std::vector<Spec> p((size_t)count), smaller;
      for (Spec& s : p) {
        s.bytes = sizes[rnd((unsigned)sizes.size())];
        s.align = rep % 4 == 0 ? 64 : rep % 4 == 1 ? 16 : (rnd(2) ? 64 : 16);
        s.null_src = rnd(5) == 0;
      }
      check_layout(p);
      check_out(p);
      PinnedBuffer pinned;
      DeviceBuffer dev;
      if (count == 0) { StageIn in; CHECK(in.total() == 0); ++cases; continue; }
      check_in(p, pinned, dev);
      // a second, smaller block over the first: fewer parts, every part at most as large, both buffers back to 0xA5 first
      const int fewer = count - (int)rnd((unsigned)count);
      for (int k = 0; k < fewer; ++k) {
        Spec s = p[(size_t)k];
        size_t b;
        do b = sizes[rnd((unsigned)sizes.size())]; while (b > s.bytes);
        s.bytes = b;
        s.null_src = rnd(5) == 0;
        smaller.push_back(s);
      }
      const void* before = dev.ptr;
      pinned.fill(); dev.fill();
      check_in(smaller, pinned, dev);
      CHECK(dev.ptr == before);  // grow-only: the smaller block went over the larger one's memory
      ++cases;
    }
  {  // sw_stage_begin's block for n = 5, q_pool_bytes = 37, t_pool_bytes = 0, worked out by hand from its formulas:
     // q_len 0; t_len a16(20) = 32; q_off a16(32 + 20) = 64; t_off a16(64 + 40) = 112; q_rev a16(112 + 40) = 160; q_pool a16(160 + 5) = 176;
     // t_pool a16(176 + 37) = 224; packed a64(224 + 0) = 256; total a16(256 + 32 * 5) = 416
    const size_t n = 5, q = 37, t = 0;
    StageLayout lay;
    CHECK(lay.add(4 * n) == 0); CHECK(lay.add(4 * n) == 32); CHECK(lay.add(8 * n) == 64); CHECK(lay.add(8 * n) == 112);
    CHECK(lay.add(n) == 160); CHECK(lay.add(q) == 176); CHECK(lay.add(t) == 224); CHECK(lay.add(32 * n, 64) == 256);
    CHECK(lay.total() == 416);
  }
  printf("stage_host OK: %ld cases\n", cases);
  return 0;
}
