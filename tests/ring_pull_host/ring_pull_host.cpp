// ring_pull_host.cpp -- csrc/bpsw_ring_pull_core.h on the host, under -fsanitize=address,undefined (tests/test_ring_pull_core_host.py).
//
// For generated job tables in blocks laid out like sw_stage_begin's (and with the window pool LAST, so that a window can end on the
// block's last byte), every unit a worker can take -- each pair, and each two consecutive pairs -- is planned and then PULLED the way
// the kernel does it: chunk i of the plan, 16 bytes, from the block into a slice.  The block is a heap allocation of exactly its
// length and the slice one of exactly the class's capacity, so a load that leaves the block or a store that leaves the slice is the
// sanitizer's to report.  Checked per unit:
//   * every byte a job reads (its mate, its window) is in the slice where the rewritten record says;
//   * no range leaves its pool's 16-byte-rounded extent, nor the block;
//   * no slice byte is written twice, the records' 128 bytes are not written at all, and chunk i lands at 128 + 16 i -- the order
//     in which a wave's LDS-direct loads write (lane l of round r is chunk 64 r + l);
//   * a mate that several jobs of the unit name is pulled once;
//   * `fits` says exactly: within the slice and within 320 chunks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpsw_ring_pull_core.h"

namespace rp = bpsw::rp;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); abort(); } \
  } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }

struct Table {
  std::vector<rp::Job> job;
  uint64_t q_bytes = 0, t_bytes = 0;
  bool windows = true;
};

struct Counters { long units = 0, fit = 0, misfit = 0, shared = 0, last_byte = 0, chunks = 0; };

static uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// One unit, pulled.  `block`: the heap block, `o_q` / `o_t`: the pools' offsets, `total`: its length.
static void pull_unit(const Table& T, const int first, const int n_here, const uint8_t* block, const uint64_t o_q, const uint64_t o_t,
                      const uint64_t total, const uint32_t cap, Counters& C) {
  rp::Job job[rp::kMaxJobs] = {};
  for (int k = 0; k < n_here; ++k) job[k] = T.job[(size_t)(first + k)];
  const rp::Plan P = rp::plan(job, n_here, T.windows, cap);
  ++C.units;
  uint32_t chunks = 0, bytes = rp::kRecsBytes;
  int mate_ranges = 0;
  for (int s = 0; s < rp::kSlots; ++s) {
    chunks += P.chunks[s];
    bytes += P.chunks[s] * rp::kChunk;
    if (P.chunks[s] == 0) continue;
    CHECK(s / 2 < n_here);
    if ((s & 1) == 0) ++mate_ranges;
    CHECK((s & 1) == 0 || T.windows);
    CHECK(P.src[s] % rp::kChunk == 0 && P.dst[s] % rp::kChunk == 0);
    const uint64_t pool = (s & 1) ? o_t : o_q, pool_bytes = (s & 1) ? T.t_bytes : T.q_bytes;
    CHECK(P.src[s] + (uint64_t)P.chunks[s] * rp::kChunk <= align16(pool_bytes));   // inside the pool's rounded extent ...
    CHECK(pool + P.src[s] + (uint64_t)P.chunks[s] * rp::kChunk <= total);          // ... and so inside the block
  }
  CHECK(chunks == P.n_chunks && bytes == P.bytes);
  CHECK(P.fits == (P.bytes <= cap && P.n_chunks <= rp::kMaxChunks));
  // distinct mates of the unit
  int distinct = 0;
  for (int k = 0; k < n_here; ++k) {
    bool seen = false;
    for (int j = 0; j < k; ++j) seen |= job[j].q_off == job[k].q_off && job[j].q_len == job[k].q_len;
    distinct += !seen;
  }
  CHECK(mate_ranges == distinct);
  if (distinct < n_here) ++C.shared;
  if (!P.fits) { ++C.misfit; return; }
  ++C.fit;
  C.chunks += P.n_chunks;
  // the pull itself, into a slice of exactly `cap` bytes
  uint8_t* slice = (uint8_t*)malloc(cap);
  uint8_t* written = (uint8_t*)calloc(cap, 1);
  CHECK(slice && written);
  memset(slice, 0xee, cap);
  for (uint32_t i = 0; i < P.n_chunks; ++i) {
    bool w = false;
    uint64_t src = 0;
    uint32_t dst = 0;
    CHECK(rp::chunk_at(P, i, &w, &src, &dst));
    CHECK(dst == rp::kRecsBytes + rp::kChunk * i);
    CHECK(w == false || T.windows);
    memcpy(slice + dst, block + (w ? o_t : o_q) + src, rp::kChunk);   // (ASan: the load stays in the block, the store in the slice)
    for (uint32_t b = 0; b < rp::kChunk; ++b) { CHECK(written[dst + b] == 0); written[dst + b] = 1; }
  }
  {
    bool w; uint64_t src; uint32_t dst;
    CHECK(!rp::chunk_at(P, P.n_chunks, &w, &src, &dst));
    CHECK(!rp::chunk_at(P, rp::kMaxChunks + 7, &w, &src, &dst));
  }
  for (uint32_t b = 0; b < rp::kRecsBytes; ++b) CHECK(written[b] == 0);
  // every byte a job reads
  for (int k = 0; k < n_here; ++k) {
    CHECK(P.q_at[k] >= rp::kRecsBytes && P.q_at[k] + job[k].q_len <= P.bytes);
    CHECK(memcmp(slice + P.q_at[k], block + o_q + job[k].q_off, job[k].q_len) == 0);
    for (uint32_t b = 0; b < job[k].q_len; ++b) CHECK(written[P.q_at[k] + b] == 1);
    if (T.windows && job[k].t_len > 0) {
      CHECK(P.t_at[k] >= rp::kRecsBytes && P.t_at[k] + job[k].t_len <= P.bytes);
      CHECK(memcmp(slice + P.t_at[k], block + o_t + job[k].t_off, job[k].t_len) == 0);
      for (uint32_t b = 0; b < job[k].t_len; ++b) CHECK(written[P.t_at[k] + b] == 1);
      if (o_t + job[k].t_off + job[k].t_len == total) ++C.last_byte;
      // the jobs of a unit do not share slice bytes (two windows never, two mates only when they are the same mate)
      for (int j = 0; j < k; ++j)
        if (job[j].t_len > 0) CHECK(P.t_at[j] + job[j].t_len <= P.t_at[k] || P.t_at[k] + job[k].t_len <= P.t_at[j]);
    }
    for (int j = 0; j < k; ++j) {
      const bool same = job[j].q_off == job[k].q_off && job[j].q_len == job[k].q_len;
      if (same) CHECK(P.q_at[j] == P.q_at[k]);
      else CHECK(P.q_at[j] + job[j].q_len <= P.q_at[k] || P.q_at[k] + job[k].q_len <= P.q_at[j]);
      if (T.windows && job[k].t_len > 0) CHECK(P.q_at[j] + job[j].q_len <= P.t_at[k] || P.t_at[k] + job[k].t_len <= P.q_at[j]);
    }
  }
  free(slice);
  free(written);
}

// A table in a block: [q pool][packed records][t pool], the window pool last; every part at a multiple of 16.
static void run_table(const Table& T, const uint32_t cap_pair, const uint32_t cap_quartet, Counters& C) {
  const uint64_t o_q = 0;
  const uint64_t o_packed = (align16(o_q + T.q_bytes) + 63) & ~(uint64_t)63;
  const uint64_t o_t = align16(o_packed + 32 * T.job.size());
  const uint64_t total = align16(o_t + (T.windows ? T.t_bytes : 0));
  uint8_t* block = (uint8_t*)malloc(total ? total : 1);
  CHECK(block);
  for (uint64_t i = 0; i < total; ++i) block[i] = (uint8_t)(rnd() % 5);
  CHECK(rp::block_ok((uint64_t)(uintptr_t)block & ~(uint64_t)15, o_q, T.q_bytes, o_t, T.windows ? T.t_bytes : 0, o_packed, total));
  const int n = (int)T.job.size();
  for (int first = 0; first < n; first += 2) {
    pull_unit(T, first, n - first < 2 ? n - first : 2, block, o_q, o_t, total, cap_pair, C);
    pull_unit(T, first, n - first < 4 ? n - first : 4, block, o_q, o_t, total, cap_quartet, C);
  }
  free(block);
}

// jobs whose mates / windows are packed into the pools at the given alignment rule: 0 = 16-byte slots, 1 = back to back, 2 = random gaps
static Table make_table(const std::vector<uint32_t>& q_len, const std::vector<uint32_t>& t_len, const int packing, const bool windows,
                        const int share_every) {
  Table T;
  T.windows = windows;
  uint64_t qa = 0, ta = 0;
  for (size_t i = 0; i < q_len.size(); ++i) {
    rp::Job J;
    if (packing == 2) { qa += rnd_in(0, 31); ta += rnd_in(0, 31); }
    if (share_every > 0 && i % (size_t)share_every != 0 && q_len[i] == T.job[i - i % (size_t)share_every].q_len) {
      J.q_off = T.job[i - i % (size_t)share_every].q_off;   // the group's first mate again
    } else {
      J.q_off = qa; qa += q_len[i];
      if (packing == 0) qa = align16(qa);
    }
    J.q_len = q_len[i];
    J.t_len = t_len[i];
    if (windows) {
      J.t_off = ta; ta += t_len[i];
      if (packing == 0 && i + 1 < q_len.size()) ta = align16(ta);   // (the last window ends the pool)
    } else {
      J.t_off = 1000003ull * (i + 1);   // a coordinate
    }
    T.job.push_back(J);
  }
  T.q_bytes = qa; T.t_bytes = windows ? ta : 0;
  return T;
}

int main() {
  const uint32_t cap3 = rp::slice_bytes_pair(1024), cap5 = rp::slice_bytes_pair(1536), caph = rp::kSliceHalves;
  Counters C;
  static const uint32_t mates[] = {1, 149, 150, 151, 256};
  static const uint32_t wins[] = {0, 1, 255, 256, 257, 1023, 1024, 1535, 1536};
  // every edge mate with every edge window, in batches of 1, 2, 3, 4, 5, 15, 16, 17 jobs, the three packings, with and without windows
  for (int packing = 0; packing < 3; ++packing)
    for (int windows = 0; windows < 2; ++windows)
      for (const int n : {1, 2, 3, 4, 5, 15, 16, 17}) {
        std::vector<uint32_t> ql, tl;
        for (int i = 0; i < n; ++i) {
          ql.push_back(mates[(i + n) % 5]);
          tl.push_back(wins[(3 * i + n + packing) % 9]);
        }
        run_table(make_table(ql, tl, packing, windows != 0, 0), cap5, cap5 + cap5, C);
        // the half-wave class's unit: mates of at most 150 bases, windows of at most 1 024 rows; many of these quartets do not fit
        for (auto& v : ql) v = v > 150 ? 150 : v;
        for (auto& v : tl) v = v > 1024 ? 1024 : v;
        run_table(make_table(ql, tl, packing, windows != 0, 0), cap3, caph, C);
      }
  // one mate for the four jobs of every quartet
  for (int packing = 0; packing < 3; ++packing) {
    std::vector<uint32_t> ql(16, 150), tl;
    for (int i = 0; i < 16; ++i) tl.push_back(rnd_in(300, 800));
    run_table(make_table(ql, tl, packing, true, 4), cap3, caph, C);
    run_table(make_table(ql, tl, packing, false, 4), cap3, caph, C);
  }
  // the last window ends on the block's last byte: a pool whose length is a multiple of 16, and one whose is not (the block is rounded up)
  for (const uint32_t last : {512u, 513u, 527u, 1u}) {
    std::vector<uint32_t> ql = {150, 150, 150, 150}, tl = {500, 501, 502, last};
    Table T = make_table(ql, tl, 1, true, 0);
    const long before = C.last_byte;
    run_table(T, cap3, caph, C);
    if ((T.t_bytes & 15) == 0) CHECK(C.last_byte > before);
  }
  // random tables of typical rescue units
  for (int it = 0; it < 300; ++it) {
    const int n = (int)rnd_in(1, 40);
    std::vector<uint32_t> ql, tl;
    const bool long_mates = it % 3 == 0;
    for (int i = 0; i < n; ++i) {
      ql.push_back(long_mates ? rnd_in(1, 256) : rnd_in(1, 150));
      tl.push_back(long_mates ? rnd_in(0, 1536) : rnd_in(0, 1024));
    }
    const Table T = make_table(ql, tl, it % 3, it % 5 != 0, it % 7 == 0 ? 2 : 0);
    if (long_mates) run_table(T, cap5, cap5 + cap5, C);
    else run_table(T, cap3, caph, C);
  }
  // a descriptor the host did not write: lengths and offsets that are anything
  for (int it = 0; it < 2000; ++it) {
    rp::Job job[rp::kMaxJobs];
    for (auto& J : job) {
      J.q_off = ((uint64_t)rnd() << 32) | rnd(); J.t_off = ((uint64_t)rnd() << (rnd() % 33)) | rnd();
      J.q_len = it % 2 ? rnd() : rnd_in(0, 6000); J.t_len = it % 3 ? rnd() : rnd_in(0, 6000);
    }
    const rp::Plan P = rp::plan(job, (int)rnd_in(0, 4), it % 4 != 0, caph);
    if (P.fits) {
      CHECK(P.bytes <= caph && P.n_chunks <= rp::kMaxChunks && P.bytes == rp::kRecsBytes + rp::kChunk * P.n_chunks);
      bool w; uint64_t src; uint32_t dst;
      for (uint32_t i = 0; i < P.n_chunks; ++i) { CHECK(rp::chunk_at(P, i, &w, &src, &dst)); CHECK(dst + rp::kChunk <= caph); }
    }
  }
  // blocks the pull refuses
  CHECK(!rp::block_ok(0x1008, 0, 100, 128, 100, 256, 512));   // base
  CHECK(!rp::block_ok(0x1000, 8, 100, 128, 100, 256, 512));   // a pool's offset
  CHECK(!rp::block_ok(0x1000, 0, 100, 128, 100, 256, 500));   // the length
  CHECK(!rp::block_ok(0x1000, 0, 100, 128, 400, 256, 512));   // a pool that ends beyond the block
  CHECK(rp::block_ok(0x1000, 0, 100, 128, 100, 256, 512));
  printf("ring pull core: %ld units planned, %ld pulled (%ld chunks), %ld beyond their slice, %ld with a shared mate, %ld windows on the block's last byte\n",
         C.units, C.fit, C.chunks, C.misfit, C.shared, C.last_byte);
  fflush(stdout);
  CHECK(C.fit > 2000 && C.misfit > 20 && C.shared > 40 && C.last_byte > 10);
  return 0;
}
