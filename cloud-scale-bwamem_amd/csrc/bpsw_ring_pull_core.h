// bpsw_ring_pull_core.h -- what a resident rescue worker pulls for one unit, and where it puts it: for the host and for the device.
//
// A rescue batch that goes through the submission ring lies in the caller's pinned staging block (sw_stage_begin: the job table, the
// mate pool, the window pool, the 32-byte job records; every part at a multiple of 16 bytes, the block's length a multiple of 16).
// A worker that reads such a block piecemeal pays a PCIe round trip per dependent access.  With the pull it reads a unit's records
// with one load and then, in ONE burst of 16-byte loads, everything its two or four jobs need: each distinct mate once, and each
// window's t_len bytes (none in coordinate mode, where the windows come from the resident 2-bit reference).  The bytes go into a
// slice of the wave's own in LDS, and the job code runs on records rewritten to point into the slice.
//
// This header is the arithmetic of that: which byte ranges a unit pulls (plan), their widening to whole 16-byte chunks, and the
// slice layout.  A range is widened DOWN to the 16-byte boundary at or below its first byte and UP to the one at or above its end;
// the bytes keep their position within a chunk, so a chunk is stored as it was loaded (head: the range's first byte sits
// `off & 15` bytes into its slot; tail: up to 15 bytes behind the last one are pulled and never read).  Because every part of the
// block starts at a multiple of 16 and the block's length is one, a widened range never leaves [base, base + total): block_ok() is
// the host's check of exactly that, and a block that fails it is copied as before.
//
//   slice:  [0, 128)   the unit's records, rewritten: q_off / t_off are offsets into the slice
//           [128, ..)  the ranges in plan order, back to back: mate of job 0, window of job 0, mate of job 1, ...  Chunk i of the
//                      unit (the slots in order) lies at 128 + 16 i -- the order in which a wave's LDS-direct loads write their
//                      lanes' 16 bytes, which is how the kernel pulls (swp_pull_unit)
//
// The slots are fixed (2 k: mate of job k, 2 k + 1: its window; absent = 0 chunks), so nothing in here indexes an array by a
// run-time value: the kernels that compile it have no scratch.  The host runs plan() over every unit of a batch before it decides to
// pull (fits), the device runs it again for the unit it took and, should the two ever disagree, reads the block in place.
//
// Compiled by hipcc for swp_resident_kernel (bpsw_swalign.hip), by the host compiler for sw_stage_run (bpsw_sw_runtime.cpp) and by
// g++ for tests/ring_pull_host/ring_pull_host.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BPSW_RP_HD __host__ __device__ __forceinline__
#else
#define BPSW_RP_HD inline
#endif

namespace bpsw {
namespace rp {

constexpr int kMaxJobs = 4;                      // a quartet; a pair uses the first two
constexpr int kSlots = 2 * kMaxJobs;
constexpr uint32_t kChunk = 16;                  // bytes per lane and load
constexpr uint32_t kRecsBytes = 32 * kMaxJobs;   // the rewritten records at the slice's start
constexpr int kRounds = 5;                       // loads a lane issues at most: a unit is at most 64 * kRounds chunks
constexpr uint32_t kMaxChunks = 64 * kRounds;

// Slice bytes per worker wave, by ring class (bpsw_ring.h).  Classes 3 and 5 hold any unit their kernel takes: two windows of the
// class's key rows (1 024 / 1 536) and two mates of 256 bases, each with its 16 bytes of head and tail.  The half-wave class holds
// four jobs in what its workgroup's 64 KB of LDS leave (static 11 008 + key rows 36 864 + 4 x 4 352 = 65 280): four windows of up
// to ~870 rows with four 150-base mates -- every 2x150 bp rescue unit; a batch with a unit that does not fit is copied as before.
constexpr uint32_t kKeyRows3 = 1024, kKeyRows5 = 1536;   // the longest window of a class (swp_resident_key_rows, bpsw_swalign.hip)
constexpr uint32_t slice_bytes_pair(uint32_t key_rows) { return kRecsBytes + 2 * (256 + kChunk) + 2 * (key_rows + kChunk); }
constexpr uint32_t kSliceHalves = 4352;
// `columns`: the class's columns per lane, 3 or 5; `halves`: the half-wave class (columns 3, four jobs per worker)
constexpr uint32_t slice_bytes(int columns, bool halves) { return halves ? kSliceHalves : slice_bytes_pair(columns <= 3 ? kKeyRows3 : kKeyRows5); }

struct Job {
  uint64_t q_off, t_off;   // offsets into the mate pool / the window pool (t_off: a coordinate when there is no window pool)
  uint32_t q_len, t_len;
};

struct Plan {
  uint64_t src[kSlots];     // first byte pulled, as an offset into the slot's pool (even slots: mates, odd: windows); a multiple of 16
  uint32_t chunks[kSlots];  // 16-byte chunks (0: nothing pulled for this slot)
  uint32_t dst[kSlots];     // where the first chunk goes in the slice; a multiple of 16
  uint32_t q_at[kMaxJobs];  // the job's mate / window in the slice (the rewritten record's offsets)
  uint32_t t_at[kMaxJobs];
  uint32_t n_chunks;        // all slots
  uint32_t bytes;           // slice bytes used, the records included
  bool fits;                // within `slice_cap` and kMaxChunks
};

BPSW_RP_HD uint64_t down16(uint64_t v) { return v & ~(uint64_t)(kChunk - 1); }
BPSW_RP_HD uint64_t up16(uint64_t v) { return (v + (kChunk - 1)) & ~(uint64_t)(kChunk - 1); }

// The staging block as the pull needs it: base address, the two pools' offsets and the block's length all multiples of 16 (so a
// widened range stays inside a pool's own 16-byte-rounded extent, and that inside the block).
BPSW_RP_HD bool block_ok(uint64_t base, uint64_t o_qpool, uint64_t q_bytes, uint64_t o_tpool, uint64_t t_bytes, uint64_t o_packed, uint64_t total) {
  if (((base | o_qpool | o_tpool | o_packed | total) & (kChunk - 1)) != 0) return false;
  return up16(o_qpool + q_bytes) <= total && up16(o_tpool + t_bytes) <= total;
}

// The ranges of the unit whose jobs are job[0 .. n) (n <= kMaxJobs), `windows`: the batch has a window pool.
// A mate that an earlier job of the unit names too (same offset, same length) is pulled once.
BPSW_RP_HD Plan plan(const Job (&job)[kMaxJobs], const int n, const bool windows, const uint32_t slice_cap) {
  Plan P;
  uint32_t at = kRecsBytes, chunks = 0;
  bool ok = true;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int k = 0; k < kMaxJobs; ++k) {
    P.src[2 * k] = P.src[2 * k + 1] = 0;
    P.chunks[2 * k] = P.chunks[2 * k + 1] = 0;
    P.dst[2 * k] = P.dst[2 * k + 1] = 0;
    P.q_at[k] = P.t_at[k] = 0;
    if (k >= n) continue;
    int dup = -1;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = kMaxJobs - 1; j >= 0; --j)
      if (j < k && job[j].q_off == job[k].q_off && job[j].q_len == job[k].q_len) dup = j;
    if (dup >= 0) {
#ifdef __HIPCC__
#pragma unroll
#endif
      for (int j = 0; j < kMaxJobs; ++j)
        if (j == dup) P.q_at[k] = P.q_at[j];
    } else if (job[k].q_len > 0) {
      const uint64_t lo = down16(job[k].q_off), hi = up16(job[k].q_off + job[k].q_len);
      if (hi - lo > (uint64_t)kMaxChunks * kChunk) { ok = false; continue; }
      P.src[2 * k] = lo; P.chunks[2 * k] = (uint32_t)((hi - lo) / kChunk); P.dst[2 * k] = at;
      P.q_at[k] = at + (uint32_t)(job[k].q_off - lo);
      at += (uint32_t)(hi - lo); chunks += P.chunks[2 * k];
    }
    if (windows && job[k].t_len > 0) {
      const uint64_t lo = down16(job[k].t_off), hi = up16(job[k].t_off + job[k].t_len);
      if (hi - lo > (uint64_t)kMaxChunks * kChunk) { ok = false; continue; }
      P.src[2 * k + 1] = lo; P.chunks[2 * k + 1] = (uint32_t)((hi - lo) / kChunk); P.dst[2 * k + 1] = at;
      P.t_at[k] = at + (uint32_t)(job[k].t_off - lo);
      at += (uint32_t)(hi - lo); chunks += P.chunks[2 * k + 1];
    }
  }
  P.n_chunks = chunks;
  P.bytes = at;
  P.fits = ok && at <= slice_cap && chunks <= kMaxChunks;
  return P;
}

// Chunk i of the unit (0 <= i < n_chunks, the slots in order): which slot, and which chunk of it.  false: no such chunk.
BPSW_RP_HD bool chunk_at(const Plan& P, const uint32_t i, bool* window, uint64_t* src, uint32_t* dst) {
  uint32_t first = 0;
  bool found = false;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int s = 0; s < kSlots; ++s) {
    const bool here = !found && i >= first && i < first + P.chunks[s];
    if (here) {
      *window = (s & 1) != 0;
      *src = P.src[s] + (uint64_t)(i - first) * kChunk;
      *dst = P.dst[s] + (i - first) * kChunk;
      found = true;
    }
    first += P.chunks[s];
  }
  return found;
}

}  // namespace rp
}  // namespace bpsw
