// bpsw_bam_sort.hip -- a coordinate-sorted BAM and its .bai from the BAM entries' outputs: bpsw_bam_sort, bpsw_bam_sort_set_window,
// bpsw_last_bam_sort_times.  The records stay in device memory between the copy in and the copy out.
//
// The rules -- the walk's step, what is asked of a record, the key, the BAI -- are bpsw_bam_sort_core.h's; this file is who applies them:
//   the inflate        the calling thread walks the BGZF headers (inflcore::bgzf_walk), bgzf_inflate_kernel (bpsw_bgzf_in.hip) gives the
//                      stream of records; a segment's compressed offsets become offsets of that stream through the block table;
//   bam_walk_kernel    one wavefront per segment: a window of the stream in LDS, loaded 16 bytes a lane, and one lane that follows
//                      block_size through it; the window moves on when the next length field leaves it (a record may: only its length
//                      field is read).  It runs twice: counting, and -- after scan_exclusive_i64 over the segments' counts -- storing
//                      every record's offset in rec_off[n].  A broken chain is one atomicMin on a status word: the lowest segment wins;
//   bam_key_kernel     one record per lane: the fixed fields and the CIGAR a byte at a time, the checks (the lowest bad record's index
//                      and reason to a status word by atomicMin), the key, and what the index needs of the record (bamsort::Meta);
//   the sort           radix_sort_pairs (bpsw_index.hip) over (key, record index), as many 8-bit passes as the key has bits;
//   bam_len_kernel     one sorted place per lane: its record's length; scan_exclusive_i64 makes them offsets of the sorted stream;
//   bam_gather_kernel  the wavefronts take the sorted places in turn: the record to its offset, 16 bytes a lane (copy_lines: source
//                      and destination have unrelated alignment), and the place's bamsort::Entry for the calling thread;
//   the framing        bgzf_frame_kernel, or bgzf_deflate_kernel and bgzf_pack_kernel (bpsw_bam.hip), over the sorted stream.
// What comes back: the entries (16 bytes a record) with the status words and the blocks' sizes, then the framed blocks.  The calling
// thread assembles the BAI from the entries and the blocks' offsets (bamsort::build_bai).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "bpsw_internal.h"
#include "bpsw_inflate_core.h"
#include "bpsw_bam_sort_core.h"
#include "bpsw_wave.h"

using namespace bpsw;
namespace ic = bpsw::inflcore;
namespace bs = bpsw::bamsort;
typedef long long i64;
typedef unsigned long long u64;

namespace {

constexpr int kThreads = 256;
inline unsigned grid_for(i64 n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// Segment g is stream[seg[g], seg[g + 1]).  base null: count[g] = its records.  Else record k of it: rec_off[base[g] + k] = its offset
// (k below base[g + 1] - base[g], which the first run counted).  status: the lowest g << 32 | offset at which a chain broke.
// The stream's block is readable up to the 16-byte line behind its last byte.
__global__ __launch_bounds__(64) void bam_walk_kernel(const uint8_t* __restrict__ stream, const i64* __restrict__ seg, int window,
                                                      const i64* __restrict__ base, i64* __restrict__ count, i64* __restrict__ rec_off,
                                                      u64* status) {
  __shared__ __attribute__((aligned(16))) uint8_t win[bs::kWindowMax];
  const int lane = (int)threadIdx.x;
  const i64 g = blockIdx.x, end = seg[g + 1];
  const i64 first = base ? base[g] : 0, room = base ? base[g + 1] - first : 0;
  i64 at = seg[g], k = 0;
  int bad = 0;
  while (at < end && !bad) {  // (at and bad are the wavefront's: lane 0's, broadcast below)
    const i64 w0 = at & ~(i64)15;
    i64 lines = (((end + 15) & ~(i64)15) - w0) >> 4;
    if (lines > window / 16) lines = window / 16;
    for (int v = lane; v < (int)lines; v += 64)
      *reinterpret_cast<uint4*>(win + 16 * v) = *reinterpret_cast<const uint4*>(stream + w0 + 16 * (i64)v);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
      const i64 w1 = w0 + 16 * lines;
      while (at < end && (at + 4 > end || at + 4 <= w1)) {  // (the first length field of a window always lies inside it: at - w0 < 16)
        const i64 next = bs::walk_step(at, end, win + (at - w0));  // (a field cut by `end` is refused before it is read)
        if (next < 0) { bad = 1; break; }
        if (base && k < room) rec_off[first + k] = at;
        ++k;
        at = next;
      }
    }
    at = ((i64)__shfl((int)(at >> 32), 0, 64) << 32) | (u64)(uint32_t)__shfl((int)at, 0, 64);
    bad = __shfl(bad, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (lane == 0) {
    if (bad) atomicMin(status, (u64)g << 32 | (u64)at);
    if (!base) count[g] = bad ? 0 : k;
  }
}

// record i at rec_off[i]: K[i] its key, V[i] = i, meta[i]; a refused record gets key 0 and a length of 0 (it moves no byte), and
// status takes the lowest i << 8 | reason
__global__ __launch_bounds__(kThreads) void bam_key_kernel(const uint8_t* __restrict__ stream, const i64* __restrict__ rec_off, i64 n,
                                                           bs::KeyShape ks, const int32_t* __restrict__ len, u64* __restrict__ K,
                                                           i64* __restrict__ V, bs::Meta* __restrict__ meta, u64* status) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  u64 key = 0;
  bs::Meta m = {0, 0, 0, 0u};
  const int reason = bs::check_record(stream + rec_off[i], ks, len, &key, &m);
  if (reason) {
    atomicMin(status, (u64)i << 8 | (u64)reason);
    key = 0;
    m = bs::Meta{0, 0, 0, 0u};
  }
  K[i] = key;
  V[i] = i;
  meta[i] = m;
}

// place j of the sorted list: the bytes of its record (the scan behind this makes them offsets)
__global__ __launch_bounds__(kThreads) void bam_len_kernel(const i64* __restrict__ V, const bs::Meta* __restrict__ meta, i64 n,
                                                           i64* __restrict__ place) {
  const i64 j = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (j < n) place[j] = (i64)(meta[V[j]].len_unmapped & 0x7fffffffu);
}

// place j: record V[j] from stream[rec_off[V[j]] ..) to sorted[place[j] ..), and its entry
__global__ __launch_bounds__(kThreads) void bam_gather_kernel(const uint8_t* __restrict__ stream, const i64* __restrict__ rec_off,
                                                              const i64* __restrict__ V, const bs::Meta* __restrict__ meta,
                                                              const i64* __restrict__ place, i64 n, uint8_t* __restrict__ sorted,
                                                              bs::Entry* __restrict__ table) {
  const int lane = (int)threadIdx.x & 63;
  const i64 waves = (i64)gridDim.x * (kThreads / 64);
  for (i64 j = (i64)blockIdx.x * (kThreads / 64) + ((int)threadIdx.x >> 6); j < n; j += waves) {
    const i64 i = V[j], to = place[j];
    const bs::Meta m = meta[i];
    copy_lines(stream + rec_off[i], sorted + to, (int)(m.len_unmapped & 0x7fffffffu), lane);
    if (lane == 0) table[j] = bs::Entry{m.ref, m.pos, m.end, (uint32_t)to | (m.len_unmapped & 0x80000000u)};
  }
}

std::atomic<int> g_window{0};
// inflate, walk, keys, sort, gather, frame or deflate, the index table's way back with the BAI's assembly, the round trip
thread_local double t_sort[8] = {0., 0., 0., 0., 0., 0., 0., 0.};

float between(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

}  // namespace

extern "C" {

int bpsw_bam_sort(bpsw_ctx_t* c, const char* in, size_t in_bytes, const int64_t* seg_off, int64_t n_seg, int32_t n_seqs, const int32_t* len,
                  int64_t file_off, int flags, char* out, size_t cap, size_t* out_needed, char* bai, size_t bai_cap, size_t* bai_needed,
                  int64_t* n_records) {
  if (!c || (!in && in_bytes) || !out_needed || !bai_needed || !n_records || (n_seg > 0 && !seg_off))
    return fail(BPSW_ERR_ARG, "bam_sort: null argument");
  if (flags & ~BPSW_BAM_DEFLATE) return fail(BPSW_ERR_ARG, "bam_sort: unknown flag");
  if (n_seg < 0 || n_seg >= (1ll << 31) || file_off < 0 || file_off >= (1ll << 47))
    return fail(BPSW_ERR_ARG, "bam_sort: n_seg or file_off outside its range");
  *out_needed = 0; *bai_needed = 0; *n_records = 0;
  for (double& t : t_sort) t = 0.;
  if (in_bytes >= ((size_t)1 << 31)) return fail(BPSW_ERR_LIMIT, "bam_sort: an input of 2^31 bytes or more");
  const double t0 = wall_ms();

  // ---- the contigs, the blocks, the segments ----------------------------------------------------------------------------------------------
  std::vector<int32_t> lens;
  if (len) {
    if (n_seqs < 0) return fail(BPSW_ERR_ARG, "bam_sort: n_seqs below 0");
    lens.assign(len, len + n_seqs);
  } else {
    DeviceRef& r = device_ref(c->device);
    std::lock_guard<std::mutex> g(r.mu);
    lens = r.ann_len;
    if (lens.empty() && n_seqs != 0)
      return fail(BPSW_ERR_ARG, "bam_sort: no contig lengths in the arguments and no table on the context's device (bpsw_bns_load)");
  }
  i64 longest = 0;
  for (size_t k = 0; k < lens.size(); ++k) {
    if (lens[k] < 0) return fail(BPSW_ERR_ARG, "bam_sort: contig " + std::to_string(k) + " has a negative length");
    if ((i64)lens[k] > bs::kMaxContig)
      return fail(BPSW_ERR_LIMIT, "bam_sort: contig " + std::to_string(k) + " is longer than 2^29 bases: a BAI cannot bin it");
    longest = std::max(longest, (i64)lens[k]);
  }
  const int32_t n_ref = (int32_t)lens.size();
  const bs::KeyShape ks = bs::key_shape(n_ref, longest);

  thread_local ic::Walk W;
  ic::bgzf_walk((const uint8_t*)in, (i64)in_bytes, &W);
  if (W.bad_reason) return fail(BPSW_ERR_ARG, "bam_sort: block " + std::to_string(W.bad_block) + ": " + ic::inflate_reason_text(W.bad_reason));
  if (W.consumed != (i64)in_bytes)
    return fail(BPSW_ERR_ARG, "bam_sort: " + std::to_string((i64)in_bytes - W.consumed) + " bytes behind the last whole block");
  if (W.total >= (1ll << 31)) return fail(BPSW_ERR_LIMIT, "bam_sort: 2^31 inflated bytes or more");
  const i64 U = W.total;  // the stream's bytes, and the sorted stream's: every byte is some record's
  // segment g of n_seg + 1: from seg_off[g - 1] (0 for the first) to seg_off[g] (in_bytes for the last), as offsets of the stream
  const i64 n_segs = n_seg + 1;
  std::vector<i64> seg((size_t)n_segs + 1, 0);
  seg[(size_t)n_segs] = U;
  {
    size_t b = 0;
    i64 before = 0;
    for (i64 g = 0; g < n_seg; ++g) {
      const i64 o = seg_off[g];
      if (o < before || o > (i64)in_bytes)
        return fail(BPSW_ERR_ARG, "bam_sort: seg_off[" + std::to_string(g) + "] = " + std::to_string(o) + " is not ascending inside the input");
      while (b < W.blocks.size() && (i64)W.blocks[b].coff < o) ++b;
      if (b < W.blocks.size() ? (i64)W.blocks[b].coff != o : o != (i64)in_bytes)
        return fail(BPSW_ERR_ARG, "bam_sort: segment " + std::to_string(g + 1) + " begins at offset " + std::to_string(o) +
                                      ", which is not a block boundary (stream offset " +
                                      std::to_string(b ? (i64)W.blocks[b - 1].out_off : 0) + " and on)");
      seg[(size_t)g + 1] = b < W.blocks.size() ? (i64)W.blocks[b].out_off : U;
      before = o;
    }
  }
  const int P = bam_payload_bytes();
  const size_t blocks = ((size_t)U + (size_t)P - 1) / (size_t)P;
  const bool deflate = (flags & BPSW_BAM_DEFLATE) != 0;
  int window = g_window.load(std::memory_order_relaxed);
  if (window <= 0) window = bs::kWindowDefault;
  const int scan_tile = scan_tile_items();

  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  hipStream_t s = c->stream;

  // ---- the stream and its records' number ---------------------------------------------------------------------------------------------------
  // d_bgzf: [the status words | the stream, readable to the line behind its end | the segments' counts | the scan's sums]
  StageIn up;
  const int i_chunk = up.add(in, (size_t)W.consumed), i_tab = up.add(W.blocks.data(), sizeof(ic::Block) * W.blocks.size()),
            i_seg = up.add(seg.data(), 8 * seg.size()), i_len = up.add(lens.data(), 4 * lens.size());
  StageLayout A;
  const size_t a_status = A.add(64), a_stream = A.add(align16((size_t)U) + 16), a_count = A.add(8 * ((size_t)n_segs + 1)),
               a_sums = A.add(8 * (size_t)scan_tiles(n_segs, scan_tile) + 8);
  HIP_TRY(c->d_bgzf.reserve(A.total()));
  HIP_TRY(c->h_stage_out.reserve(128));
  uint8_t* DA = (uint8_t*)c->d_bgzf.ptr;
  u64* d_status = (u64*)(DA + a_status);  // [0], [1]: the inflater's; [2]: the walk's; [3]: the keys'
  const uint8_t* d_stream = DA + a_stream;
  i64* d_count = (i64*)(DA + a_count);
  HIP_TRY(up.stage(c->h_stage_in, c->d_sw_in, s));
  HIP_TRY(hipMemsetAsync(d_status, 0xff, 64, s));
  HIP_TRY(hipEventRecord(c->ev[0], s));
  HIP_TRY(launch_bgzf_inflate(s, up.dev<uint8_t>(i_chunk), up.dev<ic::Block>(i_tab), (int)W.blocks.size(), DA + a_stream, -1, d_status));
  HIP_TRY(hipEventRecord(c->ev[1], s));
  hipLaunchKernelGGL(bam_walk_kernel, dim3((unsigned)n_segs), dim3(64), 0, s, d_stream, up.dev<i64>(i_seg), window, (const i64*)nullptr, d_count,
                     (i64*)nullptr, d_status + 2);
  HIP_TRY(hipGetLastError());
  HIP_TRY(scan_exclusive_i64(s, d_count, 1, n_segs, scan_tile, (i64*)(DA + a_sums)));
  HIP_TRY(hipEventRecord(c->ev[2], s));
  HIP_TRY(hipMemcpyAsync(c->h_stage_out.ptr, d_status, 64, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync((uint8_t*)c->h_stage_out.ptr + 64, d_count + n_segs, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t_sort[0] = between(c->ev[0], c->ev[1]);
  t_sort[1] = between(c->ev[1], c->ev[2]);
  {
    const u64* st = (const u64*)c->h_stage_out.ptr;
    if (st[0] != ~0ull)
      return fail(BPSW_ERR_ARG, "bam_sort: block " + std::to_string((i64)(st[0] >> 8)) + ": " + ic::inflate_reason_text((int)(st[0] & 0xff)));
    if (st[2] != ~0ull)
      return fail(BPSW_ERR_ARG, "bam_sort: segment " + std::to_string((i64)(st[2] >> 32)) + ": the chain of block_size fields does not end on the "
                                    "segment's end (stream offset " + std::to_string((i64)(st[2] & 0xffffffffull)) + ")");
  }
  const i64 n = *(const i64*)((const uint8_t*)c->h_stage_out.ptr + 64);
  if (n < 0 || 4 * n > U) return fail(BPSW_ERR_DEVICE, "bam_sort: the walk counted more records than the stream can hold");
  *n_records = n;

  // ---- offsets, keys, the sort, the sorted stream, its blocks ----------------------------------------------------------------------------------
  // d_gl_z: [the entries | the status words | the blocks' sizes | the blocks] (what comes back), then the working set
  StageOut fr;
  const int r_table = fr.add(16 * (size_t)n), r_status = fr.add(64), r_sizes = fr.add(deflate ? 4 * blocks : 0),
            r_out = fr.add(bgzf_framed_size((size_t)U, P));
  const size_t n8 = 8 * (size_t)n;
  const i64 table_n = sort_table_items(n);
  const size_t stride = bgzf_deflate_stride(P);
  StageLayout B;
  B.add(fr.total());
  const size_t b_rec = B.add(n8), b_key0 = B.add(n8), b_key1 = B.add(n8), b_val0 = B.add(n8), b_val1 = B.add(n8), b_meta = B.add(16 * (size_t)n),
               b_place = B.add(n8 + 8), b_tab = B.add(8 * (size_t)table_n),
               b_sums = B.add(8 * (size_t)scan_tiles(std::max(table_n, n), scan_tile) + 8), b_sorted = B.add((size_t)U + 16),
               b_wide = B.add(deflate ? blocks * stride : 0, 256), b_tok = B.add(deflate ? 2 * (size_t)U : 0);
  HIP_TRY(c->d_gl_z.reserve(B.total()));
  HIP_TRY(fr.reserve(c->h_stage_out, c->d_gl_z));
  uint8_t* D = (uint8_t*)c->d_gl_z.ptr;
  i64* rec_off = (i64*)(D + b_rec);
  u64* key[2] = {(u64*)(D + b_key0), (u64*)(D + b_key1)};
  i64* val[2] = {(i64*)(D + b_val0), (i64*)(D + b_val1)};
  bs::Meta* meta = (bs::Meta*)(D + b_meta);
  i64* place = (i64*)(D + b_place);
  uint8_t* sorted = D + b_sorted;
  HIP_TRY(hipEventRecord(c->ev[0], s));
  hipLaunchKernelGGL(bam_walk_kernel, dim3((unsigned)n_segs), dim3(64), 0, s, d_stream, up.dev<i64>(i_seg), window, (const i64*)d_count, (i64*)nullptr,
                     rec_off, d_status + 2);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[1], s));
  int at = 0, passes = 0;
  if (n > 0) {
    hipLaunchKernelGGL(bam_key_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, d_stream, (const i64*)rec_off, n, ks, up.dev<int32_t>(i_len), key[0],
                       val[0], meta, d_status + 3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], s));
    hipError_t e = hipSuccess;
    at = radix_sort_pairs(s, key, val, 0, n, bs::key_bits(ks), (i64*)(D + b_tab), scan_tile, (i64*)(D + b_sums), &passes, &e);
    HIP_TRY(e);
    HIP_TRY(hipEventRecord(c->ev[3], s));
    hipLaunchKernelGGL(bam_len_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, (const i64*)val[at], (const bs::Meta*)meta, n, place);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_exclusive_i64(s, place, 1, n, scan_tile, (i64*)(D + b_sums)));
    const i64 per_block = kThreads / 64, want = (n + per_block - 1) / per_block, most = 16ll * c->num_cu;
    hipLaunchKernelGGL(bam_gather_kernel, dim3((unsigned)std::min(want, most)), dim3(kThreads), 0, s, d_stream, (const i64*)rec_off,
                       (const i64*)val[at], (const bs::Meta*)meta, (const i64*)place, n, sorted, fr.dev<bs::Entry>(r_table));
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipEventRecord(c->ev[2], s));
    HIP_TRY(hipEventRecord(c->ev[3], s));
  }
  HIP_TRY(hipEventRecord(c->ev[4], s));
  if (blocks > 0x7fffffffull) return fail(BPSW_ERR_LIMIT, "bam_sort: more than 2^31 - 1 BGZF blocks");
  if (deflate) HIP_TRY(launch_bgzf_deflate(s, sorted, U, P, blocks, (uint16_t*)(D + b_tok), D + b_wide, fr.dev<uint32_t>(r_sizes)));
  else HIP_TRY(launch_bgzf_frame(s, sorted, U, P, blocks, fr.dev<uint8_t>(r_out)));
  HIP_TRY(hipEventRecord(c->ev[5], s));
  HIP_TRY(hipMemcpyAsync(fr.dev<u64>(r_status), d_status, 64, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(fr.h, fr.d, fr.at[r_out], hipMemcpyDeviceToHost, s));  // (the entries, the status words and the sizes lie together)
  HIP_TRY(hipEventRecord(c->ev[6], s));
  HIP_TRY(hipStreamSynchronize(s));
  t_sort[1] += between(c->ev[0], c->ev[1]);
  t_sort[2] = between(c->ev[1], c->ev[2]);
  t_sort[3] = between(c->ev[2], c->ev[3]);
  t_sort[4] = between(c->ev[3], c->ev[4]);
  t_sort[5] = between(c->ev[4], c->ev[5]);
  t_sort[6] = between(c->ev[5], c->ev[6]);
  const double t1 = wall_ms();
  {
    const u64* st = fr.host<u64>(r_status);
    if (st[3] != ~0ull)
      return fail(BPSW_ERR_ARG, "bam_sort: record " + std::to_string((i64)(st[3] >> 8)) + ": " + bs::reason_text((int)(st[3] & 0xff)));
  }
  const bs::Entry* table = fr.host<bs::Entry>(r_table);
  if (n > 0 && (i64)(table[n - 1].off_unmapped & 0x7fffffffu) >= U)
    return fail(BPSW_ERR_DEVICE, "bam_sort: the last record's place is outside the sorted stream");
  std::vector<i64> coff;
  if (deflate) {
    if (!bgzf_block_offsets(fr.host<uint32_t>(r_sizes), (size_t)U, P, blocks, &coff))
      return fail(BPSW_ERR_DEVICE, "bam_sort: a block came back with a size no block has");
  } else {
    coff.resize(blocks + 1);
    for (size_t b = 0; b <= blocks; ++b) coff[b] = (i64)bgzf_framed_size(std::min(b * (size_t)P, (size_t)U), P);
  }
  const size_t total = (size_t)coff[blocks];
  thread_local std::vector<uint8_t> index;
  bs::build_bai(table, n, U, n_ref, bs::Blocks{coff.data(), (i64)P, (i64)file_off}, &index);
  t_sort[6] += wall_ms() - t1;
  *out_needed = total;
  *bai_needed = index.size();
  if ((total && !out) || total > cap || !bai || index.size() > bai_cap) {
    t_sort[7] = wall_ms() - t0;
    return fail(BPSW_ERR_CAPACITY, "bam_sort: out or bai is too small (see *out_needed, *bai_needed)");
  }
  if (total) {
    HIP_TRY(hipEventRecord(c->ev[0], s));
    if (deflate) {
      StageIn po;  // (the input has been used)
      const int p_off = po.add(coff.data(), 8 * (blocks + 1));
      HIP_TRY(po.stage(c->h_stage_in, c->d_sw_in, s));
      HIP_TRY(launch_bgzf_pack(s, D + b_wide, P, po.dev<i64>(p_off), blocks, fr.dev<uint8_t>(r_out)));
    }
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(fr.h + fr.at[r_out], fr.d + fr.at[r_out], total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    t_sort[5] += between(c->ev[0], c->ev[1]);
    memcpy(out, fr.host<char>(r_out), total);
  }
  memcpy(bai, index.data(), index.size());
  t_sort[7] = wall_ms() - t0;
  return BPSW_OK;
}

int bpsw_bam_sort_set_window(int bytes) {
  if (bytes != 0 && (bytes < bs::kWindowMin || bytes > bs::kWindowMax))
    return fail(BPSW_ERR_ARG, "bam_sort_set_window: 64 .. 16384 bytes, or 0 for the default");
  g_window.store((bytes + 15) & ~15, std::memory_order_relaxed);
  return BPSW_OK;
}

void bpsw_last_bam_sort_times(double ms[8]) {
  if (ms) memcpy(ms, t_sort, sizeof t_sort);
}

}  // extern "C"
