// bpsw_fastq.hip -- four-line FASTQ text to the library's read pools on the device: bpsw_fastq_parse, and the two entries that go from
// FASTQ text to SAM text in one call, bpsw_align_fastq_se and bpsw_align_fastq_pe, with their twins that end in BAM
// (bpsw_align_fastq_bam_se / _pe: the same two bodies, fastq_se and fastq_pe, ending in bpsw_bam.hip's align entries).
//
// The record rules are bpsw_fastq_core.h's; this file is who applies them.  With BPSW_FASTQ_HOST that is parse_serial of the same
// header on the calling thread (nothing is launched, no device is needed).  Otherwise the text goes to the device in one staged block
// and four kernels run over it, none of whose workgroups ever waits for another (the rule of bpsw_scan.hip, for its reason: what a
// workgroup needs from the others it gets from the launch before):
//   fastq_count_kernel   a wavefront per 1 KiB tile, 16 bytes a lane: the tile's number of '\n'                 -> count[tile]
//   scan_exclusive_i64   (bpsw_scan.hip) each tile's first line number; entry `tiles` is the text's number of '\n'
//   fastq_lines_kernel   the same tiles: a lane ranks its newlines behind the lanes below it (the DPP scan of bpsw_wave.h) and stores
//                        line_start[L + 1] = p + 1 for the '\n' at p that ends line L; a store past the table's room is dropped
//   fastq_record_kernel  a read per lane: fq_read on lines 4r .. 4r + 3, read_len and name_len into two 64-bit columns (one scan call
//                        sums both, as the seeding plan does), where its bases, qualities and name begin, and a bad read by one vector
//                        atomicMin on a 64-bit word (read << 8 | reason): the lowest bad read wins, as in the serial parse
//   fastq_emit_kernel    indexed by OUTPUT position: a lane owns 4 consecutive bytes of a pool and finds their read by bisection over
//                        the summed offsets (as seed_sa_kernel does over its intervals), so that loads and stores are both coalesced;
//                        one launch for bases and qualities, one for the names
// The host waits three times: for the line counts (they size the line table and say how many reads there are), for the totals and
// the bad-read word (they decide between a refusal, BPSW_ERR_CAPACITY and the emit), and for the pools.
//
// The bpsw_*_bgzf_* entries are the same bodies over BGZF chunks.  The calling thread walks the block headers (bpsw_inflate_core.h), the
// whole blocks and their tables are what is staged, bgzf_inflate_kernel (bpsw_bgzf_in.hip) writes the text into a buffer of the
// context's own, d_bgzf, and the four kernels read it there: the text never crosses PCIe.  The count kernels are launched right behind
// the inflate and its status word comes back in the first wait, together with the text's last byte (open_line needs it); an inflate
// refusal wins over every refusal of the parse.  Offsets into such a text go back to the caller as BGZF virtual offsets.
//
// The line table has room for 4 * fq_records_to_parse(lines, bytes) + 1 starts, not for 4 * max_reads + 1: `needed` is to be complete
// after one call, also when max_reads is the capacity that is short, and fq_records_to_parse bounds the room by the text's size.
#include <string.h>

#include <string>
#include <vector>

#include "bpsw_internal.h"
#include "bpsw_wave.h"
#include "bpsw_fastq_core.h"
#include "bpsw_inflate_core.h"

using namespace bpsw;
namespace fq = bpsw::fqcore;
namespace ic = bpsw::inflcore;

static_assert(fq::FINAL == BPSW_FASTQ_FINAL && fq::INTERLEAVED == BPSW_FASTQ_INTERLEAVED && fq::PAIR_NAMES == BPSW_FASTQ_PAIR_NAMES &&
              fq::HOST == BPSW_FASTQ_HOST, "the core's flags are the header's");

namespace {

constexpr int kFqThreads = 256, kFqTileBytes = 1024;  // a wavefront's tile: 64 lanes x 16 bytes

// bit k set: byte k of the 32-bit word is '\n'
__device__ __forceinline__ unsigned newline_bits4(unsigned w) {
  const unsigned x = w ^ 0x0a0a0a0au;
  const unsigned z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 in every byte of x that is zero, exactly
  return (z >> 7 & 1u) | (z >> 14 & 2u) | (z >> 21 & 4u) | (z >> 28 & 8u);
}
// the '\n' among text[p0 .. p0 + 16) as 16 bits; nothing at or past `bytes` is read.  text is 16-byte aligned and p0 a multiple of 16.
__device__ __forceinline__ unsigned newline_bits16(const char* __restrict__ text, long long bytes, long long p0) {
  if (p0 + 16 <= bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + p0);
    return newline_bits4(v.x) | newline_bits4(v.y) << 4 | newline_bits4(v.z) << 8 | newline_bits4(v.w) << 12;
  }
  unsigned m = 0;
  for (int k = 0; k < 16; ++k)
    if (p0 + k < bytes && text[p0 + k] == '\n') m |= 1u << k;
  return m;
}

__global__ __launch_bounds__(kFqThreads) void fastq_count_kernel(const char* __restrict__ text, long long bytes, long long tiles,
                                                                  long long* __restrict__ count) {
  const long long tile = (long long)blockIdx.x * (kFqThreads / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long long p0 = tile * kFqTileBytes + lane * 16;
  const int mine = tile < tiles ? __popc(newline_bits16(text, bytes, p0)) : 0;
  const int upto = wave_scan_add(mine);  // (every lane of the wavefront is here)
  if (lane == 63 && tile < tiles) count[tile] = upto;
}

// first[tile]: the number of '\n' in front of the tile (the scanned counts), first[tiles] the text's; open_line: the text's last line
// has no '\n' and counts as a line (BPSW_FASTQ_FINAL): its end is stored as if a '\n' stood at `bytes`.
__global__ __launch_bounds__(kFqThreads) void fastq_lines_kernel(const char* __restrict__ text, long long bytes, long long tiles,
                                                                  const long long* __restrict__ first, int open_line,
                                                                  fq::pos_t* __restrict__ line_start, long long room) {
  const long long tile = (long long)blockIdx.x * (kFqThreads / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long long p0 = tile * kFqTileBytes + lane * 16;
  unsigned m = tile < tiles ? newline_bits16(text, bytes, p0) : 0;
  const int mine = __popc(m);
  const int upto = wave_scan_add(mine);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_start[0] = 0;  // (room >= 1)
    const long long at = first[tiles] + 1;
    if (open_line && at < room) line_start[at] = (fq::pos_t)(bytes + 1);
  }
  if (tile >= tiles) return;
  long long at = first[tile] + (upto - mine) + 1;  // where the start of the line behind my first '\n' goes
  while (m) {
    const int k = __ffs(m) - 1;
    m &= m - 1;
    if (at < room) line_start[at] = (fq::pos_t)(p0 + k + 1);
    ++at;
  }
}

struct FqTexts {
  const char* text[2];
  const fq::pos_t* lt[2];
  long long bytes[2];
};
struct FqReads {  // per read, n of each; the two columns have n + 1 entries each and lie behind one another (column k at cols + k (n + 1))
  long long* cols;
  int32_t* read_len;
  fq::pos_t *seq_beg, *qual_beg, *name_beg;
};
// result: [0] the lowest read << 8 | reason (all ones: none), [1], [2] the offsets behind the last parsed record of text 1 and 2
__global__ __launch_bounds__(kFqThreads) void fastq_record_kernel(FqTexts T, fq::Shape S, FqReads R, unsigned long long* __restrict__ result) {
  const long long i = (long long)blockIdx.x * kFqThreads + threadIdx.x;
  if (i == 0) {
    const long long at0 = T.lt[0][4 * S.used[0]], at1 = S.two ? (long long)T.lt[1][4 * S.used[1]] : 0;
    result[1] = (unsigned long long)(at0 > T.bytes[0] ? T.bytes[0] : at0);
    result[2] = (unsigned long long)(at1 > T.bytes[1] ? T.bytes[1] : at1);
  }
  if (i >= S.n_reads) return;
  fq::Record rec;
  const int reason = fq::fq_read(S, T.text, T.lt, T.bytes, i, &rec);
  R.cols[i] = rec.seq_len;
  R.cols[S.n_reads + 1 + i] = S.pair_names && (i & 1) ? 0 : rec.name_len;
  R.read_len[i] = rec.seq_len;
  R.seq_beg[i] = rec.seq_beg; R.qual_beg[i] = rec.qual_beg; R.name_beg[i] = rec.name_beg;
  if (reason) atomicMin(result, (unsigned long long)i << 8 | (unsigned)reason);
}

// Output bytes [4 g, 4 g + 4) of a pool whose read i owns [off[i], off[i + 1]): byte p of it comes from src_a[i] + (p - off[i]) of the
// read's text -- translated to a base code when `translate` -- and, into dst_b when there is one, from src_b[i] + (p - off[i]) as it is.
__global__ __launch_bounds__(kFqThreads) void fastq_emit_kernel(FqTexts T, int two, long long n, const long long* __restrict__ off,
                                                                 const fq::pos_t* __restrict__ src_a, const fq::pos_t* __restrict__ src_b,
                                                                 uint8_t* __restrict__ dst_a, uint8_t* __restrict__ dst_b, int translate) {
  const long long p0 = 4 * ((long long)blockIdx.x * kFqThreads + threadIdx.x), total = off[n];
  if (p0 >= total) return;
  long long lo = 0, hi = n - 1;
  while (lo < hi) {  // the last read whose offset is <= p0 (reads without bytes share an offset with the next one)
    const long long mid = (lo + hi + 1) >> 1;
    if (off[mid] <= p0) lo = mid;
    else hi = mid - 1;
  }
  long long r = lo, beg = off[r], end = off[r + 1];
  unsigned a4 = 0, b4 = 0;
  const int cnt = total - p0 < 4 ? (int)(total - p0) : 4;
  for (int k = 0; k < cnt; ++k) {
    const long long p = p0 + k;
    while (p >= end && r + 1 < n) { ++r; beg = end; end = off[r + 1]; }
    const int which = two ? (int)(r & 1) : 0;
    const char* t = fq::fq_pick(T.text, which);
    const long long bytes = fq::fq_pick(T.bytes, which);
    const long long sa = (long long)src_a[r] + (p - beg);
    const unsigned char a = sa < bytes ? (unsigned char)t[sa] : 0;
    a4 |= (translate ? (unsigned)fq::fq_base_code(a) : (unsigned)a) << (8 * k);
    if (dst_b) {
      const long long sb = (long long)src_b[r] + (p - beg);
      b4 |= (unsigned)(sb < bytes ? (unsigned char)t[sb] : 0) << (8 * k);
    }
  }
  if (cnt == 4) {  // (the pools begin at multiples of 16)
    *reinterpret_cast<unsigned*>(dst_a + p0) = a4;
    if (dst_b) *reinterpret_cast<unsigned*>(dst_b + p0) = b4;
  } else {
    for (int k = 0; k < cnt; ++k) {
      dst_a[p0 + k] = (uint8_t)(a4 >> (8 * k));
      if (dst_b) dst_b[p0 + k] = (uint8_t)(b4 >> (8 * k));
    }
  }
}

thread_local double t_fq[5] = {0., 0., 0., 0., 0.};

struct Caller {  // what a parse is asked for, whoever applies the rules
  const char* who;
  const char* text[2];
  long long bytes[2];
  int n_texts, flags;
};

// The compressed side of a parse whose texts are BGZF chunks (the bpsw_*_bgzf_* entries): per text the chunk, the walk of its headers
// and how many bytes of the first block's output earlier calls consumed.  The Caller of such a parse has no host text (text[t] null);
// its bytes[t] are the inflated bytes behind skip[t].
struct Bgzf {
  const char* in[2];
  int32_t skip[2];
  ic::Walk walk[2];
};
int refuse_block(const char* who, int t, long long block, int reason) {
  return fail(BPSW_ERR_ARG, std::string(who) + ": text " + std::to_string(t + 1) + ": block " + std::to_string(block) + ": " + ic::inflate_reason_text(reason));
}
// where text t's 16-byte status line and its bytes lie in d_bgzf: the inflated stream begins (-skip) & 15 bytes behind a 16-byte line, so
// that the text, which begins `skip` bytes into it, begins on one (the count / lines / emit kernels load it 16 bytes at a time)
struct BgzfPlace { size_t status, stream, text, end; };
BgzfPlace bgzf_place(const Bgzf& Z, int t, size_t from) {
  BgzfPlace P;
  P.status = from;
  P.stream = from + 16 + (size_t)((16 - (Z.skip[t] & 15)) & 15);
  P.text = P.stream + (size_t)Z.skip[t];
  P.end = align16(P.stream + (size_t)Z.walk[t].total) + 16;
  return P;
}

// the refusal of read `bad` for `reason`: the entry, the record, the text and the reason in fixed words
int refuse(const Caller& A, const fq::Shape& S, long long bad, int reason) {
  if (reason == fq::R_TABLE) return fail(BPSW_ERR_DEVICE, std::string(A.who) + ": the line table is inconsistent");
  std::string m = std::string(A.who) + ": record " + std::to_string(fq::fq_record_of(S, bad)) + " of text " + std::to_string(fq::fq_text_of(S, bad) + 1);
  if (S.pair_names) m += " (pair " + std::to_string(bad >> 1) + ")";
  return fail(BPSW_ERR_ARG, m + ": " + fq::fq_reason_text(reason));
}

unsigned grid_of(long long items) { return (unsigned)((items + kFqThreads - 1) / kFqThreads); }

// The parse on the device.  Caller holds c->mu through a ContextEntry.  room: as parse_serial's.
// Z: the texts are BGZF chunks -- what is staged is the chunks' whole blocks and their tables, bgzf_inflate_kernel writes the text into
// d_bgzf, and the kernels below read it there; its status words come back with the line counts.
template <class Room>
int parse_device(bpsw_ctx* c, const Caller& A, Room&& room, fq::Result* res, const Bgzf* Z = nullptr) {
  const double t0 = wall_ms();
  hipStream_t s = c->stream;
  // ---- the text, and its newlines per tile --------------------------------------------------------------------------------------
  StageIn in;
  int i_text[2] = {-1, -1}, i_tab[2] = {-1, -1};
  long long tiles[2] = {0, 0};
  BgzfPlace place[2] = {};
  for (int t = 0; t < A.n_texts; ++t) {
    if (Z) {
      i_text[t] = in.add(Z->in[t], (size_t)Z->walk[t].consumed);
      i_tab[t] = in.add(Z->walk[t].blocks.data(), sizeof(ic::Block) * Z->walk[t].blocks.size());
      place[t] = bgzf_place(*Z, t, t ? place[0].end : 0);
    } else {
      i_text[t] = in.add(A.text[t], (size_t)A.bytes[t]);
    }
    tiles[t] = (A.bytes[t] + kFqTileBytes - 1) / kFqTileBytes;
  }
  const int tile_items = scan_tile_items();
  StageLayout L1;  // d_seed[3]: per text the count column (tiles + 1 entries) and the scan's tile sums
  size_t o_cnt[2] = {0, 0}, o_sums[2] = {0, 0};
  for (int t = 0; t < A.n_texts; ++t) {
    o_cnt[t] = L1.add(8 * ((size_t)tiles[t] + 1));
    o_sums[t] = L1.add(8 * (size_t)scan_tiles(tiles[t], tile_items));
  }
  HIP_TRY(c->d_seed[3].reserve(L1.total()));
  uint8_t* W1 = (uint8_t*)c->d_seed[3].ptr;
  HIP_TRY(in.stage(c->h_stage_in, c->d_sw_in, s));
  FqTexts T;
  for (int t = 0; t < 2; ++t) {
    T.text[t] = t < A.n_texts ? in.dev<char>(i_text[t]) : nullptr;
    T.lt[t] = nullptr;
    T.bytes[t] = t < A.n_texts ? A.bytes[t] : 0;
  }
  if (Z) {
    HIP_TRY(c->d_bgzf.reserve(place[A.n_texts - 1].end));
    uint8_t* D = (uint8_t*)c->d_bgzf.ptr;
    for (int t = 0; t < A.n_texts; ++t) {
      const std::vector<ic::Block>& blocks = Z->walk[t].blocks;
      int last = (int)blocks.size() - 1;  // the block that holds the text's last byte
      while (last >= 0 && !blocks[(size_t)last].isize) --last;
      HIP_TRY(hipMemsetAsync(D + place[t].status, 0xff, 16, s));
      HIP_TRY(launch_bgzf_inflate(s, in.dev<uint8_t>(i_text[t]), in.dev<ic::Block>(i_tab[t]), (int)blocks.size(), D + place[t].stream, last,
                                  (unsigned long long*)(D + place[t].status)));
      T.text[t] = (const char*)(D + place[t].text);
    }
  }
  HIP_TRY(hipEventRecord(c->ev[0], s));
  for (int t = 0; t < A.n_texts; ++t) {
    if (!tiles[t]) continue;
    hipLaunchKernelGGL(fastq_count_kernel, dim3(grid_of(tiles[t] * 64)), dim3(kFqThreads), 0, s, T.text[t], T.bytes[t], tiles[t],
                       (long long*)(W1 + o_cnt[t]));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[1], s));
  HIP_TRY(c->h_stage_out.reserve(64));
  for (int t = 0; t < A.n_texts; ++t) {
    HIP_TRY(scan_exclusive_i64(s, (long long*)(W1 + o_cnt[t]), 1, tiles[t], tile_items, (long long*)(W1 + o_sums[t])));
    HIP_TRY(hipMemcpyAsync((long long*)c->h_stage_out.ptr + t, (long long*)(W1 + o_cnt[t]) + tiles[t], 8, hipMemcpyDeviceToHost, s));
    if (Z)  // (the inflate's status comes back in the wait for the line counts: a bad block costs no wait of its own)
      HIP_TRY(hipMemcpyAsync((long long*)c->h_stage_out.ptr + 2 + 2 * t, (uint8_t*)c->d_bgzf.ptr + place[t].status, 16, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  t_fq[0] = ms;
  long long lines[2] = {0, 0};
  int open_line[2] = {0, 0};
  char last_byte[2] = {'\n', '\n'};
  for (int t = 0; t < A.n_texts; ++t) {
    if (Z) {
      const unsigned long long* st = (const unsigned long long*)c->h_stage_out.ptr + 2 + 2 * t;
      if (st[0] != ~0ull) return refuse_block(A.who, t, (long long)(st[0] >> 8), (int)(st[0] & 0xff));
      last_byte[t] = (char)(uint8_t)st[1];
    } else if (A.bytes[t] > 0) {
      last_byte[t] = A.text[t][A.bytes[t] - 1];
    }
  }
  for (int t = 0; t < A.n_texts; ++t) {
    open_line[t] = (A.flags & BPSW_FASTQ_FINAL) && A.bytes[t] > 0 && last_byte[t] != '\n';
    lines[t] = ((const long long*)c->h_stage_out.ptr)[t] + open_line[t];
  }
  const fq::Shape S = fq::fq_shape(A.n_texts, A.flags, lines, A.bytes);
  const long long n = S.n_reads;
  res->n_reads = n;
  res->bad_read = -1; res->bad_reason = 0;
  res->consumed[0] = res->consumed[1] = 0;
  res->needed[0] = n; res->needed[1] = res->needed[2] = 0;
  if (n == 0) {
    t_fq[4] = wall_ms() - t0;
    if (S.trunc_read >= 0) { res->bad_read = S.trunc_read; res->bad_reason = fq::R_TRUNCATED; return fq::PARSE_BAD; }
    fq::Outputs o;
    if (!room(*res, &o)) return fq::PARSE_CAPACITY;
    o.name_off[0] = 0;
    return fq::PARSE_OK;
  }
  // ---- line starts, the reads' records, their summed lengths ---------------------------------------------------------------------
  long long lt_room[2] = {0, 0};
  const long long scan_t = scan_tiles(n, tile_items);
  StageLayout L2;  // d_seed[1]
  size_t o_lt[2] = {0, 0};
  for (int t = 0; t < A.n_texts; ++t) {
    lt_room[t] = 4 * fq::fq_records_to_parse(lines[t], A.bytes[t]) + 1;
    o_lt[t] = L2.add(sizeof(fq::pos_t) * (size_t)lt_room[t]);
  }
  // (back in one copy after the emit: the two columns, then read_len)
  const size_t o_cols = L2.add(8 * 2 * ((size_t)n + 1)), o_rlen = L2.add(4 * (size_t)n), cols_bytes = L2.end - o_cols;
  const size_t o_seq = L2.add(4 * (size_t)n), o_qual = L2.add(4 * (size_t)n), o_name = L2.add(4 * (size_t)n);
  const size_t o_sums2 = L2.add(8 * 2 * (size_t)scan_t), o_res = L2.add(32);
  HIP_TRY(c->d_seed[1].reserve(L2.total()));
  uint8_t* W2 = (uint8_t*)c->d_seed[1].ptr;
  unsigned long long* d_res = (unsigned long long*)(W2 + o_res);
  HIP_TRY(hipMemsetAsync(d_res, 0xff, 8, s));
  HIP_TRY(hipMemsetAsync(d_res + 1, 0, 24, s));
  HIP_TRY(hipEventRecord(c->ev[0], s));
  for (int t = 0; t < A.n_texts; ++t) {
    T.lt[t] = (const fq::pos_t*)(W2 + o_lt[t]);
    hipLaunchKernelGGL(fastq_lines_kernel, dim3(tiles[t] ? grid_of(tiles[t] * 64) : 1u), dim3(kFqThreads), 0, s, T.text[t], T.bytes[t], tiles[t],
                       (const long long*)(W1 + o_cnt[t]), open_line[t], (fq::pos_t*)(W2 + o_lt[t]), lt_room[t]);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[1], s));
  FqReads R;
  R.cols = (long long*)(W2 + o_cols); R.read_len = (int32_t*)(W2 + o_rlen);
  R.seq_beg = (fq::pos_t*)(W2 + o_seq); R.qual_beg = (fq::pos_t*)(W2 + o_qual); R.name_beg = (fq::pos_t*)(W2 + o_name);
  hipLaunchKernelGGL(fastq_record_kernel, dim3(grid_of(n)), dim3(kFqThreads), 0, s, T, S, R, d_res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], s));
  HIP_TRY(scan_exclusive_i64(s, R.cols, 2, n, tile_items, (long long*)(W2 + o_sums2)));
  long long* hb = (long long*)c->h_stage_out.ptr;  // [0 .. 2] the result words, [4] the bases, [5] the names' bytes
  HIP_TRY(hipMemcpyAsync(hb, d_res, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hb + 4, R.cols + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hb + 5, R.cols + 2 * n + 1, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  t_fq[1] = ms;
  (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
  t_fq[2] = ms;
  const unsigned long long bad = (unsigned long long)hb[0];
  res->consumed[0] = hb[1]; res->consumed[1] = hb[2];
  const long long bases = hb[4], names = hb[5];
  res->needed[1] = bases; res->needed[2] = names;
  t_fq[4] = wall_ms() - t0;
  if (bad != ~0ull) { res->bad_read = (long long)(bad >> 8); res->bad_reason = (int)(bad & 0xff); return fq::PARSE_BAD; }
  if (S.trunc_read >= 0) { res->bad_read = S.trunc_read; res->bad_reason = fq::R_TRUNCATED; return fq::PARSE_BAD; }
  fq::Outputs o;
  if (!room(*res, &o)) return fq::PARSE_CAPACITY;
  // ---- the pools ------------------------------------------------------------------------------------------------------------------
  StageOut out;
  const int r_seq = out.add((size_t)bases), r_qual = out.add((size_t)bases), r_names = out.add((size_t)names), r_cols = out.add(cols_bytes);
  HIP_TRY(out.reserve(c->h_stage_out, c->d_sw_out));
  HIP_TRY(hipEventRecord(c->ev[0], s));
  if (bases) {
    hipLaunchKernelGGL(fastq_emit_kernel, dim3(grid_of((bases + 3) / 4)), dim3(kFqThreads), 0, s, T, S.two, n, (const long long*)R.cols,
                       (const fq::pos_t*)R.seq_beg, (const fq::pos_t*)R.qual_beg, out.dev<uint8_t>(r_seq), out.dev<uint8_t>(r_qual), 1);
    HIP_TRY(hipGetLastError());
  }
  if (names) {
    hipLaunchKernelGGL(fastq_emit_kernel, dim3(grid_of((names + 3) / 4)), dim3(kFqThreads), 0, s, T, S.two, n, (const long long*)(R.cols + n + 1),
                       (const fq::pos_t*)R.name_beg, (const fq::pos_t*)nullptr, out.dev<uint8_t>(r_names), (uint8_t*)nullptr, 0);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[1], s));
  HIP_TRY(hipMemcpyAsync(out.dev<uint8_t>(r_cols), W2 + o_cols, cols_bytes, hipMemcpyDeviceToDevice, s));
  HIP_TRY(out.fetch(s));
  HIP_TRY(hipStreamSynchronize(s));
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  t_fq[3] = ms;
  const long long* col = out.host<long long>(r_cols);
  memcpy(o.read_pool, out.host<uint8_t>(r_seq), (size_t)bases);
  memcpy(o.qual_pool, out.host<uint8_t>(r_qual), (size_t)bases);
  memcpy(o.name_pool, out.host<char>(r_names), (size_t)names);
  memcpy(o.read_off, col, 8 * (size_t)n);
  memcpy(o.read_len, (const uint8_t*)col + (o_rlen - o_cols), 4 * (size_t)n);
  const long long* ncol = col + n + 1;
  if (S.pair_names) {
    for (long long k = 0; k < n / 2; ++k) o.name_off[k] = ncol[2 * k];
    o.name_off[n / 2] = ncol[n];
  } else {
    memcpy(o.name_off, ncol, 8 * ((size_t)n + 1));
  }
  t_fq[4] = wall_ms() - t0;
  return fq::PARSE_OK;
}

// the arguments every entry checks the same way; A is filled
int check_texts(const char* who, const char* text1, size_t bytes1, const char* text2, size_t bytes2, int flags, Caller* A) {
  const std::string w(who);
  if (flags & ~(BPSW_FASTQ_FINAL | BPSW_FASTQ_INTERLEAVED | BPSW_FASTQ_PAIR_NAMES | BPSW_FASTQ_HOST)) return fail(BPSW_ERR_ARG, w + ": unknown flag");
  if ((!text1 && bytes1) || (!text2 && bytes2)) return fail(BPSW_ERR_ARG, w + ": null argument");
  if (text2 && (flags & BPSW_FASTQ_INTERLEAVED)) return fail(BPSW_ERR_ARG, w + ": BPSW_FASTQ_INTERLEAVED with two texts");
  if (!text2 && (flags & BPSW_FASTQ_PAIR_NAMES) && !(flags & BPSW_FASTQ_INTERLEAVED))
    return fail(BPSW_ERR_ARG, w + ": BPSW_FASTQ_PAIR_NAMES needs two texts or BPSW_FASTQ_INTERLEAVED");
  if (bytes1 >= ((size_t)1 << 31) || bytes2 >= ((size_t)1 << 31)) return fail(BPSW_ERR_LIMIT, w + ": a text of 2^31 bytes or more");
  A->who = who;
  A->text[0] = text1 ? text1 : ""; A->bytes[0] = (long long)bytes1;
  A->text[1] = text2; A->bytes[1] = text2 ? (long long)bytes2 : 0;
  A->n_texts = text2 ? 2 : 1;
  A->flags = flags;
  return BPSW_OK;
}

// ... and what the BGZF entries check on top: the headers of every chunk, that a final chunk ends on a block, the skips, the limit.
// A's texts become the inflated ones (no host pointer, the bytes behind the skip).
int open_bgzf(const int32_t skip[2], Caller* A, Bgzf* Z) {
  const std::string w(A->who);
  for (int t = 0; t < A->n_texts; ++t) {
    const std::string wt = w + ": text " + std::to_string(t + 1);
    Z->in[t] = A->text[t];
    Z->skip[t] = skip[t];
    ic::Walk& W = Z->walk[t];
    ic::bgzf_walk((const uint8_t*)A->text[t], A->bytes[t], &W);
    if (W.bad_reason) return refuse_block(A->who, t, W.bad_block, W.bad_reason);
    if ((A->flags & BPSW_FASTQ_FINAL) && W.consumed != A->bytes[t]) return fail(BPSW_ERR_ARG, wt + ": the text ends inside a BGZF block");
    if (skip[t] < 0 || (W.blocks.empty() ? skip[t] != 0 : (uint32_t)skip[t] > W.blocks[0].isize))
      return fail(BPSW_ERR_ARG, wt + ": skip is not within the first block's bytes");
    if (W.total >= (1ll << 31)) return fail(BPSW_ERR_LIMIT, wt + ": 2^31 inflated bytes or more");
    A->text[t] = nullptr;
    A->bytes[t] = W.total - skip[t];
  }
  return BPSW_OK;
}

// one parse by either path; PARSE_BAD has become the refusal, PARSE_CAPACITY is the caller's to report
template <class Room>
int parse_any(bpsw_ctx* c, const Caller& A, Room&& room, fq::Result* res, int* how, const Bgzf* Z = nullptr) {
  if (A.flags & BPSW_FASTQ_HOST) {
    const double t0 = wall_ms();
    Caller H = A;
    if (Z) {  // inflate_serial into a buffer of the calling thread; the text begins `skip` bytes into it
      thread_local std::vector<uint8_t> text[2];
      thread_local std::vector<ic::Work> work(1);
      for (int t = 0; t < A.n_texts; ++t) {
        if (text[t].size() < (size_t)Z->walk[t].total + 1) text[t].resize((size_t)Z->walk[t].total + 1);
        long long bad_block = -1;
        const int reason = ic::inflate_serial(work[0], (const uint8_t*)Z->in[t], Z->walk[t], text[t].data(), &bad_block);
        if (reason) return refuse_block(A.who, t, bad_block, reason);
        H.text[t] = (const char*)text[t].data() + Z->skip[t];
      }
    }
    *how = fq::parse_serial(H.text, H.bytes, H.n_texts, H.flags, room, res);
    t_fq[0] = t_fq[1] = t_fq[2] = t_fq[3] = 0.;
    t_fq[4] = wall_ms() - t0;
  } else {
    ContextEntry entry(c);
    if (entry.rc != BPSW_OK) return entry.rc;
    const int rc = parse_device(c, A, room, res, Z);
    if (rc < 0) return rc;
    *how = rc;
  }
  if (Z)  // how far each text was consumed, as a virtual offset
    for (int t = 0; t < A.n_texts; ++t) res->consumed[t] = ic::virtual_offset(Z->walk[t], (long long)Z->skip[t] + res->consumed[t]);
  if (*how == fq::PARSE_BAD) {
    long long lines[2] = {0, 0};  // (the shape's mapping of reads to records does not depend on the line counts)
    return refuse(A, fq::fq_shape(A.n_texts, A.flags, lines, A.bytes), res->bad_read, res->bad_reason);
  }
  return BPSW_OK;
}

// the pools of a parse inside one of the align entries: sized when the parse knows what it needs, kept by the calling thread
struct Parsed {
  std::vector<int32_t> read_len;
  std::vector<int64_t> read_off, name_off;
  std::vector<uint8_t> read_pool, qual_pool;
  std::vector<char> name_pool;
  bool operator()(const fq::Result& r, fq::Outputs* o) {
    const size_t n = (size_t)r.needed[0] + 1, pool = (size_t)r.needed[1] + 1, names = (size_t)r.needed[2] + 1;
    if (read_len.size() < n) { read_len.resize(n); read_off.resize(n); name_off.resize(n); }
    if (read_pool.size() < pool) { read_pool.resize(pool); qual_pool.resize(pool); }
    if (name_pool.size() < names) name_pool.resize(names);
    o->read_len = read_len.data(); o->read_off = read_off.data(); o->read_pool = read_pool.data(); o->qual_pool = qual_pool.data();
    o->name_off = name_off.data(); o->name_pool = name_pool.data();
    return true;
  }
};

// the bodies of the align entries: the parse, then the align entry of the form asked for (bam: the BAM twin, which has no out_off)
// skip: null for plain text, else the texts are BGZF chunks and skip[t] text t's
int fastq_se(const char* who, bool bam, bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text,
             size_t bytes, const int32_t* skip, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags, char* out_text, size_t text_cap,
             int64_t* out_off, int64_t max_reads, size_t* out_needed, int64_t* n_reads, int64_t* consumed) {
  const std::string w(who);
  if (!c || !opt || !sopt || !topt || (!bam && !out_off) || !n_reads || !consumed || max_reads < 0) return fail(BPSW_ERR_ARG, w + ": null argument");
  if (fastq_flags & (BPSW_FASTQ_INTERLEAVED | BPSW_FASTQ_PAIR_NAMES)) return fail(BPSW_ERR_ARG, w + ": a pair flag in a single-end call");
  Caller A;
  int rc = check_texts(who, text, bytes, nullptr, 0, fastq_flags, &A);
  if (rc != BPSW_OK) return rc;
  thread_local Parsed P;  // (grown, never shrunk: fresh pools of a 30 MB chunk cost the call more than its parse)
  thread_local Bgzf Z;
  fq::Result res;
  int how = fq::PARSE_OK;
  *n_reads = 0; *consumed = 0;
  if (skip && (rc = open_bgzf(skip, &A, &Z)) != BPSW_OK) return rc;
  rc = parse_any(c, A, P, &res, &how, skip ? &Z : nullptr);
  if (rc != BPSW_OK) return rc;
  *n_reads = res.n_reads;
  if (!bam && res.n_reads > max_reads) return fail(BPSW_ERR_CAPACITY, w + ": out_off has room for fewer reads than the text holds (*n_reads)");
  if (res.n_reads > 0x7fffffffll) return fail(BPSW_ERR_LIMIT, w + ": more than 2^31 - 1 reads");
  bpsw_se_reads_t g;
  memset(&g, 0, sizeof g);
  g.n_reads = (int32_t)res.n_reads; g.id0 = id0; g.id_step = id_step;
  g.read_len = P.read_len.data(); g.read_off = P.read_off.data(); g.read_pool = P.read_pool.data(); g.qual_pool = P.qual_pool.data();
  g.read_pool_bytes = (size_t)res.needed[1];
  g.name_off = P.name_off.data(); g.name_pool = P.name_pool.data();
  rc = bam ? bpsw_align_bam_se_batch(c, opt, sopt, topt, &g, zdrop_mode, w1_flags, flags, out_text, text_cap, out_needed)
           : bpsw_align_se_batch(c, opt, sopt, topt, &g, zdrop_mode, w1_flags, flags, out_text, text_cap, out_off, out_needed);
  if (rc == BPSW_OK || rc == BPSW_ERR_CAPACITY) *consumed = res.consumed[0];
  return rc;
}

int fastq_pe(const char* who, bool bam, bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text1,
             size_t bytes1, const char* text2, size_t bytes2, const int32_t* skip, int fastq_flags, int64_t id0, const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags,
             int rescue_mode, int flags, char* out_text, size_t text_cap, int64_t* out_off, int64_t max_reads, size_t* out_needed,
             bpsw_pestat_t* out_pes, int64_t* n_reads, int64_t consumed[2]) {
  const std::string w(who);
  if (!c || !opt || !sopt || !topt || (!bam && !out_off) || !n_reads || !consumed || max_reads < 0) return fail(BPSW_ERR_ARG, w + ": null argument");
  if (!text2 && !(fastq_flags & BPSW_FASTQ_INTERLEAVED)) return fail(BPSW_ERR_ARG, w + ": one text without BPSW_FASTQ_INTERLEAVED");
  if (!text2) fastq_flags |= BPSW_FASTQ_PAIR_NAMES;
  Caller A;
  int rc = check_texts(who, text1, bytes1, text2, bytes2, fastq_flags, &A);
  if (rc != BPSW_OK) return rc;
  thread_local Parsed P;
  thread_local Bgzf Z;
  fq::Result res;
  int how = fq::PARSE_OK;
  *n_reads = 0; consumed[0] = consumed[1] = 0;
  if (skip && (rc = open_bgzf(skip, &A, &Z)) != BPSW_OK) return rc;
  rc = parse_any(c, A, P, &res, &how, skip ? &Z : nullptr);
  if (rc != BPSW_OK) return rc;
  *n_reads = res.n_reads;
  if (!bam && res.n_reads > max_reads) return fail(BPSW_ERR_CAPACITY, w + ": out_off has room for fewer reads than the texts hold (*n_reads)");
  if (res.n_reads / 2 > 0x7fffffffll) return fail(BPSW_ERR_LIMIT, w + ": more than 2^31 - 1 pairs");
  bpsw_pairs_t g;
  memset(&g, 0, sizeof g);
  g.group_size = (int32_t)(res.n_reads / 2); g.id0 = id0;
  g.read_len = P.read_len.data(); g.read_off = P.read_off.data(); g.read_pool = P.read_pool.data(); g.qual_pool = P.qual_pool.data();
  g.read_pool_bytes = (size_t)res.needed[1];
  g.name_off = P.name_off.data(); g.name_pool = P.name_pool.data();
  rc = bam ? bpsw_align_bam_pe_batch(c, opt, sopt, topt, &g, pes0, zdrop_mode, w1_flags, rescue_mode, flags, out_text, text_cap, out_needed, out_pes)
           : bpsw_align_pe_batch(c, opt, sopt, topt, &g, pes0, zdrop_mode, w1_flags, rescue_mode, flags, out_text, text_cap, out_off, out_needed, out_pes);
  if (rc == BPSW_OK || rc == BPSW_ERR_CAPACITY) { consumed[0] = res.consumed[0]; consumed[1] = res.consumed[1]; }
  return rc;
}

}  // namespace

extern "C" {

static int fastq_parse_body(const char* who, bpsw_ctx_t* c, const char* text1, size_t bytes1, const char* text2, size_t bytes2, const int32_t* skip,
                            int flags, int64_t max_reads, size_t pool_cap, size_t name_cap, int32_t* read_len, int64_t* read_off, uint8_t* read_pool,
                            uint8_t* qual_pool, int64_t* name_off, char* name_pool, int64_t* n_reads, int64_t consumed[2], int64_t needed[3]) {
  const std::string w(who);
  if ((!c && !(flags & BPSW_FASTQ_HOST)) || !read_len || !read_off || !read_pool || !qual_pool || !name_off || !name_pool || !n_reads || !consumed ||
      !needed || max_reads < 0)
    return fail(BPSW_ERR_ARG, w + ": null argument");
  Caller A;
  int rc = check_texts(who, text1, bytes1, text2, bytes2, flags, &A);
  if (rc != BPSW_OK) return rc;
  thread_local Bgzf Z;
  auto room = [&](const fq::Result& r, fq::Outputs* o) {
    if (r.needed[0] > max_reads || (unsigned long long)r.needed[1] > pool_cap || (unsigned long long)r.needed[2] > name_cap) return false;
    o->read_len = read_len; o->read_off = read_off; o->read_pool = read_pool; o->qual_pool = qual_pool;
    o->name_off = name_off; o->name_pool = name_pool;
    return true;
  };
  fq::Result res;
  int how = fq::PARSE_OK;
  *n_reads = 0;
  consumed[0] = consumed[1] = 0;
  needed[0] = needed[1] = needed[2] = 0;
  if (skip && (rc = open_bgzf(skip, &A, &Z)) != BPSW_OK) return rc;
  rc = parse_any(c, A, room, &res, &how, skip ? &Z : nullptr);
  if (rc != BPSW_OK) return rc;
  for (int k = 0; k < 3; ++k) needed[k] = res.needed[k];
  if (how == fq::PARSE_CAPACITY)
    return fail(BPSW_ERR_CAPACITY, w + ": the outputs are too small (needed: " + std::to_string(res.needed[0]) + " reads, " +
                                       std::to_string(res.needed[1]) + " pool bytes, " + std::to_string(res.needed[2]) + " name bytes)");
  *n_reads = res.n_reads;
  consumed[0] = res.consumed[0]; consumed[1] = res.consumed[1];
  return BPSW_OK;
}

int bpsw_fastq_parse(bpsw_ctx_t* c, const char* text1, size_t bytes1, const char* text2, size_t bytes2, int flags, int64_t max_reads,
                     size_t pool_cap, size_t name_cap, int32_t* read_len, int64_t* read_off, uint8_t* read_pool, uint8_t* qual_pool,
                     int64_t* name_off, char* name_pool, int64_t* n_reads, int64_t consumed[2], int64_t needed[3]) {
  return fastq_parse_body("fastq_parse", c, text1, bytes1, text2, bytes2, nullptr, flags, max_reads, pool_cap, name_cap, read_len, read_off, read_pool,
                          qual_pool, name_off, name_pool, n_reads, consumed, needed);
}

int bpsw_align_fastq_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text,
                        size_t bytes, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags, char* out_text,
                        size_t text_cap, int64_t* out_off, int64_t max_reads, size_t* out_needed, int64_t* n_reads, int64_t* consumed) {
  return fastq_se("align_fastq_se", false, c, opt, sopt, topt, text, bytes, nullptr, fastq_flags, id0, id_step, zdrop_mode, w1_flags, flags, out_text, text_cap,
                  out_off, max_reads, out_needed, n_reads, consumed);
}

int bpsw_align_fastq_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text1,
                        size_t bytes1, const char* text2, size_t bytes2, int fastq_flags, int64_t id0, const bpsw_pestat_t* pes0, int zdrop_mode,
                        int w1_flags, int rescue_mode, int flags, char* out_text, size_t text_cap, int64_t* out_off, int64_t max_reads,
                        size_t* out_needed, bpsw_pestat_t* out_pes, int64_t* n_reads, int64_t consumed[2]) {
  return fastq_pe("align_fastq_pe", false, c, opt, sopt, topt, text1, bytes1, text2, bytes2, nullptr, fastq_flags, id0, pes0, zdrop_mode, w1_flags, rescue_mode,
                  flags, out_text, text_cap, out_off, max_reads, out_needed, out_pes, n_reads, consumed);
}

// the BAM twins (the other writer is bpsw_bam.hip's: these only end in its align entries)
int bpsw_align_fastq_bam_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text,
                            size_t bytes, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags, char* out,
                            size_t cap, size_t* out_needed, int64_t* n_reads, int64_t* consumed) {
  return fastq_se("align_fastq_bam_se", true, c, opt, sopt, topt, text, bytes, nullptr, fastq_flags, id0, id_step, zdrop_mode, w1_flags, flags, out, cap, nullptr,
                  0, out_needed, n_reads, consumed);
}

int bpsw_align_fastq_bam_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text1,
                            size_t bytes1, const char* text2, size_t bytes2, int fastq_flags, int64_t id0, const bpsw_pestat_t* pes0,
                            int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out, size_t cap, size_t* out_needed,
                            bpsw_pestat_t* out_pes, int64_t* n_reads, int64_t consumed[2]) {
  return fastq_pe("align_fastq_bam_pe", true, c, opt, sopt, topt, text1, bytes1, text2, bytes2, nullptr, fastq_flags, id0, pes0, zdrop_mode, w1_flags,
                  rescue_mode, flags, out, cap, nullptr, 0, out_needed, out_pes, n_reads, consumed);
}

// the same entries over BGZF chunks (bpsw_bgzf_in.hip inflates them; the text stays on the device)
int bpsw_fastq_bgzf_parse(bpsw_ctx_t* c, const char* text1, size_t bytes1, int32_t skip1, const char* text2, size_t bytes2, int32_t skip2, int flags,
                          int64_t max_reads, size_t pool_cap, size_t name_cap, int32_t* read_len, int64_t* read_off, uint8_t* read_pool,
                          uint8_t* qual_pool, int64_t* name_off, char* name_pool, int64_t* n_reads, int64_t consumed[2], int64_t needed[3]) {
  const int32_t skip[2] = {skip1, skip2};
  return fastq_parse_body("fastq_bgzf_parse", c, text1, bytes1, text2, bytes2, skip, flags, max_reads, pool_cap, name_cap, read_len, read_off,
                          read_pool, qual_pool, name_off, name_pool, n_reads, consumed, needed);
}

int bpsw_align_fastq_bgzf_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text,
                             size_t bytes, int32_t skip, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags,
                             char* out_text, size_t text_cap, int64_t* out_off, int64_t max_reads, size_t* out_needed, int64_t* n_reads,
                             int64_t* consumed) {
  const int32_t sk[2] = {skip, 0};
  return fastq_se("align_fastq_bgzf_se", false, c, opt, sopt, topt, text, bytes, sk, fastq_flags, id0, id_step, zdrop_mode, w1_flags, flags, out_text,
                  text_cap, out_off, max_reads, out_needed, n_reads, consumed);
}

int bpsw_align_fastq_bgzf_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text1,
                             size_t bytes1, int32_t skip1, const char* text2, size_t bytes2, int32_t skip2, int fastq_flags, int64_t id0,
                             const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out_text, size_t text_cap,
                             int64_t* out_off, int64_t max_reads, size_t* out_needed, bpsw_pestat_t* out_pes, int64_t* n_reads, int64_t consumed[2]) {
  const int32_t sk[2] = {skip1, skip2};
  return fastq_pe("align_fastq_bgzf_pe", false, c, opt, sopt, topt, text1, bytes1, text2, bytes2, sk, fastq_flags, id0, pes0, zdrop_mode, w1_flags,
                  rescue_mode, flags, out_text, text_cap, out_off, max_reads, out_needed, out_pes, n_reads, consumed);
}

int bpsw_align_fastq_bgzf_bam_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text,
                                 size_t bytes, int32_t skip, int fastq_flags, int64_t id0, int32_t id_step, int zdrop_mode, int w1_flags, int flags,
                                 char* out, size_t cap, size_t* out_needed, int64_t* n_reads, int64_t* consumed) {
  const int32_t sk[2] = {skip, 0};
  return fastq_se("align_fastq_bgzf_bam_se", true, c, opt, sopt, topt, text, bytes, sk, fastq_flags, id0, id_step, zdrop_mode, w1_flags, flags, out, cap,
                  nullptr, 0, out_needed, n_reads, consumed);
}

int bpsw_align_fastq_bgzf_bam_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const char* text1,
                                 size_t bytes1, int32_t skip1, const char* text2, size_t bytes2, int32_t skip2, int fastq_flags, int64_t id0,
                                 const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out, size_t cap,
                                 size_t* out_needed, bpsw_pestat_t* out_pes, int64_t* n_reads, int64_t consumed[2]) {
  const int32_t sk[2] = {skip1, skip2};
  return fastq_pe("align_fastq_bgzf_bam_pe", true, c, opt, sopt, topt, text1, bytes1, text2, bytes2, sk, fastq_flags, id0, pes0, zdrop_mode, w1_flags,
                  rescue_mode, flags, out, cap, nullptr, 0, out_needed, out_pes, n_reads, consumed);
}

void bpsw_last_fastq_times(double ms[5]) {
  if (ms) memcpy(ms, t_fq, sizeof t_fq);
}

}  // extern "C"
