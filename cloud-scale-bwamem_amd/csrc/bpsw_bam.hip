// bpsw_bam.hip -- alignments out as BAM: the records of a call's lines and the BGZF blocks around them, written on the device; the
// header and the end-of-file block on the calling thread.  Behind the C ABI: bpsw_bam_se_batch, bpsw_bam_pe_batch,
// bpsw_align_bam_se_batch, bpsw_align_bam_pe_batch (bpsw_align_fastq_bam_* are bpsw_fastq.hip's and end here), bpsw_sam_header,
// bpsw_bam_header (and the two with _ex), bpsw_bam_eof, bpsw_bam_set_block_payload, bpsw_last_bam_times, bpsw_last_bam_deflate_times.
//
// bam_on_device is a second writer beside text_on_device (bpsw_sam_se.hip): the entries hand it to sam_batch (bpsw_tail.cpp) through
// the same pointer, it stages the same line table (stage_lines, with the mate assertion), and it has the text's shape -- a length per
// line, the host's prefix sum, a write per line -- with a third kernel behind it:
//   bam_len_kernel     one line per lane: the number of bytes of its record (bpsw_bam_core.h); the host sums them to record offsets
//                      and the stream's size S, from which the framed size S + 31 ceil(S / P) and the capacity verdict follow;
//   bam_write_kernel   one line per lane: the record at its offset in one device block, the stream;
//   bgzf_frame_kernel  one wavefront per BGZF block: payload b is stream[b P, b P + P) (the last one is shorter), copied to its framed
//                      place 16 bytes a lane; its CRC-32 from 64 contiguous slices, one a lane, over a byte table in LDS, each
//                      slice's CRC shifted by the bytes behind the slice (crc32_shift) and the 64 XORed across the wave; the 23
//                      bytes in front and the 8 behind stored by the first lanes.  A block depends on no other block.
// The framed block comes back in one copy; the stream never leaves the device.  With BPSW_BAM_DEFLATE the third kernel is another:
//   bgzf_deflate_kernel  one wavefront per block: the payload as one dynamic-Huffman deflate block with LZ77 matches (bpsw_deflate_core.h),
//                      or stored when that is not smaller, at a worst-case place of its own, and the block's size into a table;
//   bgzf_pack_kernel   one wavefront per block, once the host has summed the table: the block to its offset in the output.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "bpsw_tail_internal.h"
#include "bpsw_bam_core.h"
#include "bpsw_deflate_core.h"
#include "bpsw_wave.h"

using namespace bpsw;
namespace sc = bpsw::samcore;
namespace bc = bpsw::bamcore;
namespace dc = bpsw::deflcore;

namespace {

__global__ __launch_bounds__(64) void bam_len_kernel(sc::SamBatch B, int n_lines, int32_t* __restrict__ len) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  len[i] = (int32_t)bc::bam_rec_len(B, i);
}

// record i goes to stream[rec_off[i] .. rec_off[i + 1]); status: the OR of every record's bam_rec_write status
__global__ __launch_bounds__(64) void bam_write_kernel(sc::SamBatch B, int n_lines, const long long* __restrict__ rec_off, char* stream,
                                                       int* status) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  const long long at = rec_off[i], len = rec_off[i + 1] - at;
  int st = 0;
  bc::bam_rec_write(stream + at, stream + at + len, B, i, len, &st);
  if (st) atomicOr(status, st);
}

// block b of ceil(S / P): out[b (P + 31) ..) = head(23) | stream[b P .. b P + n) | CRC32 | ISIZE, n = min(P, S - b P)
__global__ __launch_bounds__(64) void bgzf_frame_kernel(const uint8_t* __restrict__ stream, long long S, int P, uint8_t* __restrict__ out) {
  __shared__ uint32_t tab[256];
  const int lane = (int)threadIdx.x;
  for (int k = 0; k < 4; ++k) tab[4 * lane + k] = bc::crc32_table_entry((uint32_t)(4 * lane + k));
  __syncthreads();
  const long long at = (long long)blockIdx.x * P;
  if (at >= S) return;
  const int n = (int)(S - at < P ? S - at : P);
  const uint8_t* src = stream + at;
  uint8_t* dst = out + (long long)blockIdx.x * (P + bc::kBgzfAround);
  uint8_t* pay = dst + bc::kBgzfHead;
  // ---- the payload: bytes up to the first 16-byte line of the destination, whole lines, the rest -----------------------------------
  int head = (int)((16 - ((uintptr_t)pay & 15)) & 15);
  if (head > n) head = n;
  const int lines = (n - head) / 16, rest = head + 16 * lines;
  if (lane < head) pay[lane] = src[lane];
  for (int v = lane; v < lines; v += 64) {
    uint4 x;
    __builtin_memcpy(&x, src + head + 16 * v, 16);  // (the source is wherever the cut fell)
    *reinterpret_cast<uint4*>(pay + head + 16 * v) = x;
  }
  if (rest + lane < n) pay[rest + lane] = src[rest + lane];  // (fewer than 16 bytes)
  // ---- the CRC: a slice a lane, a multiple of four bytes so that every lane's loads are aligned alike ---------------------------------
  const int slice = ((n + 63) / 64 + 3) & ~3;
  const int lo = lane * slice < n ? lane * slice : n, hi = lo + slice < n ? lo + slice : n;
  uint32_t crc = bc::crc32_shift(bc::crc32_bytes(tab, 0u, src + lo, hi - lo), n - hi);
  for (int d = 1; d < 64; d <<= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
  // ---- the bytes around it ------------------------------------------------------------------------------------------------------------
  if (lane < bc::kBgzfHead) dst[lane] = bc::bgzf_head_byte(lane, (uint32_t)n);
  if (lane < bc::kBgzfTail) pay[n + lane] = bc::bgzf_tail_byte(lane, crc, (uint32_t)n);
}

// ---- BPSW_BAM_DEFLATE: the payload as one dynamic-Huffman deflate block (bpsw_deflate_core.h) -----------------------------------------------
// (copy_lines, bpsw_wave.h: `n` bytes from src to dst, 16 bytes a lane where the destination allows -- bgzf_frame_kernel's payload copy)
// Block b of ceil(S / P), one wavefront: payload b compressed to wide[b stride ..), a place of its own that begins on a 16-byte line
// (the words two lanes share are OR-ed into by both, and they must not be a neighbour's), sizes[b] = its framed bytes.  tok: two bytes of
// scratch per byte of the stream.  The phases and what a lane does in each are bpsw_deflate_core.h's; the barriers are here.  When the
// deflate bytes would not be fewer than n + 5 the block is written as bgzf_frame_kernel writes it.  LDS: 70 892 bytes (dc::Work, of which
// 64 KB are the lanes' hash tables), so two workgroups a CU.
__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t* __restrict__ stream, long long S, int P, uint16_t* tok_all,
                                                          uint8_t* wide, long long stride, uint32_t* __restrict__ sizes) {
  __shared__ dc::Work w;
  const int lane = (int)threadIdx.x;
  const long long at = (long long)blockIdx.x * P;
  if (at >= S) return;
  const int n = (int)(S - at < P ? S - at : P);
  const uint8_t* src = stream + at;
  uint16_t* tok = tok_all + at;
  uint8_t* dst = wide + (long long)blockIdx.x * stride;
  dc::init_lane(w, lane);
  __syncthreads();
  dc::lz_lane(w, lane, src, n, tok);
  __syncthreads();
  dc::rank_lane(w, w.ll_freq, dc::kNumLL, lane);
  __syncthreads();
  if (lane == 0) dc::lengths_serial(w, w.ll_freq, dc::kNumLL, dc::kBitsLL, w.ll_len);
  __syncthreads();
  dc::rank_lane(w, w.d_freq, dc::kNumD, lane);
  __syncthreads();
  if (lane == 0) { dc::lengths_serial(w, w.d_freq, dc::kNumD, dc::kBitsLL, w.d_len); dc::cl_counts_serial(w); }
  __syncthreads();
  dc::rank_lane(w, w.cl_freq, dc::kNumCL, lane);
  __syncthreads();
  if (lane == 0) { dc::lengths_serial(w, w.cl_freq, dc::kNumCL, dc::kBitsCL, w.cl_len); dc::header_serial(w); }
  __syncthreads();
  // ---- where each lane's bits begin, the CRC, the verdict ------------------------------------------------------------------------------
  const uint32_t bits = dc::count_lane(w, lane, n, tok);
  uint32_t upto = bits;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = (uint32_t)__shfl_up((int)upto, d, 64);
    if (lane >= d) upto += below;
  }
  const uint32_t token_bits = (uint32_t)__shfl((int)upto, 63, 64);
  uint32_t crc = dc::crc_lane(w, lane, src, n);
  for (int d = 1; d < 64; d <<= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
  const uint32_t dbytes = dc::deflate_bytes(w, token_bits);
  if (dbytes >= (uint32_t)n + dc::kStoredExtra) {
    copy_lines(src, dst + bc::kBgzfHead, n, lane);
    if (lane < bc::kBgzfHead) dst[lane] = bc::bgzf_head_byte(lane, (uint32_t)n);
    if (lane < bc::kBgzfTail) dst[bc::kBgzfHead + n + lane] = bc::bgzf_tail_byte(lane, crc, (uint32_t)n);
    if (lane == 0) sizes[blockIdx.x] = (uint32_t)n + bc::kBgzfAround;
    return;
  }
  // ---- the framed block: zeros from byte 16 on, then every lane's bits -------------------------------------------------------------------
  const uint32_t framed = dc::kHead + dbytes + bc::kBgzfTail;  // (< n + 31 <= stride, and so is its end rounded up to a word)
  uint32_t* words = reinterpret_cast<uint32_t*>(dst + 16);
  const uint32_t n_words = (framed - 16 + 3) / 4;
  for (uint32_t k = (uint32_t)lane; k < n_words; k += 64) words[k] = 0u;
  if (lane < 16) dst[lane] = bc::bgzf_deflate_head_byte(lane, dbytes);
  __threadfence();
  __syncthreads();
  dc::write_lane(w, lane, n, tok, words, upto - bits, token_bits, crc);
  if (lane == 0) sizes[blockIdx.x] = framed;
}

// block b: wide[b stride, b stride + off[b + 1] - off[b]) to out[off[b] ..)
__global__ __launch_bounds__(64) void bgzf_pack_kernel(const uint8_t* __restrict__ wide, long long stride, const long long* __restrict__ off,
                                                       uint8_t* __restrict__ out) {
  const long long to = off[blockIdx.x];
  copy_lines(wide + (long long)blockIdx.x * stride, out + to, (int)(off[blockIdx.x + 1] - to), (int)threadIdx.x);
}

std::atomic<int> g_payload{0};

// bam_len_kernel, bam_write_kernel, bgzf_frame_kernel, tables, round trip
thread_local double t_bam[5] = {0., 0., 0., 0., 0.};
// bgzf_deflate_kernel, bgzf_pack_kernel, the size table's way back with the offsets' way out, the copy of the packed blocks
thread_local double t_deflate[4] = {0., 0., 0., 0.};

// ---- the calling thread's side: the table, a payload framed without a device, the header ----------------------------------------------
const uint32_t* host_table() {
  static const std::vector<uint32_t> tab = [] {
    std::vector<uint32_t> t(256);
    for (uint32_t i = 0; i < 256; ++i) t[i] = bc::crc32_table_entry(i);
    return t;
  }();
  return tab.data();
}
void frame_host(const std::string& s, int P, char* out) {
  for (size_t at = 0; at < s.size(); at += (size_t)P) {
    const uint32_t n = (uint32_t)std::min(s.size() - at, (size_t)P);
    for (int k = 0; k < bc::kBgzfHead; ++k) *out++ = (char)bc::bgzf_head_byte(k, n);
    memcpy(out, s.data() + at, n);
    out += n;
    const uint32_t crc = bc::crc32_bytes(host_table(), 0u, (const uint8_t*)s.data() + at, n);
    for (int k = 0; k < bc::kBgzfTail; ++k) *out++ = (char)bc::bgzf_tail_byte(k, crc, n);
  }
}

struct Contigs {
  std::vector<std::string> name;
  std::vector<int32_t> len;
};
int contigs_of(const char* who, bpsw_ctx_t* c, int32_t n_seqs, const int32_t* len, const char* names, Contigs* out) {
  if (c) {
    BnsView bns;
    const int rc = snapshot_bns(c, &bns);
    if (rc != BPSW_OK) return rc;
    out->name = bns.name; out->len = bns.len;
  } else {
    if (n_seqs < 0 || (n_seqs > 0 && !len)) return fail(BPSW_ERR_ARG, std::string(who) + ": no context and no contig table");
    out->len.assign(len, len + n_seqs);
    out->name.assign((size_t)n_seqs, std::string());
    for (int k = 0; names && k < n_seqs; ++k) { out->name[(size_t)k] = names; names += out->name[(size_t)k].size() + 1; }
  }
  for (size_t k = 0; k < out->name.size(); ++k)
    if (out->name[k].empty()) out->name[k] = "ctg" + std::to_string(k + 1);  // (put_contig's rule)
  return BPSW_OK;
}
std::string header_text(const Contigs& t, const char* extra, size_t extra_bytes, int flags) {
  std::string s = (flags & BPSW_HDR_COORDINATE) ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\n";
  for (size_t k = 0; k < t.name.size(); ++k) s += "@SQ\tSN:" + t.name[k] + "\tLN:" + std::to_string(t.len[k]) + "\n";
  if (extra && extra_bytes) s.append(extra, extra_bytes);
  return s;
}
void append_u32(std::string& s, uint32_t v) {
  char b[4];
  bc::store_u32(b, v);
  s.append(b, 4);
}
// what the three host entries do with their bytes
int hand_out(const char* who, const char* src, size_t n, char* out, size_t cap, size_t* out_needed) {
  if (out_needed) *out_needed = n;
  if (!out || n > cap) return fail(BPSW_ERR_CAPACITY, std::string(who) + ": buffer too small (see *out_needed)");
  if (n) memcpy(out, src, n);
  return BPSW_OK;
}

int se_tail(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g, int flags, char* out, size_t cap,
            int64_t*, size_t* out_needed, bpsw_alnreg_t* out_regs) {
  return bpsw_bam_se_batch(c, opt, topt, g, flags, out, cap, out_needed, out_regs);
}
int pe_tail(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, int flags, char* out, size_t cap, int64_t*,
            size_t* out_needed, bpsw_alnreg_t* out_regs) {
  return bpsw_bam_pe_batch(c, opt, topt, g, flags, out, cap, out_needed, out_regs);
}
// the record offsets sam_batch asks its writer for: the BAM entries have no out_off, the calling thread keeps them
int64_t* own_offsets(long long n_reads) {
  static thread_local std::vector<int64_t> off;
  const size_t want = n_reads > 0 && n_reads <= (2ll << 29) ? (size_t)n_reads + 1 : 1;  // (past that sam_batch refuses before it looks)
  if (off.size() < want) off.resize(want);
  return off.data();
}

// What follows the lengths with BPSW_BAM_DEFLATE: the records, a compressed block per payload at its worst-case place, the table of their
// sizes back to the calling thread, which sums it as it summed the lengths; then, when the sum fits `cap`, the blocks packed to their
// offsets and copied out in one piece.  *total_out is the sum: the size is known only here, so the blocks are made whatever `cap` is.
// One reservation of c->d_gl_z holds it all: [packed blocks | status | sizes] (what comes back), the stream, the blocks at their
// stride, and the tokens (two bytes a stream byte).
int deflate_on_device(bpsw_ctx* c, const std::string& w, const sc::SamBatch& B, int n_lines, const std::vector<long long>& rec_off, size_t S, int P,
                      size_t blocks, char* out, size_t cap, size_t* total_out, double times[5], double t1) {
  const dim3 grid((unsigned)((n_lines + 63) / 64));
  const size_t stride = bgzf_deflate_stride(P);
  StageIn io;
  const int i_off = io.add(rec_off.data(), 8 * ((size_t)n_lines + 1));
  StageOut fr;
  const int r_out = fr.add(bgzf_framed_size(S, P)), r_status = fr.add(16), r_sizes = fr.add(4 * blocks);
  StageLayout dev;
  dev.add(fr.total());
  const size_t o_stream = dev.add(S), o_wide = dev.add(blocks * stride, 256), o_tok = dev.add(2 * S);
  HIP_TRY(c->d_gl_z.reserve(dev.total()));
  HIP_TRY(fr.reserve(c->h_stage_out, c->d_gl_z));
  uint8_t* base = (uint8_t*)c->d_gl_z.ptr;
  HIP_TRY(io.stage(c->h_stage_in, c->d_sw_out, c->stream));
  HIP_TRY(hipMemsetAsync(fr.dev<int>(r_status), 0, 16, c->stream));
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  hipLaunchKernelGGL(bam_write_kernel, grid, dim3(64), 0, c->stream, B, n_lines, io.dev<long long>(i_off), (char*)(base + o_stream),
                     fr.dev<int>(r_status));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(launch_bgzf_deflate(c->stream, base + o_stream, (long long)S, P, blocks, (uint16_t*)(base + o_tok), base + o_wide,
                              fr.dev<uint32_t>(r_sizes)));
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  const size_t back = fr.total() - fr.at[r_status];  // (the status and the sizes lie together)
  HIP_TRY(hipMemcpyAsync(fr.h + fr.at[r_status], fr.d + fr.at[r_status], back, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double t2 = wall_ms();
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev[6], c->ev[7]);
  times[1] = ms;
  (void)hipEventElapsedTime(&ms, c->ev[7], c->ev[0]);
  t_deflate[0] = ms;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  t_deflate[2] = ms;
  if (*fr.host<int>(r_status)) return fail(BPSW_ERR_DEVICE, w + ": a record's bytes differ in number from its length (bam_rec_write's status)");
  std::vector<long long> off;
  if (!bgzf_block_offsets(fr.host<uint32_t>(r_sizes), S, P, blocks, &off))
    return fail(BPSW_ERR_DEVICE, w + ": a block came back with a size no block has");
  const size_t total = (size_t)off[blocks];
  *total_out = total;
  if (!out || total > cap) { times[4] = wall_ms() - t1; return BPSW_OK; }  // (the caller reports the capacity)
  StageIn po;  // (the record offsets have been used)
  const int p_off = po.add(off.data(), 8 * (blocks + 1));
  HIP_TRY(po.stage(c->h_stage_in, c->d_sw_out, c->stream));
  t_deflate[2] += wall_ms() - t2;
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  HIP_TRY(launch_bgzf_pack(c->stream, base + o_wide, P, po.dev<long long>(p_off), blocks, fr.dev<uint8_t>(r_out)));
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(hipMemcpyAsync(fr.h + fr.at[r_out], fr.d + fr.at[r_out], total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&ms, c->ev[6], c->ev[7]);
  t_deflate[1] = ms;
  (void)hipEventElapsedTime(&ms, c->ev[7], c->ev[0]);
  t_deflate[3] = ms;
  memcpy(out, fr.host<char>(r_out), total);
  times[4] = wall_ms() - t1;
  return BPSW_OK;
}

// the writer with and without BPSW_BAM_DEFLATE: one body up to the stream's size
int bam_device(bool deflate, bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& sl,
               char* out, size_t cap, int64_t* out_off, size_t* total_out, double times[5]) {
  const std::vector<int32_t>& read_first = sl.read_first;
  const int n = g.n, n_lines = (int)sl.aa.size(), n_names = g.n >> g.name_shift;
  const std::string w = std::string(who) + " as BAM";
  for (int k = 0; k < n_names; ++k)
    if (g.name_off[k + 1] - g.name_off[k] > bc::kMaxName)
      return fail(BPSW_ERR_LIMIT, w + ": a read name of more than 254 bytes cannot be a BAM record (name " + std::to_string(k) + ")");
  const double t0 = wall_ms();
  StageOut lens;
  const int r_len = lens.add(4 * (size_t)n_lines);
  HIP_TRY(lens.reserve(c->h_stage_out, c->d_sw_out));
  StageIn in;
  sc::SamBatch B;
  const int rc = stage_lines(c, w, bns, t, g, sl, &in, &B);
  if (rc != BPSW_OK) return rc;
  const dim3 grid((unsigned)((n_lines + 63) / 64));
  const double t1 = wall_ms();
  // ---- lengths ---------------------------------------------------------------------------------------------------------------
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  hipLaunchKernelGGL(bam_len_kernel, grid, dim3(64), 0, c->stream, B, n_lines, lens.dev<int32_t>(r_len));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(lens.fetch(c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev[6], c->ev[7]);
  std::vector<long long> rec_off((size_t)n_lines + 1, 0);
  const int32_t* hl = lens.host<int32_t>(r_len);
  for (int i = 0; i < n_lines; ++i) {
    if (hl[i] < 37) return fail(BPSW_ERR_DEVICE, w + ": a record came back shorter than its fixed part");
    rec_off[(size_t)i + 1] = rec_off[(size_t)i] + hl[i];
  }
  for (int r = 0; r <= n; ++r) out_off[r] = (int64_t)rec_off[(size_t)read_first[(size_t)r]];
  const size_t S = (size_t)rec_off[(size_t)n_lines];
  const int P = bam_payload_bytes();
  const size_t blocks = (S + (size_t)P - 1) / (size_t)P, total = bgzf_framed_size(S, P);
  *total_out = total;
  times[0] = ms; times[1] = times[2] = 0.; times[3] = t1 - t0;
  if (deflate) {
    if (blocks > 0x7fffffffull) return fail(BPSW_ERR_LIMIT, w + ": more than 2^31 - 1 BGZF blocks");
    return deflate_on_device(c, w, B, n_lines, rec_off, S, P, blocks, out, cap, total_out, times, t1);
  }
  if (!out || total > cap) { times[4] = wall_ms() - t1; return BPSW_OK; }  // (the caller reports the capacity)
  if (blocks > 0x7fffffffull) return fail(BPSW_ERR_LIMIT, w + ": more than 2^31 - 1 BGZF blocks");
  // ---- records, then blocks ---------------------------------------------------------------------------------------------------------
  // (the pinned input block is free again: its copy has been waited for; the line table stays where it is on the device)
  StageIn io;
  const int i_off = io.add(rec_off.data(), 8 * ((size_t)n_lines + 1));
  StageOut fr;
  const int r_out = fr.add(total), r_status = fr.add(16);
  HIP_TRY(c->d_gl_z.reserve(fr.total() + S));  // (the backtrack scratch of run_jobs, free by now: the framed block, then the stream)
  HIP_TRY(fr.reserve(c->h_stage_out, c->d_gl_z));
  char* stream = (char*)c->d_gl_z.ptr + fr.total();
  HIP_TRY(io.stage(c->h_stage_in, c->d_sw_out, c->stream));  // (the lengths have come back)
  HIP_TRY(hipMemsetAsync(fr.dev<int>(r_status), 0, 16, c->stream));
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  hipLaunchKernelGGL(bam_write_kernel, grid, dim3(64), 0, c->stream, B, n_lines, io.dev<long long>(i_off), stream, fr.dev<int>(r_status));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(launch_bgzf_frame(c->stream, (const uint8_t*)stream, (long long)S, P, blocks, fr.dev<uint8_t>(r_out)));
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(fr.fetch(c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  (void)hipEventElapsedTime(&ms, c->ev[6], c->ev[7]);
  times[1] = ms;
  (void)hipEventElapsedTime(&ms, c->ev[7], c->ev[0]);
  times[2] = ms;
  if (*fr.host<int>(r_status)) return fail(BPSW_ERR_DEVICE, w + ": a record's bytes differ in number from its length (bam_rec_write's status)");
  memcpy(out, fr.host<char>(r_out), total);
  times[4] = wall_ms() - t1;
  return BPSW_OK;
}

int bam_deflate_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& sl,
                          char* out, size_t cap, int64_t* out_off, size_t* total_out, double times[5]) {
  return bam_device(true, c, who, bns, t, g, sl, out, cap, out_off, total_out, times);
}

}  // namespace

// ---- the blocks of a stream that lies on the device: what the writers above run behind their records, and bpsw_bam_sort.hip behind its
// sorted stream (the declarations and what they promise: bpsw_internal.h)
int bpsw::bam_payload_bytes() {
  const int p = g_payload.load(std::memory_order_relaxed);
  return p > 0 ? p : bc::kBgzfMaxPayload;
}
size_t bpsw::bgzf_framed_size(size_t S, int P) { return S + (size_t)bc::kBgzfAround * ((S + (size_t)P - 1) / (size_t)P); }
size_t bpsw::bgzf_deflate_stride(int P) { return ((size_t)P + bc::kBgzfAround + 15) & ~(size_t)15; }

hipError_t bpsw::launch_bgzf_frame(hipStream_t s, const uint8_t* d_stream, long long S, int P, size_t blocks, uint8_t* d_out) {
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(bgzf_frame_kernel, dim3((unsigned)blocks), dim3(64), 0, s, d_stream, S, P, d_out);
  return hipGetLastError();
}
hipError_t bpsw::launch_bgzf_deflate(hipStream_t s, const uint8_t* d_stream, long long S, int P, size_t blocks, uint16_t* d_tok, uint8_t* d_wide,
                                     uint32_t* d_sizes) {
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)blocks), dim3(64), 0, s, d_stream, S, P, d_tok, d_wide, (long long)bgzf_deflate_stride(P),
                     d_sizes);
  return hipGetLastError();
}
bool bpsw::bgzf_block_offsets(const uint32_t* sizes, size_t S, int P, size_t blocks, std::vector<long long>* off) {
  off->assign(blocks + 1, 0);
  for (size_t b = 0; b < blocks; ++b) {
    const size_t n = std::min(S - b * (size_t)P, (size_t)P);
    if (sizes[b] < 28 || sizes[b] > n + bc::kBgzfAround) return false;
    (*off)[b + 1] = (*off)[b] + sizes[b];
  }
  return true;
}
hipError_t bpsw::launch_bgzf_pack(hipStream_t s, const uint8_t* d_wide, int P, const long long* d_off, size_t blocks, uint8_t* d_out) {
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)blocks), dim3(64), 0, s, d_wide, (long long)bgzf_deflate_stride(P), d_off, d_out);
  return hipGetLastError();
}

int bpsw::bam_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& sl,
                        char* out, size_t cap, int64_t* out_off, size_t* total_out, double times[5]) {
  return bam_device(false, c, who, bns, t, g, sl, out, cap, out_off, total_out, times);
}

extern "C" {

int bpsw_bam_se_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g, int flags, char* out,
                      size_t cap, size_t* out_needed, bpsw_alnreg_t* out_regs) {
  if (c && topt && g && (flags & ~BPSW_BAM_DEFLATE)) return fail(BPSW_ERR_ARG, "bam_se: unknown flag");  // (after the null checks)
  memset(t_deflate, 0, sizeof t_deflate);
  SamCall m;
  m.on_device = (flags & BPSW_BAM_DEFLATE) ? bam_deflate_on_device : bam_on_device;
  m.times = t_bam; m.n_times = 5;
  return sam_batch(c, opt, topt, g, nullptr, m, out, cap, own_offsets(g ? g->n_reads : 0), out_needed, out_regs);
}

int bpsw_bam_pe_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, int flags, char* out, size_t cap,
                      size_t* out_needed, bpsw_alnreg_t* out_regs) {
  if (c && topt && g && (flags & ~BPSW_BAM_DEFLATE)) return fail(BPSW_ERR_ARG, "bam_pe: unknown flag");
  memset(t_deflate, 0, sizeof t_deflate);
  SamCall m;
  m.paired = true;
  m.on_device = (flags & BPSW_BAM_DEFLATE) ? bam_deflate_on_device : bam_on_device;
  m.times = t_bam; m.n_times = 5;
  return sam_batch(c, opt, topt, nullptr, g, m, out, cap, own_offsets(g ? 2ll * g->group_size : 0), out_needed, out_regs);
}

int bpsw_align_bam_se_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt,
                            const bpsw_se_reads_t* g, int zdrop_mode, int w1_flags, int flags, char* out, size_t cap, size_t* out_needed) {
  if (c && opt && sopt && topt && g && (flags & ~BPSW_BAM_DEFLATE)) return fail(BPSW_ERR_ARG, "align_bam_se: unknown flag");
  int64_t none[1];
  return align_se(c, opt, sopt, topt, g, zdrop_mode, w1_flags, flags, se_tail, out, cap, none, out_needed);
}

int bpsw_align_bam_pe_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g,
                            const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out, size_t cap,
                            size_t* out_needed, bpsw_pestat_t* out_pes) {
  if (c && opt && sopt && topt && g && (flags & ~BPSW_BAM_DEFLATE)) return fail(BPSW_ERR_ARG, "align_bam_pe: unknown flag");
  int64_t none[1];
  return align_pe(c, opt, sopt, topt, g, pes0, zdrop_mode, w1_flags, rescue_mode, flags, pe_tail, out, cap, none, out_needed, out_pes);
}

int bpsw_sam_header_ex(bpsw_ctx_t* c, int32_t n_seqs, const int32_t* len, const char* names, const char* extra, size_t extra_bytes, int flags,
                       char* out, size_t cap, size_t* out_needed) {
  if (flags & ~BPSW_HDR_COORDINATE) return fail(BPSW_ERR_ARG, "sam_header: unknown flag");
  Contigs t;
  const int rc = contigs_of("sam_header", c, n_seqs, len, names, &t);
  if (rc != BPSW_OK) return rc;
  const std::string s = header_text(t, extra, extra_bytes, flags);
  return hand_out("sam_header", s.data(), s.size(), out, cap, out_needed);
}

int bpsw_sam_header(bpsw_ctx_t* c, int32_t n_seqs, const int32_t* len, const char* names, const char* extra, size_t extra_bytes, char* out,
                    size_t cap, size_t* out_needed) {
  return bpsw_sam_header_ex(c, n_seqs, len, names, extra, extra_bytes, 0, out, cap, out_needed);
}

int bpsw_bam_header_ex(bpsw_ctx_t* c, int32_t n_seqs, const int32_t* len, const char* names, const char* extra, size_t extra_bytes, int flags,
                       char* out, size_t cap, size_t* out_needed) {
  if (flags & ~BPSW_HDR_COORDINATE) return fail(BPSW_ERR_ARG, "bam_header: unknown flag");
  Contigs t;
  const int rc = contigs_of("bam_header", c, n_seqs, len, names, &t);
  if (rc != BPSW_OK) return rc;
  const std::string text = header_text(t, extra, extra_bytes, flags);
  if (text.size() > 0x7fffffffull) return fail(BPSW_ERR_LIMIT, "bam_header: a header text of 2^31 bytes or more");
  std::string s("BAM\1", 4);
  append_u32(s, (uint32_t)text.size());
  s += text;
  append_u32(s, (uint32_t)t.name.size());
  for (size_t k = 0; k < t.name.size(); ++k) {
    append_u32(s, (uint32_t)t.name[k].size() + 1);
    s.append(t.name[k].c_str(), t.name[k].size() + 1);
    append_u32(s, (uint32_t)t.len[k]);
  }
  const int P = bam_payload_bytes();
  const size_t total = bgzf_framed_size(s.size(), P);
  if (out_needed) *out_needed = total;
  if (!out || total > cap) return fail(BPSW_ERR_CAPACITY, "bam_header: buffer too small (see *out_needed)");
  frame_host(s, P, out);
  return BPSW_OK;
}

int bpsw_bam_header(bpsw_ctx_t* c, int32_t n_seqs, const int32_t* len, const char* names, const char* extra, size_t extra_bytes, char* out,
                    size_t cap, size_t* out_needed) {
  return bpsw_bam_header_ex(c, n_seqs, len, names, extra, extra_bytes, 0, out, cap, out_needed);
}

int bpsw_bam_eof(char* out, size_t cap, size_t* out_needed) {
  // the empty block of the specification (4.1.2): a gzip member whose deflate stream is the empty fixed block 03 00
  static const unsigned char eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                                        0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};
  return hand_out("bam_eof", (const char*)eof, sizeof eof, out, cap, out_needed);
}

int bpsw_bam_set_block_payload(int bytes) {
  if (bytes < 0 || bytes > bc::kBgzfMaxPayload) return fail(BPSW_ERR_ARG, "bam_set_block_payload: 1 .. 65280 bytes, or 0 for the default");
  g_payload.store(bytes, std::memory_order_relaxed);
  return BPSW_OK;
}

void bpsw_last_bam_times(double ms[5]) {
  if (ms) memcpy(ms, t_bam, sizeof t_bam);
}

void bpsw_last_bam_deflate_times(double ms[4]) {
  if (ms) memcpy(ms, t_deflate, sizeof t_deflate);
}

}  // extern "C"
