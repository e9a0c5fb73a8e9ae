// bpsw_index.hip -- the FM-index built on the device from the 2-bit reference: bpsw_fmi_build and its diagnostics.
//
// The rules -- the text, the keys, the flags, the new ranks, the packing -- are bpsw_index_core.h's; this file is who applies them, one
// item per lane.  The construction is prefix doubling over a radix sort, and only unresolved suffixes stay in play:
//   index_first_key_kernel   round 0's list: every suffix with its first key
//   index_round_key_kernel   a later round's list: key = group << rank_bits | rank[suffix + h], gathered before any rank is written
//   the sort                 stable LSD radix sort of (key, suffix), eight bits a pass, only as many passes as the keys have bits
//                            (radix_sort_pairs, declared in bpsw_internal.h: bpsw_bam_sort.hip sorts its records with it too):
//     sort_hist_kernel         one workgroup per tile of 4 096: the tile's digit counts -> table[digit * tiles + tile]
//     scan_exclusive_i64       (bpsw_scan.hip) over the whole table: where every tile's every digit begins
//     sort_scatter_kernel      one workgroup per tile, 256 entries a step in list order: a lane's place is its digit's base, plus the
//                              entries of that digit in the wavefronts before its own (LDS), plus those in the lanes before it (eight
//                              64-bit ballots); the bases move on after every step.  2 KiB + 4 KiB of LDS, four wavefronts.
//   index_flags_kernel       run heads, group heads, keep -> three columns; scan_exclusive_i64 sums them
//   index_heads_kernel       the list position of every run's and group's head
//   index_assign_kernel      new ranks; runs of one to the suffix array, the rest compacted into the next list
//   index_bwt_words_kernel, index_block_counts_kernel, scan_exclusive_i64 (four columns), index_pack_kernel, index_sample_kernel
// The host reads one number a round: the length of the next list.
#include <string.h>

#include <atomic>
#include <string>
#include <utility>

#include "bpsw_internal.h"
#include "bpsw_index_core.h"

using namespace bpsw;
namespace xc = bpsw::idxcore;
using xc::i64;
using xc::u64;

namespace {

constexpr int kThreads = 256;
inline unsigned grid_for(i64 n) { return (unsigned)((n + kThreads - 1) / kThreads); }

__global__ __launch_bounds__(kThreads) void index_first_key_kernel(xc::Text T, i64 N, int k0, u64* __restrict__ K, i64* __restrict__ V) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  K[i] = xc::first_key(T, i, k0);
  V[i] = i;
}

__global__ __launch_bounds__(kThreads) void index_round_key_kernel(const i64* __restrict__ rank, i64 seq_len, const i64* __restrict__ suffix,
                                                                   const i64* __restrict__ group, i64 M, i64 h, int rank_bits,
                                                                   u64* __restrict__ K, i64* __restrict__ V) {
  const i64 m = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const i64 s = suffix[m];
  K[m] = xc::round_key(rank, seq_len, s, group[m], h, rank_bits);
  V[m] = s;
}

__global__ __launch_bounds__(xc::kSortThreads) void sort_hist_kernel(const u64* __restrict__ K, i64 M, int shift, i64 tiles, i64* __restrict__ table) {
  __shared__ int cnt[xc::kRadix];
  const int t = (int)threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  const i64 lo = (i64)blockIdx.x * xc::kSortTile, hi = lo + xc::kSortTile < M ? lo + xc::kSortTile : M;
  for (i64 i = lo + t; i < hi; i += xc::kSortThreads) atomicAdd(&cnt[xc::digit_of(K[i], shift)], 1);
  __syncthreads();
  table[(i64)t * tiles + blockIdx.x] = cnt[t];
}

__global__ __launch_bounds__(xc::kSortThreads) void sort_scatter_kernel(const u64* __restrict__ K, const i64* __restrict__ V, i64 M, int shift, i64 tiles,
                                                                        const i64* __restrict__ table, u64* __restrict__ Ko, i64* __restrict__ Vo) {
  __shared__ i64 base[xc::kRadix];
  __shared__ int wcnt[xc::kSortWaves][xc::kRadix];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  base[t] = table[(i64)t * tiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < xc::kSortWaves; ++w) wcnt[w][t] = 0;
  __syncthreads();
  const i64 lo = (i64)blockIdx.x * xc::kSortTile, hi = lo + xc::kSortTile < M ? lo + xc::kSortTile : M;
  for (i64 i0 = lo; i0 < hi; i0 += xc::kSortThreads) {  // (the trip count is the workgroup's: every barrier is met by all)
    const i64 i = i0 + t;
    const bool valid = i < hi;
    const u64 key = valid ? K[i] : 0;
    const int d = xc::digit_of(key, shift);
    u64 same = __ballot(valid);  // the valid lanes of this wavefront with the same digit
#pragma unroll
    for (int b = 0; b < xc::kRadixBits; ++b) {
      const u64 bb = __ballot((d >> b) & 1);
      same &= ((d >> b) & 1) ? bb : ~bb;
    }
    const u64 before = same & ((1ull << lane) - 1);
    if (valid && before == 0) wcnt[wave][d] = __popcll(same);
    __syncthreads();
    if (valid) {
      i64 pos = base[d] + __popcll(before);
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      Ko[pos] = key;
      Vo[pos] = V[i];
    }
    __syncthreads();
    int step = 0;
#pragma unroll
    for (int w = 0; w < xc::kSortWaves; ++w) { step += wcnt[w][t]; wcnt[w][t] = 0; }
    base[t] += step;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void index_flags_kernel(const u64* __restrict__ K, i64 M, int group_shift, i64* __restrict__ cols) {
  const i64 m = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (m < M) xc::flags_write(K, M, m, group_shift, cols);
}
__global__ __launch_bounds__(kThreads) void index_heads_kernel(const u64* __restrict__ K, i64 M, int group_shift, const i64* __restrict__ cols,
                                                               i64* __restrict__ run_pos, i64* __restrict__ group_pos) {
  const i64 m = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (m < M) xc::heads_write(K, M, m, group_shift, cols, run_pos, group_pos);
}
__global__ __launch_bounds__(kThreads) void index_assign_kernel(const u64* __restrict__ K, const i64* __restrict__ V, i64 M, int group_shift,
                                                                const i64* __restrict__ cols, const i64* __restrict__ run_pos,
                                                                const i64* __restrict__ group_pos, i64* __restrict__ rank, i64* __restrict__ sa,
                                                                i64* __restrict__ next_suffix, i64* __restrict__ next_group) {
  const i64 m = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (m < M) xc::assign_at(K, V, M, m, group_shift, cols, run_pos, group_pos, rank, sa, next_suffix, next_group);
}

__global__ __launch_bounds__(kThreads) void index_bwt_words_kernel(xc::Text T, const i64* __restrict__ sa, i64 primary, i64 n_words,
                                                                   uint32_t* __restrict__ words) {
  const i64 w = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (w < n_words) words[w] = xc::bwt_word(T, sa, primary, w);
}
__global__ __launch_bounds__(kThreads) void index_block_counts_kernel(const uint32_t* __restrict__ words, xc::Shape S, i64* __restrict__ cols) {
  const i64 b = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (b < S.n_blocks) xc::block_counts(words, S, b, cols);
}
__global__ __launch_bounds__(kThreads) void index_pack_kernel(const uint32_t* __restrict__ words, xc::Shape S, const i64* __restrict__ cols,
                                                              uint32_t* __restrict__ out) {
  const i64 b = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (b <= S.n_blocks) xc::pack_block(words, S, b, cols, out);
}
__global__ __launch_bounds__(kThreads) void index_sample_kernel(const i64* __restrict__ sa, i64 n_sa, i64 sa_intv, i64* __restrict__ out) {
  const i64 k = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (k < n_sa) out[k] = xc::sample_at(sa, k, sa_intv);
}

// ---- the working set: one block of device memory, laid out from the number of suffixes alone ------------------------------------------
struct Arena {
  size_t rank, sa, key[2], val[2], cols, run_pos, group_pos, next_suffix, next_group, table, sums, total;
};
Arena arena_of(i64 N, int scan_tile) {
  StageLayout L;
  Arena A;
  const size_t n8 = 8 * (size_t)N;
  const i64 tiles = (N + xc::kSortTile - 1) / xc::kSortTile, table_n = tiles * xc::kRadix;
  const i64 widest = table_n > N ? table_n : N;  // the longest column any scan of the build gets
  A.rank = L.add(n8); A.sa = L.add(n8);
  for (int k = 0; k < 2; ++k) { A.key[k] = L.add(n8); A.val[k] = L.add(n8); }
  const size_t list_cols = 3 * ((size_t)N + 1), count_cols = 4 * ((size_t)((N + 126) / 128) + 1);
  A.cols = L.add(8 * (list_cols > count_cols ? list_cols : count_cols));  // three columns of a list, or the four of the block counts
  A.run_pos = L.add(n8); A.group_pos = L.add(n8);
  A.next_suffix = L.add(n8); A.next_group = L.add(n8);
  A.table = L.add(8 * ((size_t)table_n + 1));
  A.sums = L.add(8 * 4 * (size_t)scan_tiles(widest, scan_tile));
  A.total = L.total();
  return A;
}

std::atomic<int> g_first_key{0};
std::atomic<long long> g_budget{0};
thread_local double t_times[5] = {0., 0., 0., 0., 0.};
thread_local int64_t t_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// (K, V)[from] sorted by the low `bits` of the keys; -> the buffer the sorted list is in
int sort_list(hipStream_t s, uint8_t* D, const Arena& A, int from, i64 M, int bits, int scan_tile, hipError_t* err) {
  u64* key[2] = {(u64*)(D + A.key[0]), (u64*)(D + A.key[1])};
  i64* val[2] = {(i64*)(D + A.val[0]), (i64*)(D + A.val[1])};
  int passes = 0;
  const int at = radix_sort_pairs(s, key, val, from, M, bits, (i64*)(D + A.table), scan_tile, (i64*)(D + A.sums), &passes, err);
  t_stats[3] += passes;
  return at;
}

int shape_fill(int64_t l_pac, int32_t sa_intv, bpsw_fmi_shape_t* out) {
  memset(out, 0, sizeof *out);
  if (l_pac < 1) return fail(BPSW_ERR_ARG, "fmi_build: l_pac below 1");
  if (sa_intv < 1 || (sa_intv & (sa_intv - 1))) return fail(BPSW_ERR_ARG, "fmi_build: sa_intv is not a power of two");
  if (l_pac > (int64_t)1 << 40) return fail(BPSW_ERR_LIMIT, "fmi_build: reference longer than 2^40 bases");
  const xc::Shape S = xc::shape_of(l_pac, sa_intv);
  out->seq_len = S.seq_len; out->bwt_size = S.bwt_size; out->n_sa = S.n_sa; out->sa_intv = sa_intv;
  return BPSW_OK;
}

}  // namespace

int bpsw::sort_tile_items() { return xc::kSortTile; }

int bpsw::radix_sort_pairs(hipStream_t s, unsigned long long* const key[2], long long* const val[2], int from, long long M, int bits,
                           long long* table, int scan_tile, long long* sums, int* passes, hipError_t* err) {
  const i64 tiles = (M + xc::kSortTile - 1) / xc::kSortTile;
  int at = from;
  *err = hipSuccess;
  *passes = 0;
  for (int p = 0; p < xc::radix_passes(bits) && M > 1; ++p, at ^= 1) {
    const u64* K = key[at];
    const i64* V = val[at];
    hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)tiles), dim3(xc::kSortThreads), 0, s, K, M, p * xc::kRadixBits, tiles, table);
    if ((*err = hipGetLastError()) != hipSuccess) return at;
    if ((*err = scan_exclusive_i64(s, table, 1, tiles * xc::kRadix, scan_tile, sums)) != hipSuccess) return at;
    hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)tiles), dim3(xc::kSortThreads), 0, s, K, V, M, p * xc::kRadixBits, tiles,
                       (const i64*)table, key[at ^ 1], val[at ^ 1]);
    if ((*err = hipGetLastError()) != hipSuccess) return at;
    ++*passes;
  }
  return at;
}

extern "C" {

int bpsw_fmi_build_shape(int64_t l_pac, int32_t sa_intv, bpsw_fmi_shape_t* shape) {
  if (!shape) return fail(BPSW_ERR_ARG, "fmi_build_shape: null shape");
  return shape_fill(l_pac, sa_intv, shape);
}

int bpsw_fmi_build(bpsw_ctx_t* c, const uint8_t* pac, int64_t l_pac, int32_t sa_intv, int flags, uint32_t* bwt, int64_t bwt_cap, int64_t* sa,
                   int64_t sa_cap, bpsw_fmi_shape_t* out) {
  if (!c || !pac || !out) return fail(BPSW_ERR_ARG, "fmi_build: null argument");
  int rc = shape_fill(l_pac, sa_intv, out);
  if (rc != BPSW_OK) return rc;
  if (flags & ~(BPSW_FMI_BUILD_LOAD | BPSW_FMI_BUILD_REF)) return fail(BPSW_ERR_ARG, "fmi_build: unknown flag");
  const bool load = (flags & BPSW_FMI_BUILD_LOAD) != 0;
  if (!load && (!bwt || !sa)) return fail(BPSW_ERR_ARG, "fmi_build: bwt or sa is null and BPSW_FMI_BUILD_LOAD is not set");
  if ((bwt && bwt_cap < out->bwt_size) || (sa && sa_cap < out->n_sa))
    return fail(BPSW_ERR_CAPACITY, "fmi_build: bwt_cap or sa_cap below the index's size (out->bwt_size, out->n_sa)");
  const xc::Shape S = xc::shape_of(l_pac, sa_intv);
  const i64 seq_len = S.seq_len, N = seq_len + 1;
  const int rank_bits = xc::bits_for((u64)(N - 1));
  if (2 * rank_bits > 64) return fail(BPSW_ERR_LIMIT, "fmi_build: more than 2^32 suffixes (a group and a rank no longer fit one 64-bit key)");

  const double t0 = wall_ms();
  for (double& t : t_times) t = 0.;
  for (int64_t& v : t_stats) v = 0;
  int k0 = g_first_key.load(std::memory_order_relaxed);
  if (k0 < 1 || k0 > xc::kMaxFirstKey) k0 = xc::kMaxFirstKey;
  const int scan_tile = scan_tile_items();
  const Arena A = arena_of(N, scan_tile);
  const size_t pac_bytes = (size_t)((l_pac + 3) >> 2), bwt_bytes = 4 * (size_t)S.bwt_size, sa_bytes = 8 * (size_t)S.n_sa;
  const size_t need = A.total + (pac_bytes + 16) + (bwt_bytes + 64) + sa_bytes;
  t_stats[4] = xc::kSortTile; t_stats[5] = (int64_t)need; t_stats[6] = k0;

  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  size_t avail = 0, dev_total = 0;
  const long long pretend = g_budget.load(std::memory_order_relaxed);
  if (pretend > 0) avail = (size_t)pretend;
  else HIP_TRY(hipMemGetInfo(&avail, &dev_total));
  if (need > avail)
    return fail(BPSW_ERR_LIMIT, "fmi_build: the working set of " + std::to_string(need) + " bytes (" + std::to_string(N) +
                                    " suffixes) does not fit the " + std::to_string(avail) + " bytes available");

  // exact-size blocks of their own (a DeviceBuffer rounds up to a power of two): freed, or handed over, before the call returns
  struct Block {
    DeviceBuffer b;
    hipError_t get(size_t bytes) { const hipError_t e = hipMalloc(&b.ptr, bytes); if (e == hipSuccess) b.cap = bytes; return e; }
    ~Block() { b.release(); }
  } work, d_pac, d_bwt, d_sa;
  HIP_TRY(work.get(A.total));
  HIP_TRY(d_pac.get(pac_bytes + 16));
  HIP_TRY(d_bwt.get(bwt_bytes + 64));  // (a whole 64-byte block may be read where the array ends inside one: bpsw_fmi_load)
  HIP_TRY(d_sa.get(sa_bytes));
  hipStream_t s = c->stream;
  uint8_t* D = (uint8_t*)work.b.ptr;
  HIP_TRY(hipMemsetAsync((uint8_t*)d_pac.b.ptr + pac_bytes, 0, 16, s));
  HIP_TRY(hipMemsetAsync((uint8_t*)d_bwt.b.ptr + bwt_bytes, 0, 64, s));
  HIP_TRY(hipMemcpyAsync(d_pac.b.ptr, pac, pac_bytes, hipMemcpyHostToDevice, s));
  const xc::Text T{(const uint8_t*)d_pac.b.ptr, l_pac};
  i64 *rank = (i64*)(D + A.rank), *full_sa = (i64*)(D + A.sa), *cols = (i64*)(D + A.cols), *run_pos = (i64*)(D + A.run_pos),
      *group_pos = (i64*)(D + A.group_pos), *next_suffix = (i64*)(D + A.next_suffix), *next_group = (i64*)(D + A.next_group),
      *sums = (i64*)(D + A.sums);

  // ---- round 0 on the first keys, then the doubling rounds on what is left -----------------------------------------------------------
  i64 M = N, h = k0;
  for (int round = 0; M > 0; ++round) {
    const int bits = round == 0 ? xc::first_key_bits(k0) : 2 * rank_bits, group_shift = round == 0 ? 64 : rank_bits;
    if (round == 0) hipLaunchKernelGGL(index_first_key_kernel, dim3(grid_for(M)), dim3(kThreads), 0, s, T, M, k0, (u64*)(D + A.key[0]), (i64*)(D + A.val[0]));
    else hipLaunchKernelGGL(index_round_key_kernel, dim3(grid_for(M)), dim3(kThreads), 0, s, (const i64*)rank, seq_len, (const i64*)next_suffix,
                            (const i64*)next_group, M, h, rank_bits, (u64*)(D + A.key[0]), (i64*)(D + A.val[0]));
    HIP_TRY(hipGetLastError());
    hipError_t e = hipSuccess;
    const int at = sort_list(s, D, A, 0, M, bits, scan_tile, &e);
    HIP_TRY(e);
    const u64* K = (const u64*)(D + A.key[at]);
    const i64* V = (const i64*)(D + A.val[at]);
    hipLaunchKernelGGL(index_flags_kernel, dim3(grid_for(M)), dim3(kThreads), 0, s, K, M, group_shift, cols);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_exclusive_i64(s, cols, 3, M, scan_tile, sums));
    hipLaunchKernelGGL(index_heads_kernel, dim3(grid_for(M)), dim3(kThreads), 0, s, K, M, group_shift, (const i64*)cols, run_pos, group_pos);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(index_assign_kernel, dim3(grid_for(M)), dim3(kThreads), 0, s, K, V, M, group_shift, (const i64*)cols, (const i64*)run_pos,
                       (const i64*)group_pos, rank, full_sa, next_suffix, next_group);
    HIP_TRY(hipGetLastError());
    i64 left = 0;
    HIP_TRY(hipMemcpyAsync(&left, cols + 2 * (M + 1) + M, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (left < 0 || left > M || left == 1) return fail(BPSW_ERR_DEVICE, "fmi_build: a round left a list of impossible length");
    if (round == 0) { t_stats[1] = left; t_times[0] = wall_ms() - t0; }
    else { ++t_stats[0]; h *= 2; }
    if (left > t_stats[2]) t_stats[2] = left;
    if (round > 0 && h > 2 * N) return fail(BPSW_ERR_DEVICE, "fmi_build: the rounds did not come to an end");
    M = left;
  }
  t_times[1] = wall_ms() - t0 - t_times[0];

  // ---- the index from the suffix array ---------------------------------------------------------------------------------------------------
  i64 primary = 0;
  HIP_TRY(hipMemcpyAsync(&primary, rank, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (primary < 1 || primary > seq_len) return fail(BPSW_ERR_DEVICE, "fmi_build: the whole text's row is outside the suffix array");
  uint32_t* words = (uint32_t*)(D + A.key[0]);  // (the lists are done with)
  hipLaunchKernelGGL(index_bwt_words_kernel, dim3(grid_for(S.n_words)), dim3(kThreads), 0, s, T, (const i64*)full_sa, primary, S.n_words, words);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(index_block_counts_kernel, dim3(grid_for(S.n_blocks)), dim3(kThreads), 0, s, (const uint32_t*)words, S, cols);
  HIP_TRY(hipGetLastError());
  HIP_TRY(scan_exclusive_i64(s, cols, 4, S.n_blocks, scan_tile, sums));
  hipLaunchKernelGGL(index_pack_kernel, dim3(grid_for(S.n_blocks + 1)), dim3(kThreads), 0, s, (const uint32_t*)words, S, (const i64*)cols,
                     (uint32_t*)d_bwt.b.ptr);
  HIP_TRY(hipGetLastError());
  i64 occ[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(&occ[k], cols + (i64)k * (S.n_blocks + 1) + S.n_blocks, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  t_times[2] = wall_ms() - t0 - t_times[0] - t_times[1];
  hipLaunchKernelGGL(index_sample_kernel, dim3(grid_for(S.n_sa)), dim3(kThreads), 0, s, (const i64*)full_sa, S.n_sa, (i64)sa_intv, (i64*)d_sa.b.ptr);
  HIP_TRY(hipGetLastError());
  if (bwt) HIP_TRY(hipMemcpyAsync(bwt, d_bwt.b.ptr, bwt_bytes, hipMemcpyDeviceToHost, s));
  if (sa) HIP_TRY(hipMemcpyAsync(sa, d_sa.b.ptr, sa_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  long long L2[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) L2[k + 1] = L2[k] + occ[k];
  if (L2[4] != seq_len) return fail(BPSW_ERR_DEVICE, "fmi_build: the base counts do not add up to seq_len");
  work.b.release();
  if (load) {
    rc = fmi_adopt(c, &d_bwt.b, &d_sa.b, primary, L2, seq_len, sa_intv);
    if (rc != BPSW_OK) return rc;
  }
  if (flags & BPSW_FMI_BUILD_REF) {
    DeviceRef& r = device_ref(c->device);
    RefWriteHold wr(&r.gate);
    std::lock_guard<std::mutex> gr(r.mu);
    RingPause ring_paused(c->device);
    HIP_TRY(hipDeviceSynchronize());  // nothing in flight may still read the previous reference
    std::swap(r.buf, d_pac.b);
    r.l_pac = l_pac;
  }
  out->primary = primary;
  for (int k = 0; k < 5; ++k) out->L2[k] = L2[k];
  t_times[3] = wall_ms() - t0 - t_times[0] - t_times[1] - t_times[2];
  t_times[4] = wall_ms() - t0;
  return BPSW_OK;
}

void bpsw_last_fmi_build_times(double ms[5]) {
  if (ms) memcpy(ms, t_times, sizeof t_times);
}
void bpsw_last_fmi_build_stats(int64_t st[8]) {
  if (st) memcpy(st, t_stats, sizeof t_stats);
}
void bpsw_fmi_build_set_first_key(int bases) {
  g_first_key.store(bases < 1 ? 0 : bases > xc::kMaxFirstKey ? xc::kMaxFirstKey : bases, std::memory_order_relaxed);
}
void bpsw_fmi_build_set_budget(int64_t bytes) { g_budget.store(bytes > 0 ? bytes : 0, std::memory_order_relaxed); }

}  // extern "C"
