// bpsw_chain_dev.hip -- worker1's chaining and chain filtering on the device: bpsw_chain_batch, and the chain stage of
// bpsw_worker1_batch with BPSW_W1_CHAIN_DEVICE.
//
// Replaces, for a batch, what bpsw_chain_seeds (bpsw_chain.cpp) does read by read on the calling thread: the tree side of
// mem_insert_seed + mem_chain (native/bwamem.c:185-304) and mem_chain_flt (:310-379).  The algorithm is bpsw_chain_core.h, the same
// text the host test compiles; integer and two float comparisons, bit-exact.
//
// Mapping: ONE READ PER LANE (chain_kernel).  A read's chaining is a serial row of dependent insertions into its own B-tree, as
// the SMEM search of seed_smem_kernel is a row of dependent index reads, and a batch has tens of thousands of reads; nothing of a
// read is shared with another.  Reads are dealt to lanes in descending order of their seed count, so that the lanes of a wave have
// about the same work and finish together.  Each read has its slice of one arena (the context's d_chain): 16 bytes of counts,
// then the workspace bpsw_chain_core.h lays out, 52 m + 256 (m / 7 + 2) + 896 bytes for m seeds.  The kernel indexes no array of
// its own, so it has no scratch.
//
// Two passes: chain_kernel leaves a read's chains in its slice and reports (chains, seeds in them); the host sums these to
// offsets; chain_emit_kernel writes seed counts and seeds of the kept chains, one read per lane again, into one block that comes
// back.  What the filter dropped never crosses the bus.
//
// The arena has a byte budget (256 MB; bpsw_chain_set_arena_budget): a batch runs in slices of reads that fit it, a single read
// larger than the budget grows the arena to that read.  Reads of more than BPSW_CHAIN_DEV_MAX_SEEDS seeds (default 128, 0 = no
// limit; read once) are chained by bpsw_chain_seeds on the calling thread while the first slice's kernel runs: one lane's
// insertions are dependent round trips to HBM, 25-40 us a seed where a CPU core in its cache takes 0.2 (up to 128
// seeds a read the kernel costs a batch no more than the calling thread does, at 512 it costs 11 ms more).
//
// RESIDENT CHAINS (chain_dev_run with a ChainTablesDev: BPSW_W1_CHAINS_RESIDENT, BPSW_CHAIN_TABLES_DEVICE).  Nothing of the chains
// comes back; the stage leaves on the device, in read order, the tables chain2aln_kernel indexes.  All of it lies in one buffer of
// the context (d_chain_tab), laid out once per batch from the two numbers the host has, n reads and S = seed_beg[n] seeds (a bound for
// the kept chains and for their seeds):
//   pool_cnt[S] pool_seeds[S]     the kept chains in the order the slices wrote them
//   where[n]                      per read: its place in both pools, its chains, its seeds (ChainWhere, bpsw_chain_tables_core.h)
//   read_cols[2 (n + 1)]          the same two counts as 64-bit columns, scanned in read order after the last slice
//   slice_cols[2 (ns + 1)]        the (chains, seeds) columns of the running slice's items, scanned per slice
//   tile sums of both scans, the slice's record, the totals
//   chain_cnt[n] chain_base[n] reg_base[n] seed_cnt[S] seed_base[S] seed_rbeg[S] seed_qbeg[S] seed_len[S]     the tables
// Per slice: chain_kernel also writes slice_cols; scan_exclusive_i64 (bpsw_scan.hip) sums them; chain_emit_resident_kernel writes
// the slice's chains into the pools at the running base plus the scanned offset, where[] and read_cols[] of its reads, and one
// record {error word, chains, seeds} -- the 32 bytes a slice fetches.  The chains of the calling thread's reads are staged and
// copied into the pools behind the last slice's, with their where[] entries (chain_host_merge_kernel).  Then one scan over
// read_cols and chain_tables_kernel, one read per lane (arithmetic in bpsw_chain_tables_core.h); 32 bytes of totals come back.
// Every kernel gets what it needs of the others from the launch before it on the stream: none waits for another workgroup.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>

#include "bpsw_internal.h"
#include "bpsw_chain_core.h"
#include "bpsw_chain_tables_core.h"

using namespace bpsw;
namespace cc = bpsw::chaincore;

namespace {

struct ChainArgs {  // by value to the kernels; the item pointers start at the launch's first item
  bpsw_seed_opt_t so;
  int w, filter, drop_bridging, n_items;
  long long l_pac;
  const int32_t* item_read;     // the read of item i
  const long long* item_work;   // where item i's slice begins in the arena
  const long long* seed_beg;    // n_reads + 1: read r's seeds are seeds[seed_beg[r] .. seed_beg[r + 1])
  const bpsw_seed_t* seeds;
  uint8_t* arena;
};
struct ItemCounts {  // the head of a read's slice, and what chain_kernel reports per item
  int32_t chains, seeds, tree_chains, pad_;
};
constexpr size_t kSliceHead = 16;
static_assert(sizeof(ItemCounts) == kSliceHead, "the head of a slice");

// cols (resident chains only, else null): the slice's two columns, chains of item i at cols[i], its seeds at cols[n_items + 1 + i]
__global__ __launch_bounds__(64) void chain_kernel(ChainArgs A, ItemCounts* __restrict__ counts, int* error, long long* __restrict__ cols) {
  const int it = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (it >= A.n_items) return;
  const int r = A.item_read[it];
  const long long s0 = A.seed_beg[r];
  const int m = (int)(A.seed_beg[r + 1] - s0);
  uint8_t* mine = A.arena + A.item_work[it];
  const cc::Work W = cc::work_carve(mine + kSliceHead, m, cc::node_bound(m));
  ItemCounts ic = {0, 0, 0, 0};
  const int nc = cc::chain_read(A.so, A.w, A.l_pac, m, A.seeds + s0, A.filter, A.drop_bridging, W, &ic.tree_chains, &ic.seeds);
  if (nc < 0) {
    atomicMax(error, -nc);
    ic.seeds = ic.tree_chains = 0;
  } else {
    ic.chains = nc;
  }
  *(ItemCounts*)mine = ic;
  counts[it] = ic;
  if (cols) {
    cols[it] = ic.chains;
    cols[A.n_items + 1 + it] = ic.seeds;
  }
}

// chain_base / seed_base: per item, where its chains' seed counts and its seeds begin in the two outputs
__global__ __launch_bounds__(64) void chain_emit_kernel(ChainArgs A, const long long* __restrict__ chain_base, const long long* __restrict__ seed_base,
                                                         int32_t* out_cnt, bpsw_seed_t* out_seeds) {
  const int it = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (it >= A.n_items) return;
  const int r = A.item_read[it];
  const long long s0 = A.seed_beg[r];
  const int m = (int)(A.seed_beg[r + 1] - s0);
  uint8_t* mine = A.arena + A.item_work[it];
  const ItemCounts ic = *(const ItemCounts*)mine;
  if (ic.chains == 0) return;
  const cc::Work W = cc::work_carve(mine + kSliceHead, m, cc::node_bound(m));
  cc::chain_emit(W, cc::result_list(W, A.filter, ic.tree_chains), ic.chains, A.seeds + s0, out_cnt + chain_base[it], out_seeds + seed_base[it]);
}

// ---- resident chains ----
struct ChainPools {
  int32_t* cnt;
  bpsw_seed_t* seeds;
  ChainWhere* where;
  long long* read_cols;  // chains of read r at [r], its seeds at [n_reads + 1 + r]
  long long n_reads;
};
constexpr size_t kRecBytes = 32;  // a slice's record and the totals, four 64-bit words each: what the stage fetches

// cols: the slice's columns after the scan (item i's offsets, and in entry n_items of each column the slice's total); cnt0 / seed0:
// what earlier slices left in the pools.  rec: {error word of chain_kernel, chains, seeds, 0} of the slice.
__global__ __launch_bounds__(64) void chain_emit_resident_kernel(ChainArgs A, const long long* __restrict__ cols, long long cnt0, long long seed0,
                                                                  ChainPools P, const int* __restrict__ error, long long* __restrict__ rec) {
  const int it = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (it == 0) {
    rec[0] = *error;
    rec[1] = cols[A.n_items];
    rec[2] = cols[2 * (long long)A.n_items + 1];
    rec[3] = 0;
  }
  if (it >= A.n_items) return;
  const int r = A.item_read[it];
  const long long s0 = A.seed_beg[r];
  const int m = (int)(A.seed_beg[r + 1] - s0);
  uint8_t* mine = A.arena + A.item_work[it];
  const ItemCounts ic = *(const ItemCounts*)mine;
  const long long cb = cnt0 + cols[it], sb = seed0 + cols[A.n_items + 1 + it];
  P.where[r].cnt_at = cb; P.where[r].seed_at = sb; P.where[r].chains = ic.chains; P.where[r].seeds = ic.seeds;
  P.read_cols[r] = ic.chains;
  P.read_cols[P.n_reads + 1 + r] = ic.seeds;
  if (ic.chains == 0) return;
  const cc::Work W = cc::work_carve(mine + kSliceHead, m, cc::node_bound(m));
  cc::chain_emit(W, cc::result_list(W, A.filter, ic.tree_chains), ic.chains, A.seeds + s0, P.cnt + cb, P.seeds + sb);
}

// The chains of the reads the calling thread chained, staged as (reads, their where[] relative to the staged lists, seed counts,
// seeds): one element of each list per lane, into the pools at cnt0 / seed0.
__global__ __launch_bounds__(256) void chain_host_merge_kernel(long long n_host, const int32_t* __restrict__ reads, const ChainWhere* __restrict__ wh,
                                                                long long n_cnt, const int32_t* __restrict__ h_cnt, long long n_seeds,
                                                                const bpsw_seed_t* __restrict__ h_seeds, long long cnt0, long long seed0, ChainPools P) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_host) {
    const int r = reads[i];
    P.where[r].cnt_at = cnt0 + wh[i].cnt_at; P.where[r].seed_at = seed0 + wh[i].seed_at;
    P.where[r].chains = wh[i].chains; P.where[r].seeds = wh[i].seeds;
    P.read_cols[r] = wh[i].chains;
    P.read_cols[P.n_reads + 1 + r] = wh[i].seeds;
  }
  if (i < n_cnt) P.cnt[cnt0 + i] = h_cnt[i];
  if (i < n_seeds) {
    P.seeds[seed0 + i].rbeg = h_seeds[i].rbeg; P.seeds[seed0 + i].qbeg = h_seeds[i].qbeg; P.seeds[seed0 + i].len = h_seeds[i].len;
  }
}

// cols: read_cols after the scan.  totals: {chains, seeds, largest seed count of a chain (an int, raised by one atomic a
// wavefront), 0}, cleared before the launch.
__global__ __launch_bounds__(256) void chain_tables_kernel(ChainPools P, const long long* __restrict__ cols, ChainTablesOut T, long long* __restrict__ totals) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x, n = P.n_reads;
  int largest = 0;
  if (r < n) largest = chain_tables_read(P.where, P.cnt, P.seeds, r, cols[r], cols[n + 1 + r], T);
  if (r == 0) {
    totals[0] = cols[n];
    totals[1] = cols[2 * n + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(largest, o);
    largest = other > largest ? other : largest;
  }
  if ((threadIdx.x & 63) == 0 && largest > 0) atomicMax((int*)(totals + 2), largest);
}

constexpr long long kArenaBudgetDefault = 256ll << 20;
std::atomic<long long> g_arena_budget{0};
int dev_max_seeds() {  // BPSW_CHAIN_DEV_MAX_SEEDS, read once
  static const int v = [] {
    const char* e = getenv("BPSW_CHAIN_DEV_MAX_SEEDS");
    if (!e || !*e) return 128;
    const long x = strtol(e, nullptr, 10);
    return x < 0 ? 0 : x > 0x3fffffffl ? 0x3fffffff : (int)x;
  }();
  return v;
}
thread_local int64_t t_last[4] = {0, 0, 0, 0};
thread_local int64_t t_chain_bytes[2] = {0, 0};  // H2D, D2H of the calling thread's last chain_dev_run (bpsw_last_chain_bytes)

size_t slice_bytes(int m) { return kSliceHead + cc::work_bytes(m, cc::node_bound(m)); }

}  // namespace

namespace bpsw {

int chain_dev_run(bpsw_ctx* c, const bpsw_seed_opt_t& so, int w, int64_t l_pac, const ChainDevJob& J, ChainDevResult* R, ChainTablesDev* T) {
  const int n = J.n_reads;
  const long long* beg = J.seed_beg;
  if (R) {
    R->chain_cnt.assign((size_t)n, 0);
    R->chain_seed_cnt.clear();
    R->seeds.clear();
  }
  if (T) *T = ChainTablesDev{};
  t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
  t_chain_bytes[0] = t_chain_bytes[1] = 0;
  if (n == 0 || (beg[n] == 0 && !T)) return BPSW_OK;  // (resident: reads without any seed still get their rows of the tables)
  const int limit = dev_max_seeds();
  const long long budget_set = g_arena_budget.load(std::memory_order_relaxed);
  const size_t budget = (size_t)(budget_set > 0 ? budget_set : kArenaBudgetDefault);

  // which reads the kernel takes, in descending order of their seed count (ties in read order), and which stay on this thread
  std::vector<int32_t> item_read, host_reads;
  for (int r = 0; r < n; ++r) {
    const long long m = beg[r + 1] - beg[r];
    if (m == 0) continue;
    if (limit > 0 && m > limit) host_reads.push_back(r);
    else item_read.push_back(r);
  }
  std::stable_sort(item_read.begin(), item_read.end(), [&](int32_t a, int32_t b) { return beg[a + 1] - beg[a] > beg[b + 1] - beg[b]; });
  const size_t n_items = item_read.size();
  // slices of consecutive items that fit the budget (a slice has at least one item), each item's offset in its slice
  std::vector<long long> item_work(n_items);
  std::vector<size_t> slice_at(1, 0);
  size_t arena_bytes = 0;
  {
    size_t used = 0;
    for (size_t i = 0; i < n_items; ++i) {
      const size_t b = slice_bytes((int)(beg[item_read[i] + 1] - beg[item_read[i]]));
      if (used > 0 && used + b > budget) { slice_at.push_back(i); used = 0; }
      item_work[i] = (long long)used;
      used += b;
      if (used > arena_bytes) arena_bytes = used;
    }
    if (n_items) slice_at.push_back(n_items);
  }
  const size_t n_slices = slice_at.size() - 1;
  t_last[0] = (int64_t)n_items; t_last[1] = (int64_t)host_reads.size(); t_last[2] = (int64_t)n_slices; t_last[3] = (int64_t)arena_bytes;

  // per read: where its chains lie in the two pools below (filled slice by slice, and by the host's reads)
  // (resident: the pools and where[] are the device's; the host's hold the calling thread's reads only, host_where[k] for host_reads[k])
  std::vector<ChainWhere> where(T ? 0 : (size_t)n, ChainWhere{0, 0, 0, 0}), host_where;
  std::vector<int32_t> pool_cnt;
  std::vector<bpsw_seed_t> pool_seeds;

  // the seeds of the host's reads, when the caller's seeds are on the device only
  std::vector<bpsw_seed_t> fetched;
  std::vector<size_t> fetched_at;
  if (!J.h_seeds && !host_reads.empty()) {
    size_t tot = 0;
    for (int32_t r : host_reads) { fetched_at.push_back(tot); tot += (size_t)(beg[r + 1] - beg[r]); }
    fetched.resize(tot);
    for (size_t k = 0; k < host_reads.size(); ++k) {
      const int32_t r = host_reads[k];
      HIP_TRY(hipMemcpyAsync(fetched.data() + fetched_at[k], J.d_seeds + beg[r], sizeof(bpsw_seed_t) * (size_t)(beg[r + 1] - beg[r]),
                             hipMemcpyDeviceToHost, c->stream));
    }
    t_chain_bytes[1] += (int64_t)(sizeof(bpsw_seed_t) * tot);
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  auto run_host_reads = [&]() -> int {
    std::vector<bpsw_seed_t> in, cs;
    std::vector<int32_t> cnt;
    for (size_t k = 0; k < host_reads.size(); ++k) {
      const int32_t r = host_reads[k];
      const bpsw_seed_t* s = J.h_seeds ? J.h_seeds + beg[r] : fetched.data() + fetched_at[k];
      int m = (int)(beg[r + 1] - beg[r]);
      if (J.drop_bridging) {
        in.clear();
        for (int i = 0; i < m; ++i)
          if (!(s[i].rbeg < l_pac && l_pac < s[i].rbeg + s[i].len)) in.push_back(s[i]);
        s = in.data();
        m = (int)in.size();
      }
      cnt.resize((size_t)m + 1);
      cs.resize((size_t)m + 1);
      const int nc = bpsw_chain_seeds(&so, w, l_pac, m, s, J.filter, cnt.data(), m, cs.data());
      if (nc < 0) return nc;
      size_t ns = 0;
      for (int ch = 0; ch < nc; ++ch) ns += (size_t)cnt[(size_t)ch];
      const ChainWhere wh{(long long)pool_cnt.size(), (long long)pool_seeds.size(), nc, (int32_t)ns};
      if (T) host_where.push_back(wh);
      else where[(size_t)r] = wh;
      pool_cnt.insert(pool_cnt.end(), cnt.begin(), cnt.begin() + nc);
      pool_seeds.insert(pool_seeds.end(), cs.begin(), cs.begin() + (long)ns);
    }
    return BPSW_OK;
  };

  // resident chains: one buffer, laid out from n and the batch's seed total (the header of this file)
  ChainPools P{};
  long long *d_slice_cols = nullptr, *d_slice_tiles = nullptr, *d_read_tiles = nullptr, *d_rec = nullptr, *d_totals = nullptr;
  ChainTablesOut TO{};
  const int tile = scan_tile_items();
  const long long* h_rec = nullptr;  // the pinned copy of a slice's record; the totals lie behind it
  if (T) {
    const size_t S = (size_t)beg[n];
    size_t max_ns = 0;
    for (size_t s = 0; s < n_slices; ++s) max_ns = std::max(max_ns, slice_at[s + 1] - slice_at[s]);
    StageLayout L;
    const size_t o_pcnt = L.add(4 * S), o_pseeds = L.add(sizeof(bpsw_seed_t) * S);
    const size_t o_where = L.add(sizeof(ChainWhere) * (size_t)n), o_rcols = L.add(8 * 2 * ((size_t)n + 1)), zero_end = L.end;
    const size_t o_rtiles = L.add(8 * 2 * (size_t)scan_tiles(n, tile));
    const size_t o_scols = L.add(8 * 2 * (max_ns + 1)), o_stiles = L.add(8 * 2 * (size_t)scan_tiles((long long)max_ns, tile));
    const size_t o_rec = L.add(kRecBytes), o_tot = L.add(kRecBytes);
    const size_t o_ccnt = L.add(4 * (size_t)n), o_cbase = L.add(4 * (size_t)n), o_rbase = L.add(8 * (size_t)n);
    const size_t o_scnt = L.add(4 * S), o_sbase = L.add(8 * S), o_srb = L.add(8 * S), o_sqb = L.add(4 * S), o_sln = L.add(4 * S);
    HIP_TRY(c->d_chain_tab.reserve(L.total()));
    HIP_TRY(c->h_stage_out.reserve(2 * kRecBytes));
    h_rec = (const long long*)c->h_stage_out.ptr;
    uint8_t* D = (uint8_t*)c->d_chain_tab.ptr;
    P.cnt = (int32_t*)(D + o_pcnt); P.seeds = (bpsw_seed_t*)(D + o_pseeds); P.where = (ChainWhere*)(D + o_where);
    P.read_cols = (long long*)(D + o_rcols); P.n_reads = n;
    d_read_tiles = (long long*)(D + o_rtiles); d_slice_cols = (long long*)(D + o_scols); d_slice_tiles = (long long*)(D + o_stiles);
    d_rec = (long long*)(D + o_rec); d_totals = (long long*)(D + o_tot);
    TO.chain_cnt = (int32_t*)(D + o_ccnt); TO.chain_base = (int32_t*)(D + o_cbase); TO.reg_base = (long long*)(D + o_rbase);
    TO.seed_cnt = (int32_t*)(D + o_scnt); TO.seed_base = (long long*)(D + o_sbase); TO.seed_rbeg = (long long*)(D + o_srb);
    TO.seed_qbeg = (int32_t*)(D + o_sqb); TO.seed_len = (int32_t*)(D + o_sln);
    // reads without seeds are nobody's item: their where[] and columns are these zeros.  The totals start at zero too.
    HIP_TRY(hipMemsetAsync(D + o_where, 0, zero_end - o_where, c->stream));
    HIP_TRY(hipMemsetAsync(D + o_rec, 0, o_tot + kRecBytes - o_rec, c->stream));
  }
  long long dev_cnt0 = 0, dev_seed0 = 0;  // resident: what the slices so far left in the pools

  if (n_items == 0) {
    const int rc = run_host_reads();
    if (rc != BPSW_OK) return rc;
  } else {
    DeviceBuffer &d_bases = c->d_seed[0], &d_out = c->d_seed[1], &d_tab = c->d_seed[3];
    HIP_TRY(c->d_chain.reserve(arena_bytes));
    StageIn tab;
    const int i_read = tab.add(item_read.data(), 4 * n_items), i_work = tab.add(item_work.data(), 8 * n_items);
    const int i_beg = tab.add(beg, 8 * ((size_t)n + 1));
    const int i_seeds = J.d_seeds ? -1 : tab.add(J.h_seeds, sizeof(bpsw_seed_t) * (size_t)beg[n]);
    HIP_TRY(tab.stage(c->h_stage_in, d_tab, c->stream));
    t_chain_bytes[0] += (int64_t)tab.total();
    HIP_TRY(hipStreamSynchronize(c->stream));  // the pinned block is used again for every slice's offsets
    ChainArgs A;
    A.so = so; A.w = w; A.filter = J.filter ? 1 : 0; A.drop_bridging = J.drop_bridging ? 1 : 0; A.l_pac = l_pac;
    A.seed_beg = tab.dev<long long>(i_beg);
    A.seeds = J.d_seeds ? J.d_seeds : tab.dev<bpsw_seed_t>(i_seeds);
    A.arena = (uint8_t*)c->d_chain.ptr;
    std::vector<ItemCounts> counts;
    std::vector<long long> chain_base, seed_base;
    for (size_t s = 0; s < n_slices; ++s) {
      const size_t i0 = slice_at[s], ns = slice_at[s + 1] - i0;
      A.n_items = (int)ns;
      A.item_read = tab.dev<int32_t>(i_read) + i0;
      A.item_work = tab.dev<long long>(i_work) + i0;
      const dim3 grid((unsigned)((ns + 63) / 64));
      if (T) {
        // the counts stay in d_seed[1], the columns are summed by the scan, the chains go to the pools: 32 bytes come back
        const size_t o_counts_end = align16(sizeof(ItemCounts) * ns);
        HIP_TRY(d_out.reserve(o_counts_end + 16));
        int* d_err = (int*)((uint8_t*)d_out.ptr + o_counts_end);
        HIP_TRY(hipMemsetAsync(d_err, 0, 16, c->stream));
        hipLaunchKernelGGL(chain_kernel, grid, dim3(64), 0, c->stream, A, (ItemCounts*)d_out.ptr, d_err, d_slice_cols);
        HIP_TRY(hipGetLastError());
        HIP_TRY(scan_exclusive_i64(c->stream, d_slice_cols, 2, (long long)ns, tile, d_slice_tiles));
        hipLaunchKernelGGL(chain_emit_resident_kernel, grid, dim3(64), 0, c->stream, A, (const long long*)d_slice_cols, dev_cnt0, dev_seed0, P,
                           (const int*)d_err, d_rec);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync((void*)h_rec, d_rec, kRecBytes, hipMemcpyDeviceToHost, c->stream));
        t_chain_bytes[1] += (int64_t)kRecBytes;
        int host_rc = BPSW_OK;
        if (s == 0) host_rc = run_host_reads();  // while the kernels run
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (host_rc != BPSW_OK) return host_rc;
        const int err = (int)h_rec[0];
        if (err == -cc::ERR_SEED) return fail(BPSW_ERR_ARG, "chain_batch: seed with a negative start or no length");
        if (err) return fail(BPSW_ERR_DEVICE, "chain_batch: a read's chains outgrew their workspace");
        dev_cnt0 += h_rec[1];
        dev_seed0 += h_rec[2];
        if (dev_cnt0 > beg[n] || dev_seed0 > beg[n]) return fail(BPSW_ERR_DEVICE, "chain_batch: more kept chains or seeds than seeds");
        continue;
      }
      StageOut oc;
      const int r_cnt = oc.add(sizeof(ItemCounts) * ns), r_err = oc.add(16);
      HIP_TRY(oc.reserve(c->h_stage_out, d_out));
      HIP_TRY(hipMemsetAsync(oc.dev<int>(r_err), 0, 16, c->stream));
      hipLaunchKernelGGL(chain_kernel, grid, dim3(64), 0, c->stream, A, oc.dev<ItemCounts>(r_cnt), oc.dev<int>(r_err), (long long*)nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(oc.fetch(c->stream));
      t_chain_bytes[1] += (int64_t)oc.total();
      int host_rc = BPSW_OK;
      if (s == 0) host_rc = run_host_reads();  // while the kernel runs
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (host_rc != BPSW_OK) return host_rc;
      const int err = *oc.host<int>(r_err);
      if (err == -cc::ERR_SEED) return fail(BPSW_ERR_ARG, "chain_batch: seed with a negative start or no length");
      if (err) return fail(BPSW_ERR_DEVICE, "chain_batch: a read's chains outgrew their workspace");
      counts.assign(oc.host<ItemCounts>(r_cnt), oc.host<ItemCounts>(r_cnt) + ns);
      chain_base.resize(ns);
      seed_base.resize(ns);
      long long tc = 0, ts = 0;
      for (size_t i = 0; i < ns; ++i) {
        chain_base[i] = tc; seed_base[i] = ts;
        tc += counts[i].chains; ts += counts[i].seeds;
      }
      if (tc == 0) continue;
      StageIn ib;
      const int i_cb = ib.add(chain_base.data(), 8 * ns), i_sb = ib.add(seed_base.data(), 8 * ns);
      StageOut oe;
      const int r_cc = oe.add(4 * (size_t)tc), r_cs = oe.add(sizeof(bpsw_seed_t) * (size_t)ts);
      HIP_TRY(oe.reserve(c->h_stage_out, d_out));
      HIP_TRY(ib.stage(c->h_stage_in, d_bases, c->stream));
      t_chain_bytes[0] += (int64_t)ib.total();
      hipLaunchKernelGGL(chain_emit_kernel, grid, dim3(64), 0, c->stream, A, ib.dev<long long>(i_cb), ib.dev<long long>(i_sb),
                         oe.dev<int32_t>(r_cc), oe.dev<bpsw_seed_t>(r_cs));
      HIP_TRY(hipGetLastError());
      HIP_TRY(oe.fetch(c->stream));
      t_chain_bytes[1] += (int64_t)oe.total();
      HIP_TRY(hipStreamSynchronize(c->stream));
      const long long cnt0 = (long long)pool_cnt.size(), seed0 = (long long)pool_seeds.size();
      pool_cnt.insert(pool_cnt.end(), oe.host<int32_t>(r_cc), oe.host<int32_t>(r_cc) + tc);
      pool_seeds.insert(pool_seeds.end(), oe.host<bpsw_seed_t>(r_cs), oe.host<bpsw_seed_t>(r_cs) + ts);
      for (size_t i = 0; i < ns; ++i)
        where[(size_t)item_read[i0 + i]] = ChainWhere{cnt0 + chain_base[i], seed0 + seed_base[i], counts[i].chains, counts[i].seeds};
    }
  }
  if (T) {
    // the calling thread's chains into the pools behind the slices', one scan in read order, the tables, the totals
    if (!host_reads.empty()) {
      if (dev_cnt0 + (long long)pool_cnt.size() > beg[n] || dev_seed0 + (long long)pool_seeds.size() > beg[n])
        return fail(BPSW_ERR_DEVICE, "chain_batch: more kept chains or seeds than seeds");
      StageIn hb;
      const int i_hr = hb.add(host_reads.data(), 4 * host_reads.size()), i_hw = hb.add(host_where.data(), sizeof(ChainWhere) * host_where.size());
      const int i_hc = hb.add(pool_cnt.data(), 4 * pool_cnt.size()), i_hs = hb.add(pool_seeds.data(), sizeof(bpsw_seed_t) * pool_seeds.size());
      HIP_TRY(hb.stage(c->h_stage_in, c->d_seed[0], c->stream));
      t_chain_bytes[0] += (int64_t)hb.total();
      const size_t most = std::max(host_reads.size(), std::max(pool_cnt.size(), pool_seeds.size()));
      hipLaunchKernelGGL(chain_host_merge_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, c->stream, (long long)host_reads.size(),
                         hb.dev<int32_t>(i_hr), hb.dev<ChainWhere>(i_hw), (long long)pool_cnt.size(), hb.dev<int32_t>(i_hc),
                         (long long)pool_seeds.size(), hb.dev<bpsw_seed_t>(i_hs), dev_cnt0, dev_seed0, P);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(scan_exclusive_i64(c->stream, P.read_cols, 2, n, tile, d_read_tiles));
    hipLaunchKernelGGL(chain_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, P, (const long long*)P.read_cols, TO, d_totals);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync((void*)(h_rec + 4), d_totals, kRecBytes, hipMemcpyDeviceToHost, c->stream));
    t_chain_bytes[1] += (int64_t)kRecBytes;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long* tot = h_rec + 4;
    if (tot[0] > 0x7fffffffll) return fail(BPSW_ERR_LIMIT, "chain_batch: too many chains in one batch");
    T->chain_cnt = TO.chain_cnt; T->chain_base = TO.chain_base; T->reg_base = TO.reg_base; T->seed_cnt = TO.seed_cnt;
    T->seed_base = TO.seed_base; T->seed_rbeg = TO.seed_rbeg; T->seed_qbeg = TO.seed_qbeg; T->seed_len = TO.seed_len;
    T->nchains = tot[0]; T->nseeds = tot[1]; T->max_seeds = (int)tot[2];
    return BPSW_OK;
  }
  // read order
  R->chain_seed_cnt.reserve(pool_cnt.size());
  R->seeds.reserve(pool_seeds.size());
  for (int r = 0; r < n; ++r) {
    const ChainWhere& wh = where[(size_t)r];
    R->chain_cnt[(size_t)r] = wh.chains;
    R->chain_seed_cnt.insert(R->chain_seed_cnt.end(), pool_cnt.begin() + (long)wh.cnt_at, pool_cnt.begin() + (long)(wh.cnt_at + wh.chains));
    R->seeds.insert(R->seeds.end(), pool_seeds.begin() + (long)wh.seed_at, pool_seeds.begin() + (long)(wh.seed_at + wh.seeds));
  }
  return BPSW_OK;
}

}  // namespace bpsw

namespace {

// bpsw_chain_batch, and with `tables` bpsw_chain_batch_ex(BPSW_CHAIN_TABLES_DEVICE): the stage leaves the chains on the device as it does
// for the round loop, and the tables are fetched for the caller only
int chain_batch_impl(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t* seed_cnt,
                     const bpsw_seed_t* seeds, int32_t filter, int32_t* chain_cnt, int32_t* chain_seed_cnt, int64_t chain_cap,
                     bpsw_seed_t* out_seeds, int64_t seed_cap, int64_t* chain_total, int64_t* seed_total, bool tables) {
  if (!c || !sopt || n_reads < 0 || !chain_total || !seed_total || (n_reads > 0 && (!seed_cnt || !chain_cnt)))
    return fail(BPSW_ERR_ARG, "chain_batch: null argument");
  *chain_total = *seed_total = 0;
  if (n_reads == 0) return BPSW_OK;
  std::vector<long long> beg((size_t)n_reads + 1, 0);
  for (int r = 0; r < n_reads; ++r) {
    if (seed_cnt[r] < 0) return fail(BPSW_ERR_ARG, "chain_batch: negative seed count");
    beg[(size_t)r + 1] = beg[(size_t)r] + seed_cnt[r];
  }
  const long long total = beg[(size_t)n_reads];
  if (total > 0 && !seeds) return fail(BPSW_ERR_ARG, "chain_batch: null argument");
  if (total > 0x3fffffffll) return fail(BPSW_ERR_LIMIT, "chain_batch: more than 2^30 seeds in one batch");
  for (long long k = 0; k < total; ++k)
    if (seeds[k].len < 1 || seeds[k].qbeg < 0) return fail(BPSW_ERR_ARG, "chain_batch: seed with a negative start or no length");
  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  ChainDevJob J;
  J.n_reads = n_reads; J.seed_beg = beg.data(); J.d_seeds = nullptr; J.h_seeds = seeds; J.filter = filter; J.drop_bridging = 0;
  if (tables) {
    ChainTablesDev T;
    const int rc = chain_dev_run(c, *sopt, w, l_pac, J, nullptr, &T);
    if (rc != BPSW_OK) return rc;
    *chain_total = (int64_t)T.nchains;
    *seed_total = (int64_t)T.nseeds;
    if (*chain_total > chain_cap || *seed_total > seed_cap || (*chain_total && !chain_seed_cnt) || (*seed_total && !out_seeds))
      return fail(BPSW_ERR_CAPACITY, "chain_batch: chain_seed_cnt / out_seeds too small (the totals say what is needed)");
    const size_t nc = (size_t)T.nchains, ns = (size_t)T.nseeds;
    std::vector<long long> rbeg(ns);
    std::vector<int32_t> qbeg(ns), len(ns);
    HIP_TRY(hipMemcpyAsync(chain_cnt, T.chain_cnt, 4 * (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
    if (nc) HIP_TRY(hipMemcpyAsync(chain_seed_cnt, T.seed_cnt, 4 * nc, hipMemcpyDeviceToHost, c->stream));
    if (ns) {
      HIP_TRY(hipMemcpyAsync(rbeg.data(), T.seed_rbeg, 8 * ns, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(qbeg.data(), T.seed_qbeg, 4 * ns, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(len.data(), T.seed_len, 4 * ns, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < ns; ++k) { out_seeds[k].rbeg = rbeg[k]; out_seeds[k].qbeg = qbeg[k]; out_seeds[k].len = len[k]; }
    return BPSW_OK;
  }
  ChainDevResult R;
  const int rc = chain_dev_run(c, *sopt, w, l_pac, J, &R);
  if (rc != BPSW_OK) return rc;
  *chain_total = (int64_t)R.chain_seed_cnt.size();
  *seed_total = (int64_t)R.seeds.size();
  if (*chain_total > chain_cap || *seed_total > seed_cap || (*chain_total && !chain_seed_cnt) || (*seed_total && !out_seeds))
    return fail(BPSW_ERR_CAPACITY, "chain_batch: chain_seed_cnt / out_seeds too small (the totals say what is needed)");
  memcpy(chain_cnt, R.chain_cnt.data(), 4 * (size_t)n_reads);
  if (*chain_total) memcpy(chain_seed_cnt, R.chain_seed_cnt.data(), 4 * R.chain_seed_cnt.size());
  if (*seed_total) memcpy(out_seeds, R.seeds.data(), sizeof(bpsw_seed_t) * R.seeds.size());
  return BPSW_OK;
}

}  // namespace

extern "C" {

int bpsw_chain_batch(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t* seed_cnt,
                     const bpsw_seed_t* seeds, int32_t filter, int32_t* chain_cnt, int32_t* chain_seed_cnt, int64_t chain_cap,
                     bpsw_seed_t* out_seeds, int64_t seed_cap, int64_t* chain_total, int64_t* seed_total) {
  return chain_batch_impl(c, sopt, w, l_pac, n_reads, seed_cnt, seeds, filter, chain_cnt, chain_seed_cnt, chain_cap, out_seeds, seed_cap,
                          chain_total, seed_total, false);
}

int bpsw_chain_batch_ex(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t* seed_cnt,
                        const bpsw_seed_t* seeds, int32_t filter, int32_t* chain_cnt, int32_t* chain_seed_cnt, int64_t chain_cap,
                        bpsw_seed_t* out_seeds, int64_t seed_cap, int64_t* chain_total, int64_t* seed_total, int flags) {
  if (flags & ~BPSW_CHAIN_TABLES_DEVICE) return fail(BPSW_ERR_ARG, "chain_batch_ex: unknown flag");
  return chain_batch_impl(c, sopt, w, l_pac, n_reads, seed_cnt, seeds, filter, chain_cnt, chain_seed_cnt, chain_cap, out_seeds, seed_cap,
                          chain_total, seed_total, flags != 0);
}

void bpsw_last_chain_bytes(int64_t b[2]) {
  if (b) memcpy(b, t_chain_bytes, sizeof t_chain_bytes);
}

void bpsw_chain_set_arena_budget(int64_t bytes) { g_arena_budget.store(bytes > 0 ? (long long)bytes : 0, std::memory_order_relaxed); }

void bpsw_chain_last_split(int64_t st[4]) {
  if (st) memcpy(st, t_last, sizeof t_last);
}

}  // extern "C"
