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
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>

#include "bpsw_internal.h"
#include "bpsw_chain_core.h"

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

__global__ __launch_bounds__(64) void chain_kernel(ChainArgs A, ItemCounts* __restrict__ counts, int* error) {
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

size_t slice_bytes(int m) { return kSliceHead + cc::work_bytes(m, cc::node_bound(m)); }

}  // namespace

namespace bpsw {

int chain_dev_run(bpsw_ctx* c, const bpsw_seed_opt_t& so, int w, int64_t l_pac, const ChainDevJob& J, ChainDevResult* R) {
  const int n = J.n_reads;
  const long long* beg = J.seed_beg;
  R->chain_cnt.assign((size_t)n, 0);
  R->chain_seed_cnt.clear();
  R->seeds.clear();
  t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
  if (n == 0 || beg[n] == 0) return BPSW_OK;
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
  struct Where { size_t cnt_at, seed_at; int32_t chains, seeds; };
  std::vector<Where> where((size_t)n, Where{0, 0, 0, 0});
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
      where[(size_t)r] = Where{pool_cnt.size(), pool_seeds.size(), nc, (int32_t)ns};
      pool_cnt.insert(pool_cnt.end(), cnt.begin(), cnt.begin() + nc);
      pool_seeds.insert(pool_seeds.end(), cs.begin(), cs.begin() + (long)ns);
    }
    return BPSW_OK;
  };

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
      StageOut oc;
      const int r_cnt = oc.add(sizeof(ItemCounts) * ns), r_err = oc.add(16);
      HIP_TRY(oc.reserve(c->h_stage_out, d_out));
      HIP_TRY(hipMemsetAsync(oc.dev<int>(r_err), 0, 16, c->stream));
      hipLaunchKernelGGL(chain_kernel, grid, dim3(64), 0, c->stream, A, oc.dev<ItemCounts>(r_cnt), oc.dev<int>(r_err));
      HIP_TRY(hipGetLastError());
      HIP_TRY(oc.fetch(c->stream));
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
      hipLaunchKernelGGL(chain_emit_kernel, grid, dim3(64), 0, c->stream, A, ib.dev<long long>(i_cb), ib.dev<long long>(i_sb),
                         oe.dev<int32_t>(r_cc), oe.dev<bpsw_seed_t>(r_cs));
      HIP_TRY(hipGetLastError());
      HIP_TRY(oe.fetch(c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      const size_t cnt0 = pool_cnt.size(), seed0 = pool_seeds.size();
      pool_cnt.insert(pool_cnt.end(), oe.host<int32_t>(r_cc), oe.host<int32_t>(r_cc) + tc);
      pool_seeds.insert(pool_seeds.end(), oe.host<bpsw_seed_t>(r_cs), oe.host<bpsw_seed_t>(r_cs) + ts);
      for (size_t i = 0; i < ns; ++i)
        where[(size_t)item_read[i0 + i]] = Where{cnt0 + (size_t)chain_base[i], seed0 + (size_t)seed_base[i], counts[i].chains, counts[i].seeds};
    }
  }
  // read order
  R->chain_seed_cnt.reserve(pool_cnt.size());
  R->seeds.reserve(pool_seeds.size());
  for (int r = 0; r < n; ++r) {
    const Where& wh = where[(size_t)r];
    R->chain_cnt[(size_t)r] = wh.chains;
    R->chain_seed_cnt.insert(R->chain_seed_cnt.end(), pool_cnt.begin() + (long)wh.cnt_at, pool_cnt.begin() + (long)(wh.cnt_at + (size_t)wh.chains));
    R->seeds.insert(R->seeds.end(), pool_seeds.begin() + (long)wh.seed_at, pool_seeds.begin() + (long)(wh.seed_at + (size_t)wh.seeds));
  }
  return BPSW_OK;
}

}  // namespace bpsw

extern "C" {

int bpsw_chain_batch(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_reads, const int32_t* seed_cnt,
                     const bpsw_seed_t* seeds, int32_t filter, int32_t* chain_cnt, int32_t* chain_seed_cnt, int64_t chain_cap,
                     bpsw_seed_t* out_seeds, int64_t seed_cap, int64_t* chain_total, int64_t* seed_total) {
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

void bpsw_chain_set_arena_budget(int64_t bytes) { g_arena_budget.store(bytes > 0 ? (long long)bytes : 0, std::memory_order_relaxed); }

void bpsw_chain_last_split(int64_t st[4]) {
  if (st) memcpy(st, t_last, sizeof t_last);
}

}  // extern "C"
