// chain_tables_host.cpp -- csrc/bpsw_chain_tables_core.h (what chain_tables_kernel calls one read per lane) compiled for the host,
// against the arrays bpsw_chain2aln_batch's host loop builds from the same chains.  A program of its own, built by
// tests/test_chain_tables_core_host.py under -fsanitize=address,undefined together with csrc/bpsw_chain.cpp (bpsw_chain_seeds).
//
// Reads: generated seed lists -- empty reads first, last and in runs, short clustered reads, one read of 3 000 seeds, one read of
// 2 000 chains of one seed.  Their filtered chains (bpsw_chain_seeds) are put into the two pools the way the chain stage does it: the
// reads dealt by descending seed count into three slices, the longest read behind them as the calling thread's; where[] records
// the places.  Then a sequential exclusive scan of the (chains, seeds) columns in read order and chain_tables_read per read, in
// an order of its own, into arrays allocated at exactly their size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bpsw.h"
#include "bpsw_chain_tables_core.h"

namespace bpsw {  // what bpsw_chain.cpp takes from the runtime
void set_error(const std::string&) {}
int fail(int code, const std::string& msg) {
  fprintf(stderr, "%s\n", msg.c_str());
  return code;
}
}  // namespace bpsw

using bpsw::ChainTablesOut;
using bpsw::ChainWhere;

namespace {

constexpr int64_t L_PAC = 1000000000;
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

std::vector<bpsw_seed_t> clustered(int n, int spots) {
  std::vector<int64_t> locus((size_t)spots);
  for (int64_t& l : locus) l = 1000 + below(399000) + (below(2) ? L_PAC : 0);
  std::vector<bpsw_seed_t> s((size_t)n);
  for (bpsw_seed_t& e : s) {
    e.qbeg = (int32_t)below(200);
    e.len = 19 + (int32_t)below(41);
    e.rbeg = locus[(size_t)below(spots)] + e.qbeg + below(7) - 3;
  }
  return s;
}
std::vector<bpsw_seed_t> distinct(int n) {  // further apart than max_chain_gap: every seed founds a chain
  std::vector<bpsw_seed_t> s((size_t)n);
  for (int i = 0; i < n; ++i) {
    s[(size_t)i].rbeg = 5000 + 20011ll * i;
    s[(size_t)i].qbeg = (int32_t)below(120);
    s[(size_t)i].len = 19 + (int32_t)below(51);
  }
  for (int i = n - 1; i > 0; --i) std::swap(s[(size_t)i], s[(size_t)below(i + 1)]);
  return s;
}

template <class Tp> Tp* exact(size_t n) { return (Tp*)malloc(sizeof(Tp) * n + (n ? 0 : 1)); }  // (the sanitizer sees one element too many)

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      return 1;                                                   \
    }                                                             \
  } while (0)

}  // namespace

int main() {
  bpsw_seed_opt_t so;
  bpsw_seed_opt_default(&so);
  // ---- the reads ----
  std::vector<std::vector<bpsw_seed_t>> reads;
  for (int i = 0; i < 3; ++i) reads.emplace_back();
  for (int i = 0; i < 400; ++i) {
    if (i % 37 == 5) for (int k = 0; k < 1 + i % 4; ++k) reads.emplace_back();  // runs of reads without seeds
    reads.push_back(clustered((int)below(40), 2 + (int)below(5)));
    if (i == 150) reads.push_back(clustered(3000, 400));
    if (i == 300) reads.push_back(distinct(2000));
  }
  for (int i = 0; i < 2; ++i) reads.emplace_back();
  const size_t n = reads.size();
  // ---- their chains, per read ----
  std::vector<std::vector<int32_t>> cnt(n);
  std::vector<std::vector<bpsw_seed_t>> kept(n);
  size_t n_empty = 0, n_no_chain = 0;
  for (size_t r = 0; r < n; ++r) {
    const int m = (int)reads[r].size();
    n_empty += m == 0;
    std::vector<int32_t> c((size_t)m + 1);
    std::vector<bpsw_seed_t> o((size_t)m + 1);
    const int nc = bpsw_chain_seeds(&so, 100, L_PAC, m, reads[r].data(), 1, c.data(), m, o.data());
    CHECK(nc >= 0);
    size_t ns = 0;
    for (int k = 0; k < nc; ++k) ns += (size_t)c[(size_t)k];
    cnt[r].assign(c.begin(), c.begin() + nc);
    kept[r].assign(o.begin(), o.begin() + (long)ns);
    n_no_chain += nc == 0;
  }
  // ---- what the host loop of bpsw_chain2aln_batch builds from them (csrc/bpsw_sw_runtime.cpp) ----
  std::vector<int32_t> w_chain_cnt(n), w_chain_base(n), w_seed_cnt, w_qbeg, w_len;
  std::vector<long long> w_reg_base(n), w_seed_base, w_rbeg;
  long long nchains = 0, nseeds = 0;
  int max_seeds = 0;
  for (size_t r = 0; r < n; ++r) {
    w_chain_cnt[r] = (int32_t)cnt[r].size();
    w_chain_base[r] = (int32_t)nchains;
    w_reg_base[r] = nseeds;
    size_t at = 0;
    for (const int32_t ns : cnt[r]) {
      w_seed_cnt.push_back(ns);
      w_seed_base.push_back(nseeds);
      for (int i = 0; i < ns; ++i, ++at) { w_rbeg.push_back(kept[r][at].rbeg); w_qbeg.push_back(kept[r][at].qbeg); w_len.push_back(kept[r][at].len); }
      max_seeds = std::max(max_seeds, ns);
      nseeds += ns;
      ++nchains;
    }
  }
  // ---- the pools, as the chain stage fills them ----
  std::vector<size_t> order;
  size_t longest = 0;
  for (size_t r = 0; r < n; ++r) if (reads[r].size() > reads[longest].size()) longest = r;
  for (size_t r = 0; r < n; ++r) if (!reads[r].empty() && r != longest) order.push_back(r);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return reads[a].size() > reads[b].size(); });
  order.push_back(longest);  // the calling thread's read: behind the slices
  int32_t* pool_cnt = exact<int32_t>((size_t)nchains);
  bpsw_seed_t* pool_seeds = exact<bpsw_seed_t>((size_t)nseeds);
  ChainWhere* where = exact<ChainWhere>(n);
  for (size_t r = 0; r < n; ++r) where[r] = ChainWhere{0, 0, 0, 0};
  long long ca = 0, sa = 0;
  for (const size_t r : order) {
    where[r] = ChainWhere{ca, sa, (int32_t)cnt[r].size(), (int32_t)kept[r].size()};
    for (const int32_t v : cnt[r]) pool_cnt[ca++] = v;
    for (const bpsw_seed_t& s : kept[r]) pool_seeds[sa++] = s;
  }
  CHECK(ca == nchains && sa == nseeds);
  // ---- a sequential exclusive scan of the two columns in read order ----
  std::vector<long long> col_c(n + 1), col_s(n + 1);
  {
    long long c = 0, s = 0;
    for (size_t r = 0; r < n; ++r) { col_c[r] = c; col_s[r] = s; c += where[r].chains; s += where[r].seeds; }
    col_c[n] = c; col_s[n] = s;
  }
  CHECK(col_c[n] == nchains && col_s[n] == nseeds);
  // ---- the tables ----
  ChainTablesOut T;
  T.chain_cnt = exact<int32_t>(n); T.chain_base = exact<int32_t>(n); T.reg_base = exact<long long>(n);
  T.seed_cnt = exact<int32_t>((size_t)nchains); T.seed_base = exact<long long>((size_t)nchains);
  T.seed_rbeg = exact<long long>((size_t)nseeds); T.seed_qbeg = exact<int32_t>((size_t)nseeds); T.seed_len = exact<int32_t>((size_t)nseeds);
  memset(T.seed_cnt, 0xff, 4 * (size_t)nchains); memset(T.seed_base, 0xff, 8 * (size_t)nchains);
  memset(T.seed_rbeg, 0xff, 8 * (size_t)nseeds); memset(T.seed_qbeg, 0xff, 4 * (size_t)nseeds); memset(T.seed_len, 0xff, 4 * (size_t)nseeds);
  std::vector<size_t> lanes(n);
  for (size_t r = 0; r < n; ++r) lanes[r] = r;
  for (size_t i = n - 1; i > 0; --i) std::swap(lanes[i], lanes[(size_t)below((int64_t)i + 1)]);
  int largest = 0;
  for (const size_t r : lanes)
    largest = std::max(largest, bpsw::chain_tables_read(where, pool_cnt, pool_seeds, (long long)r, col_c[r], col_s[r], T));
  CHECK(largest == max_seeds);
  CHECK(memcmp(T.chain_cnt, w_chain_cnt.data(), 4 * n) == 0);
  CHECK(memcmp(T.chain_base, w_chain_base.data(), 4 * n) == 0);
  CHECK(memcmp(T.reg_base, w_reg_base.data(), 8 * n) == 0);
  CHECK(memcmp(T.seed_cnt, w_seed_cnt.data(), 4 * (size_t)nchains) == 0);
  CHECK(memcmp(T.seed_base, w_seed_base.data(), 8 * (size_t)nchains) == 0);
  CHECK(memcmp(T.seed_rbeg, w_rbeg.data(), 8 * (size_t)nseeds) == 0);
  CHECK(memcmp(T.seed_qbeg, w_qbeg.data(), 4 * (size_t)nseeds) == 0);
  CHECK(memcmp(T.seed_len, w_len.data(), 4 * (size_t)nseeds) == 0);
  printf("chain tables core: %zu reads, %zu without seeds, %zu without chains, %lld chains, %lld seeds, largest chain %d: equal\n", n, n_empty,
         n_no_chain, nchains, nseeds, largest);
  free(pool_cnt); free(pool_seeds); free(where);
  free(T.chain_cnt); free(T.chain_base); free(T.reg_base); free(T.seed_cnt); free(T.seed_base); free(T.seed_rbeg); free(T.seed_qbeg); free(T.seed_len);
  return 0;
}
