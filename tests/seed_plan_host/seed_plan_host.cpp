// The seeding plan's per-read arithmetic (csrc/bpsw_seed_plan_core.h: what seed_plan_count_kernel and seed_plan_fill_kernel call,
// one read per lane) compiled for the host, with a plain sequential scan between the two, against the loop seed_run (csrc/bpsw_seed.hip)
// runs on the calling thread over the intervals it copied back.  A program of its own: tests/test_seed_plan_core_host.py builds it
// with -fsanitize=address,undefined and runs it; every array is malloc'd at exactly the size the plan gives it.
//
// The input is generated interval tables in the layout the kernels see: first-pass rows of 16 records, and for the reads with more
// than 16 intervals a second-pass row each, found through todo / base.  A read with more than 16 intervals has a first-pass row of
// poison (kept, x2 = 12345), so that a plan that reads the wrong row cannot agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpsw_seed_plan_core.h"

using namespace bpsw;

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

constexpr int kStride = 16;
constexpr int64_t kMaxX2 = 0x7fffffffll;  // max_occ is an int: a kept interval's x2 never exceeds it

template <class T>
T* exact(size_t n) {  // exactly n elements: one past the end is the sanitizer's
  T* p = (T*)malloc(n ? n * sizeof(T) : 1);
  if (!p) abort();
  return p;
}

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// one read's intervals: `shape` decides the kept flags and the widths
std::vector<bpsw_smem_t> make_read(Rng& g, int cnt, int shape) {
  std::vector<bpsw_smem_t> v((size_t)cnt);
  for (int j = 0; j < cnt; ++j) {
    bpsw_smem_t& e = v[(size_t)j];
    e.x0 = (int64_t)(g.next() >> 23);
    e.x1 = (int64_t)(g.next() >> 23);
    e.qbeg = g.below(200);
    e.qend = e.qbeg + 1 + g.below(56);
    e.pad_ = 0;
    e.kept = g.below(3) != 0;
    e.x2 = 1 + g.below(40);
    switch (shape) {
      case 1: e.kept = 0; break;                                                      // nothing kept
      case 2: e.kept = 1; break;                                                      // everything kept
      case 3: if (j == 0) { e.kept = 1; e.x2 = 0; } break;                            // a kept zero-width interval first
      case 4: if (j == cnt - 1) { e.kept = 1; e.x2 = 0; } break;                      // ... last
      case 5: if (j >= cnt / 3 && j <= cnt / 3 + 3) { e.kept = 1; e.x2 = 0; } break;  // ... a run of them
      case 6: e.kept = 1; e.x2 = 0; break;                                            // ... and nothing else
      case 7: e.kept = 1; e.x2 = kMaxX2 - g.below(3); break;                          // the widest a kept interval gets
      case 8: if (!e.kept) e.x2 = kMaxX2 * 4 + g.below(1000); break;                  // skipped intervals wider than max_occ
      default: break;
    }
  }
  return v;
}

}  // namespace

int main() {
  Rng g{20261019};
  const int n = 10007;
  // ---- the reads ----
  std::vector<std::vector<bpsw_smem_t>> reads((size_t)n);
  int census[5] = {0, 0, 0, 0, 0};  // reads with 0 intervals, with exactly 16, with 17, with more than 17, with 254
  for (int r = 0; r < n; ++r) {
    int cnt;
    const int pick = r < 40 ? r % 8 : g.below(100);  // (the first reads go through every kind once more, so that none depends on chance)
    if (pick == 0) cnt = 0;
    else if (pick == 1) cnt = kStride;
    else if (pick == 2) cnt = kStride + 1;
    else if (pick == 3) cnt = 254;
    else if (pick < 12) cnt = kStride + 2 + g.below(40);
    else cnt = 1 + g.below(kStride);
    const int shape = r < 200 ? r % 9 : g.below(12);
    reads[(size_t)r] = make_read(g, cnt, shape);
    census[0] += cnt == 0; census[1] += cnt == kStride; census[2] += cnt == kStride + 1; census[3] += cnt > kStride + 1; census[4] += cnt == 254;
  }
  reads[0].clear();                       // the first and the last read without an interval
  reads[(size_t)n - 1].clear();
  reads[1] = make_read(g, 254, 7);        // 254 x (2^31 - 1): a read's sum passes 2^32 by itself
  reads[2] = make_read(g, kStride, 7);
  CHECK(census[0] > 50 && census[1] > 50 && census[2] > 50 && census[3] > 500 && census[4] > 50);

  // ---- the layout the kernels see ----
  int32_t* cnt = exact<int32_t>((size_t)n);
  bpsw_smem_t* first = exact<bpsw_smem_t>((size_t)n * kStride);
  std::vector<int32_t> todo_v;
  std::vector<long long> base_v(1, 0);
  for (int r = 0; r < n; ++r) {
    cnt[r] = (int32_t)reads[(size_t)r].size();
    if (cnt[r] > kStride) { todo_v.push_back(r); base_v.push_back(base_v.back() + cnt[r]); }
  }
  const size_t m = todo_v.size();
  int32_t* todo = exact<int32_t>(m);
  long long* base = exact<long long>(m + 1);
  memcpy(todo, todo_v.data(), 4 * m);
  memcpy(base, base_v.data(), 8 * (m + 1));
  bpsw_smem_t* more = exact<bpsw_smem_t>((size_t)base_v.back());
  size_t ti = 0;
  for (int r = 0; r < n; ++r) {
    bpsw_smem_t* row = first + (size_t)r * kStride;
    for (int j = 0; j < kStride; ++j) {  // poison: what a first-pass row holds beyond its count, or of a read that overflowed, is not the plan's
      memset(&row[j], 0, sizeof row[j]);
      row[j].kept = 1; row[j].x2 = 12345; row[j].x0 = -7; row[j].qbeg = -1; row[j].qend = -2;
    }
    if (cnt[r] <= kStride) {
      for (int j = 0; j < cnt[r]; ++j) row[j] = reads[(size_t)r][(size_t)j];
    } else {
      for (int j = 0; j < cnt[r]; ++j) more[base[ti] + j] = reads[(size_t)r][(size_t)j];
      ++ti;
    }
  }
  CHECK(ti == m);

  // ---- seed_run's loop on the calling thread: the intervals concatenated in read order, then the plan ----
  std::vector<bpsw_smem_t> intv;
  ti = 0;
  for (int r = 0; r < n; ++r) {
    const int k = cnt[r];
    if (k <= kStride) intv.insert(intv.end(), first + (size_t)r * kStride, first + (size_t)r * kStride + k);
    else { intv.insert(intv.end(), more + base[ti], more + base[ti] + k); ++ti; }
  }
  std::vector<long long> occ_base, kept_x0;
  std::vector<int32_t> kept_q;
  std::vector<long long> read_occ((size_t)n + 1, 0);
  long long n_occ = 0;
  {
    size_t at = 0;
    for (int r = 0; r < n; ++r) {
      read_occ[(size_t)r] = n_occ;
      for (int k = 0; k < cnt[r]; ++k, ++at) {
        const bpsw_smem_t& e = intv[at];
        if (!e.kept) continue;
        occ_base.push_back(n_occ); kept_x0.push_back(e.x0);
        kept_q.push_back(e.qbeg); kept_q.push_back(e.qend);
        n_occ += e.x2;
      }
    }
    read_occ[(size_t)n] = n_occ;
  }
  const size_t nk = occ_base.size();
  occ_base.push_back(n_occ);
  CHECK(n_occ > (1ll << 32));  // the sums pass 2^32: a 32-bit scan cannot agree

  // ---- the plan as the device makes it: count per read, exclusive scan of both columns with the totals in entry n, fill ----
  SeedPlanRows R;
  R.cnt = cnt; R.first = first; R.stride = kStride; R.todo = todo; R.n_todo = (int)m; R.base = base; R.more = more;
  long long* col_kept = exact<long long>((size_t)n + 1);
  long long* col_occ = exact<long long>((size_t)n + 1);
  for (int r = 0; r < n; ++r) seed_plan_count(R, r, &col_kept[r], &col_occ[r]);
  long long sum_kept = 0, sum_occ = 0;
  for (int r = 0; r < n; ++r) {
    const long long a = col_kept[r], b = col_occ[r];
    col_kept[r] = sum_kept; col_occ[r] = sum_occ;
    sum_kept += a; sum_occ += b;
  }
  col_kept[n] = sum_kept; col_occ[n] = sum_occ;
  CHECK((size_t)sum_kept == nk);
  CHECK(sum_occ == n_occ);
  long long* d_occ_base = exact<long long>((size_t)sum_kept + 1);
  long long* d_x0 = exact<long long>((size_t)sum_kept);
  int32_t* d_q = exact<int32_t>(2 * (size_t)sum_kept);
  for (int r = n - 1; r >= 0; --r)  // (any order: the lanes of a launch have none)
    seed_plan_fill(R, r, col_kept[r], col_occ[r], d_occ_base, d_x0, d_q);
  d_occ_base[col_kept[n]] = col_occ[n];

  CHECK(memcmp(col_occ, read_occ.data(), 8 * ((size_t)n + 1)) == 0);
  CHECK(memcmp(d_occ_base, occ_base.data(), 8 * (nk + 1)) == 0);
  CHECK(memcmp(d_x0, kept_x0.data(), 8 * nk) == 0);
  CHECK(memcmp(d_q, kept_q.data(), 8 * nk) == 0);

  // every read of the second pass is found through todo, the first and the last one included
  for (size_t i = 0; i < m; ++i) CHECK(seed_plan_todo_index(R, todo[i]) == (int)i);
  long long zero_kept = 0;
  for (const bpsw_smem_t& e : intv) zero_kept += e.kept && e.x2 == 0;
  CHECK(zero_kept > 1000);

  printf("seed plan core: %d reads, %zu in the second pass, %zu intervals, %zu kept (%lld of zero width), %lld occurrences: equal\n", n, m,
         intv.size(), nk, zero_kept, n_occ);
  free(cnt); free(first); free(todo); free(base); free(more); free(col_kept); free(col_occ); free(d_occ_base); free(d_x0); free(d_q);
  return 0;
}
