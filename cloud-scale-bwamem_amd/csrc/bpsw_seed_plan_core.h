// bpsw_seed_plan_core.h -- the per-read arithmetic of the seeding plan: which bi-intervals of a read are kept, how many
// occurrences they stand for, and where their entries of the suffix-array pass's tables go.
//
// __host__ __device__: seed_plan_count_kernel / seed_plan_fill_kernel (bpsw_seed.hip) call these functions one read per lane, and
// tests/seed_plan_host/seed_plan_host.cpp compiles the same functions with g++ against the loop seed_run runs on the calling thread
// when the plan is not on the device.
//
// A read's interval row: the first pass of seed_smem_kernel writes rows of `stride` records, row r at first + r * stride; a read that
// produced more (cnt[r] > stride) is run once more alone, and its row is more + base[i] where todo[i] == r -- todo ascending, as
// the host builds it from cnt.
#pragma once
#include <stdint.h>

#include "bpsw.h"

#if defined(__HIPCC__)
#define BPSW_PLAN_HD __host__ __device__ __forceinline__
#else
#define BPSW_PLAN_HD inline
#endif

namespace bpsw {

struct SeedPlanRows {
  const int32_t* cnt;        // intervals per read (first pass)
  const bpsw_smem_t* first;  // first-pass rows
  int stride;
  const int32_t* todo;       // reads of the second pass, ascending
  int n_todo;
  const long long* base;     // n_todo + 1: where each one's row begins in `more`
  const bpsw_smem_t* more;   // second-pass rows
};

// the place of read r in todo (r is there: cnt[r] > stride)
BPSW_PLAN_HD int seed_plan_todo_index(const SeedPlanRows& R, long long r) {
  int lo = 0, hi = R.n_todo - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (R.todo[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

BPSW_PLAN_HD const bpsw_smem_t* seed_plan_row(const SeedPlanRows& R, long long r) {
  if (R.cnt[r] <= R.stride) return R.first + (size_t)r * (size_t)R.stride;
  return R.more + R.base[seed_plan_todo_index(R, r)];
}

// the number of kept intervals of read r and the sum of their x2 (zero-width kept intervals count as intervals)
BPSW_PLAN_HD void seed_plan_count(const SeedPlanRows& R, long long r, long long* n_kept, long long* n_occ) {
  const bpsw_smem_t* row = seed_plan_row(R, r);
  long long k = 0, occ = 0;
  for (int j = 0; j < R.cnt[r]; ++j) {
    if (!row[j].kept) continue;
    ++k;
    occ += row[j].x2;
  }
  *n_kept = k;
  *n_occ = occ;
}

// read r's kept intervals, in row order, into entries kept_base .. of the tables; occ: the occurrences before the read's first one
BPSW_PLAN_HD void seed_plan_fill(const SeedPlanRows& R, long long r, long long kept_base, long long occ, long long* occ_base,
                                 long long* kept_x0, int32_t* kept_q) {
  const bpsw_smem_t* row = seed_plan_row(R, r);
  for (int j = 0; j < R.cnt[r]; ++j) {
    if (!row[j].kept) continue;
    occ_base[kept_base] = occ;
    kept_x0[kept_base] = row[j].x0;
    kept_q[2 * kept_base] = row[j].qbeg;
    kept_q[2 * kept_base + 1] = row[j].qend;
    ++kept_base;
    occ += row[j].x2;
  }
}

}  // namespace bpsw
