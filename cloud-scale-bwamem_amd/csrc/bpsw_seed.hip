// bpsw_seed.hip -- worker1's seeding on the device: the FM-index resident in HBM, SMEM search and suffix-array lookup.
//
// Replaces the interval side of mem_insert_seed (native/bwamem.c:207-228): smem_next2 (:117-156) over bwt_smem1 / bwt_extend
// (native/bwt.c:261-347) and bwt_sa (:85-95), i.e. BWTSMem.scala / MemChain.scala's generateChains up to the seeds.  Integer only
// and bit-exact: the kernels perform the reference's steps in the reference's order.
//
// Mapping: ONE READ PER LANE (seed_smem_kernel), one occurrence per lane (seed_sa_kernel).  The search is a chain of dependent
// random reads -- each bwt_extend needs the 64-byte blocks of rows k - 1 and k - 1 + x2 before the next one can be addressed --
// so the rate is set by the number of independent chains in flight, not by ALU work; a wavefront per read would keep one or two
// loads in flight per wave.  Lanes diverge (reads differ in where their matches end); that costs issue slots the kernel has to spare.
//
// The per-lane interval lists (bwt_smem1's prev / curr, smem_next2's matches / sub) live in a global arena, interleaved by
// lane: entry e of lane l of a list at e * 64 + l.  No list outgrows read_len + 1 entries: the forward sweep pushes at most one
// interval per base, the backward sweep at most as many as it was given, and mem at most one per start position.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <optional>
#include <utility>

#include "bpsw_internal.h"
#include "bpsw_seed_plan_core.h"

using namespace bpsw;

namespace {

typedef unsigned long long u64;

struct FmiDev {  // by value to the kernels
  const uint32_t* bwt;
  const long long* sa;
  u64 primary, seq_len;
  u64 L2[5];
  int sa_shift;  // log2(sa_intv)
};

struct Intv {  // bwtintv_t: info = qbeg << 32 | qend
  u64 x0, x1, x2, info;
};

// ---- bwt_occ4 / bwt_occ with popcounts on the 2-bit words (__occ_aux's reduction, no byte table) ----------------------------
// Bases of a block: eight words, base j of a word in bits 30 - 2 j.  Two words make the 64-bit y of __occ_aux (first word high).
__device__ __forceinline__ u64 pair_mask(int i, int kk) {  // which of the 32 bases of pair i lie at or before base kk of the block
  const int full = kk >> 5;
  return i < full ? ~0ull : i == full ? ~((1ull << ((~kk & 31) << 1)) - 1) : 0ull;
}
__device__ __forceinline__ void occ4(const FmiDev& F, u64 k, u64 cnt[4]) {
  if (k == ~0ull) { cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0; return; }
  k = k > F.seq_len ? F.seq_len : k;  // (a valid index never asks beyond seq_len; this keeps a corrupt one inside the array)
  k -= (k >= F.primary);
  const uint4* blk = (const uint4*)(F.bwt + ((k >> 7) << 4));
  const uint4 c0 = blk[0], c1 = blk[1], b0 = blk[2], b1 = blk[3];
  const u64 y[4] = {(u64)b0.x << 32 | b0.y, (u64)b0.z << 32 | b0.w, (u64)b1.x << 32 | b1.y, (u64)b1.z << 32 | b1.w};
  const int kk = (int)(k & 127);
  unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 v = y[i] & pair_mask(i, kk), hi = v >> 1, m = 0x5555555555555555ull;
    n0 += __popcll(~hi & ~v & m);
    n1 += __popcll(~hi & v & m);
    n2 += __popcll(hi & ~v & m);
    n3 += __popcll(hi & v & m);
  }
  n0 -= (unsigned)(127 - kk);  // the masked-out bases read as A
  cnt[0] = ((u64)c0.y << 32 | c0.x) + n0;
  cnt[1] = ((u64)c0.w << 32 | c0.z) + n1;
  cnt[2] = ((u64)c1.y << 32 | c1.x) + n2;
  cnt[3] = ((u64)c1.w << 32 | c1.z) + n3;
}
__device__ __forceinline__ u64 occ1(const FmiDev& F, u64 k, int c) {  // bwt_occ
  if (k == F.seq_len) return F.L2[c + 1] - F.L2[c];
  u64 cnt[4];
  occ4(F, k, cnt);
  return cnt[c];
}

// bwt_extend, native/bwt.c:261-274.  (bwt_2occ4's same-block shortcut is an optimisation of two bwt_occ4: not restated.)
__device__ __forceinline__ void extend(const FmiDev& F, const Intv& ik, Intv ok[4], int is_back) {
  const u64 a = is_back ? ik.x0 : ik.x1, b = is_back ? ik.x1 : ik.x0;  // a = x[!is_back], the side that is extended; b = x[is_back]
  u64 tk[4], tl[4];
  occ4(F, a - 1, tk);
  occ4(F, a - 1 + ik.x2, tl);
  u64 na[4], nb[4], n2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { na[i] = F.L2[i] + 1 + tk[i]; n2[i] = tl[i] - tk[i]; }
  nb[3] = b + (a <= F.primary && a + ik.x2 - 1 >= F.primary);
  nb[2] = nb[3] + n2[3];
  nb[1] = nb[2] + n2[2];
  nb[0] = nb[1] + n2[1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ok[i].x0 = is_back ? na[i] : nb[i];
    ok[i].x1 = is_back ? nb[i] : na[i];
    ok[i].x2 = n2[i];
    ok[i].info = 0;
  }
}

struct List {  // one lane's list in the arena
  Intv* base;  // entry e at base[e * 64]
  int n, cap;
  int* overflow;
  __device__ __forceinline__ void push(const Intv& v) {
    if (n < cap) base[(size_t)n++ * 64] = v;
    else *overflow = 1;  // (never with cap = read_len + 1; the host turns it into an error)
  }
  __device__ __forceinline__ Intv get(int e) const { return base[(size_t)e * 64]; }
  __device__ __forceinline__ void reverse() {
    for (int j = 0; j < n >> 1; ++j) {
      const Intv t = base[(size_t)(n - 1 - j) * 64];
      base[(size_t)(n - 1 - j) * 64] = base[(size_t)j * 64];
      base[(size_t)j * 64] = t;
    }
  }
};

// bwt_smem1, native/bwt.c:288-347.  t0 / t1: the two temporary lists (tmpvec); returns the reference's return value.
__device__ int smem1(const FmiDev& F, int len, const uint8_t* q, int x, u64 min_intv, List& mem, List& t0, List& t1) {
  mem.n = 0;
  if (q[x] > 3) return x + 1;
  if (min_intv < 1) min_intv = 1;
  List* prev = &t0;
  List* curr = &t1;
  Intv ik, ok[4];
  const int c0 = q[x];
  ik.x0 = F.L2[c0] + 1; ik.x2 = F.L2[c0 + 1] - F.L2[c0]; ik.x1 = F.L2[3 - c0] + 1;  // bwt_set_intv
  ik.info = (u64)(x + 1);
  int i;
  curr->n = 0;
  for (i = x + 1; i < len; ++i) {  // forward search
    if (q[i] < 4) {
      const int c = 3 - q[i];
      extend(F, ik, ok, 0);
      if (ok[c].x2 != ik.x2) {
        curr->push(ik);
        if (ok[c].x2 < min_intv) break;
      }
      ik = ok[c]; ik.info = (u64)(i + 1);
    } else {
      curr->push(ik);
      break;
    }
  }
  if (i == len) curr->push(ik);
  curr->reverse();
  const int ret = (int)(unsigned)curr->get(0).info;
  { List* s = curr; curr = prev; prev = s; }
  for (i = x - 1; i >= -1; --i) {  // backward search for MEMs
    const int c = i < 0 ? -1 : q[i] < 4 ? q[i] : -1;
    curr->n = 0;
    for (int j = 0; j < prev->n; ++j) {
      const Intv p = prev->get(j);
      bool small = c < 0;
      if (!small) { extend(F, p, ok, 1); small = ok[c].x2 < min_intv; }
      if (small) {
        if (curr->n == 0) {
          if (mem.n == 0 || (u64)(i + 1) < (mem.get(mem.n - 1).info >> 32)) {
            ik = p; ik.info |= (u64)(i + 1) << 32;
            mem.push(ik);
          }
        }
      } else if (curr->n == 0 || ok[c].x2 != curr->get(curr->n - 1).x2) {
        ok[c].info = p.info;
        curr->push(ok[c]);
      }
    }
    if (curr->n == 0) break;
    { List* s = curr; curr = prev; prev = s; }
  }
  mem.reverse();
  return ret;
}

struct SeedParams {
  int min_seed_len, max_occ, split_width, start_width;
  int split_len0;  // (int)(min_seed_len * split_factor + .499), before the per-read minimum with the read length
};

// smem_next2 until the read is used up (mem_insert_seed's loop, native/bwamem.c:207-219), one read per lane, grid-stride.
// Item i is read todo[i] (read i when todo is null); its records go to out + row_base[i], room row_base[i + 1] - row_base[i] (rows of
// `stride` records when row_base is null); cnt[i] = the number the read produced, which may exceed the room: the host then runs
// those reads alone once more, each with exactly the room it asked for.
__global__ __launch_bounds__(64) void seed_smem_kernel(FmiDev F, SeedParams P, int n_items, const int32_t* __restrict__ todo,
                                                        const int32_t* __restrict__ read_len, const long long* __restrict__ read_off,
                                                        const uint8_t* __restrict__ read_pool, Intv* arena, int list_cap, bpsw_smem_t* out,
                                                        int stride, const long long* __restrict__ row_base, int32_t* cnt, int* overflow) {
  const int lane = threadIdx.x;
  Intv* mine = arena + (size_t)blockIdx.x * 4 * (size_t)list_cap * 64 + lane;
  List M{mine, 0, list_cap, overflow}, S{mine + (size_t)list_cap * 64, 0, list_cap, overflow};
  List T0{mine + 2 * (size_t)list_cap * 64, 0, list_cap, overflow}, T1{mine + 3 * (size_t)list_cap * 64, 0, list_cap, overflow};
  for (long long it = (long long)blockIdx.x * 64 + lane; it < n_items; it += (long long)gridDim.x * 64) {
    const long long r = todo ? todo[it] : it;
    const int len = read_len[r];
    const uint8_t* q = read_pool + read_off[r];
    bpsw_smem_t* o = row_base ? out + row_base[it] : out + (size_t)it * (size_t)stride;
    const int room = row_base ? (int)(row_base[it + 1] - row_base[it]) : stride;
    int n_out = 0;
    auto emit = [&](const Intv& v) {
      if (n_out < room) {
        bpsw_smem_t e;
        e.x0 = (int64_t)v.x0; e.x1 = (int64_t)v.x1; e.x2 = (int64_t)v.x2;
        e.qbeg = (int)(v.info >> 32); e.qend = (int)(unsigned)v.info;
        e.kept = !(e.qend - e.qbeg < P.min_seed_len || v.x2 > (u64)P.max_occ);
        e.pad_ = 0;
        o[n_out] = e;
      }
      ++n_out;
    };
    if (len >= P.min_seed_len && len <= list_cap - 1) {  // mem_chain: a query shorter than the seed length has no match
      const int split_len = P.split_len0 < len ? P.split_len0 : len;
      int start = 0;
      for (;;) {
        while (start < len && q[start] > 3) ++start;  // skip ambiguous bases
        if (start >= len) break;
        const int ori_start = start;
        start = smem1(F, len, q, ori_start, (u64)P.start_width, M, T0, T1);
        if (M.n == 0) continue;
        int max = 0, max_i = 0;
        for (int i = 0; i < M.n; ++i) {
          const Intv p = M.get(i);
          const int l = (int)((unsigned)p.info - (unsigned)(p.info >> 32));
          if (max < l) { max = l; max_i = i; }
        }
        const Intv best = M.get(max_i);
        if (split_len > 0 && max >= split_len && best.x2 <= (u64)P.split_width) {  // re-seed from the middle of the longest SMEM
          smem1(F, len, q, (int)(((unsigned)best.info + (unsigned)(best.info >> 32)) >> 1), best.x2 + 1, S, T0, T1);
          int i = 0, j = 0;
          auto sub_ok = [&](const Intv& s) {
            return (int)((unsigned)s.info - (unsigned)(s.info >> 32)) >= (max >> 1) && (int)(unsigned)s.info > ori_start;
          };
          while (i < M.n && j < S.n) {  // ordered merge
            const Intv a = M.get(i), b = S.get(j);
            const long long xi = (long long)(a.info >> 32 << 32 | (u64)(len - (int)(unsigned)a.info));
            const long long xj = (long long)(b.info >> 32 << 32 | (u64)(len - (int)(unsigned)b.info));
            if (xi < xj) { emit(a); ++i; }
            else { if (sub_ok(b)) emit(b); ++j; }
          }
          for (; i < M.n; ++i) emit(M.get(i));
          for (; j < S.n; ++j) { const Intv b = S.get(j); if (sub_ok(b)) emit(b); }
        } else {
          for (int i = 0; i < M.n; ++i) emit(M.get(i));
        }
      }
    }
    cnt[it] = n_out;
  }
}

// bwt_sa(x0 + k), native/bwt.c:85-95 with bwt_invPsi (:52-58), one occurrence per lane.  Occurrence t belongs to the kept
// interval whose base (prefix sum of x2) is the last one <= t: a binary search over occ_base[0 .. n_kept].
__global__ __launch_bounds__(256) void seed_sa_kernel(FmiDev F, long long n_occ, int n_kept, const long long* __restrict__ occ_base,
                                                      const long long* __restrict__ kept_x0, const int2* __restrict__ kept_q,
                                                      bpsw_seed_t* out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_occ) return;
  int lo = 0, hi = n_kept - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (occ_base[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  u64 k = (u64)kept_x0[lo] + (u64)(t - occ_base[lo]);
  const u64 mask = ((u64)1 << F.sa_shift) - 1;
  u64 sa = 0;
  while ((k & mask) && sa <= F.seq_len) {  // (a valid index reaches a sampled row within seq_len steps)
    ++sa;
    if (k == F.primary) { k = 0; continue; }
    k = k > F.seq_len ? F.seq_len : k;
    const u64 x = k - (k > F.primary);
    const uint32_t w = F.bwt[((x >> 7) << 4) + 8 + ((x & 0x7f) >> 4)];
    const int c = (int)(w >> ((~x & 0xf) << 1) & 3);
    k = F.L2[c] + occ1(F, k, c);
  }
  const int2 qq = kept_q[lo];
  bpsw_seed_t s;
  s.rbeg = (int64_t)(sa + (u64)F.sa[k >> F.sa_shift]);
  s.qbeg = qq.x;
  s.len = qq.y - qq.x;
  out[t] = s;
}

// ---- the plan of the suffix-array pass on the device (BPSW_SEED_PLAN_DEVICE), one read per lane ---------------------------------------
// What seed_run's loop over the intervals computes on the calling thread, from the rows where seed_smem_kernel left them
// (bpsw_seed_plan_core.h): seed_plan_count_kernel writes per read the number of kept intervals and the sum of their x2, the scan of
// bpsw_scan.hip turns both columns into kept_base[] and read_occ[] with the totals in entry n, and seed_plan_fill_kernel writes the
// three tables seed_sa_kernel reads.  flags[1] is set when the second pass counted another number of intervals than the first.
__global__ __launch_bounds__(256) void seed_plan_count_kernel(SeedPlanRows R, int n, const int32_t* __restrict__ cnt2, int* flags,
                                                              long long* __restrict__ n_kept, long long* __restrict__ n_occ) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  if (R.cnt[r] > R.stride && cnt2[seed_plan_todo_index(R, r)] != R.cnt[r]) flags[1] = 1;
  seed_plan_count(R, r, n_kept + r, n_occ + r);
}
__global__ __launch_bounds__(256) void seed_plan_fill_kernel(SeedPlanRows R, int n, const long long* __restrict__ kept_base,
                                                             const long long* __restrict__ read_occ, long long* __restrict__ occ_base,
                                                             long long* __restrict__ kept_x0, int32_t* __restrict__ kept_q) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) occ_base[kept_base[n]] = read_occ[n];  // the end of the last interval: seed_sa_kernel's search stops below it
  if (r >= n) return;
  seed_plan_fill(R, r, kept_base[r], read_occ[r], occ_base, kept_x0, kept_q);
}

// ---- the index, per device --------------------------------------------------------------------------------------------
struct DeviceFmi {
  RefGate gate;
  std::mutex mu;
  DeviceBuffer bwt, sa;
  FmiDev dev{};
  long long seq_len = 0;
};
DeviceFmi& device_fmi(int device) {
  static DeviceFmi table[64];
  return table[device >= 0 && device < 64 ? device : 0];
}

// lanes of seed_smem_kernel resident at a time: four wavefronts per compute unit (one per SIMD), each lane with four lists of
// read_len + 1 intervals of 32 bytes -- 32.9 KB a lane at 256 bases, 2.2 GB on 256 CUs; 1.3 GB at 150 bases.
// bpsw_seed_set_resident_lanes (diagnostics, include/bpsw.h) overrides the count.
std::atomic<int> g_seed_lanes{0};
int seed_resident_waves(int num_cu, long long n_reads) {
  const long long forced = g_seed_lanes.load(std::memory_order_relaxed) / 64;
  long long waves = forced >= 1 ? forced : (long long)num_cu * 4;
  const long long need = (n_reads + 63) / 64;
  return (int)(need < waves ? need : waves);
}

thread_local double t_w1_ms[3] = {0., 0., 0.};
thread_local int64_t t_seed_bytes[2] = {0, 0};  // H2D, D2H of the calling thread's last seed_run (bpsw_last_seed_bytes)

// seeding of a validated batch: per read the intervals and the seeds (bridging ones dropped), concatenated in read order.
// With dev_read_occ (the caller then holds c->mu through a ContextEntry of its own): the seeds stay where seed_sa_kernel wrote them,
// at the start of c->d_seed[4], bridging ones included -- read r's are [dev_read_occ[r], dev_read_occ[r + 1]) --, and scnt / seeds
// come back empty.
// With plan_dev the tables of the suffix-array pass are made on the device from the interval rows (seed_plan_*_kernel and the scan):
// the rows come back only with want_intv, for the caller; otherwise intv comes back empty.
int seed_run(bpsw_ctx* c, const bpsw_seed_opt_t& so, const bpsw_reads_t& R, std::vector<int32_t>* icnt, std::vector<bpsw_smem_t>* intv,
             std::vector<int32_t>* scnt, std::vector<bpsw_seed_t>* seeds, std::vector<long long>* dev_read_occ = nullptr,
             bool plan_dev = false, bool want_intv = true) {
  const int n = R.n_reads;
  t_seed_bytes[0] = t_seed_bytes[1] = 0;
  int max_len = 1;
  for (int r = 0; r < n; ++r) {
    const int ql = R.read_len[r];
    const long long qo = R.read_off[r];
    if (ql < 0 || qo < 0 || (unsigned long long)(qo + ql) > R.read_pool_bytes) return fail(BPSW_ERR_ARG, "seed: read outside read_pool");
    if (ql > BPSW_SEED_MAX_QLEN) return fail(BPSW_ERR_LIMIT, "seed: read longer than 256 bases");
    if (ql > max_len) max_len = ql;
  }
  if (so.min_seed_len < 1 || so.max_occ < 0 || so.split_width < 0) return fail(BPSW_ERR_ARG, "seed: min_seed_len must be >= 1, max_occ and split_width >= 0");
  std::optional<ContextEntry> entry;
  if (!dev_read_occ) {
    entry.emplace(c);
    if (entry->rc != BPSW_OK) return entry->rc;
  }
  DeviceFmi& fm = device_fmi(c->device);
  const RefHold hold(&fm.gate);
  FmiDev F;
  { std::lock_guard<std::mutex> g(fm.mu); F = fm.dev; }
  if (F.seq_len == 0) return fail(BPSW_ERR_ARG, "seed: no index is loaded (bpsw_fmi_load)");
  const u64 l_pac = F.seq_len >> 1;

  DeviceBuffer &d_in = c->d_seed[0], &d_out = c->d_seed[1], &d_arena = c->d_seed[2], &d_sa_in = c->d_seed[3], &d_sa_out = c->d_seed[4];
  SeedParams P;
  P.min_seed_len = so.min_seed_len; P.max_occ = so.max_occ; P.split_width = so.split_width;
  P.start_width = so.no_exact ? 2 : 1;
  P.split_len0 = (int)(so.min_seed_len * so.split_factor + .499);

  // ---- intervals ----
  StageIn in;
  const int i_len = in.add(R.read_len, 4 * (size_t)n), i_off = in.add(R.read_off, 8 * (size_t)n);
  const int i_pool = in.add(R.read_pool, R.read_pool_bytes);
  in.add(nullptr, 16);  // room behind the pool
  HIP_TRY(in.stage(c->h_stage_in, d_in, c->stream));
  t_seed_bytes[0] += (int64_t)in.total();
  const int waves = seed_resident_waves(c->num_cu, n);
  const int list_cap = max_len + 1;
  HIP_TRY(d_arena.reserve((size_t)waves * 4 * (size_t)list_cap * 64 * sizeof(Intv)));
  // what seed_sa_kernel reads: staged from the calling thread's loop over the intervals, or written by the plan kernels
  const long long *d_occ_base = nullptr, *d_kept_x0 = nullptr;
  const int2* d_kept_q = nullptr;
  size_t nk = 0;
  long long n_occ = 0;
  std::vector<long long> read_occ((size_t)n + 1, 0);
  // first pass: rows of 16 records (a read of 150 bases has about five intervals); the reads that produced more are run once more
  // by themselves, each with exactly the room its count asks for -- so the records of a batch never take more than
  // 16 n + (the intervals of the overflowing reads), whatever one repeat-rich read produces
  const int stride = 16;
  {
    StageOut out;
    const int r_cnt = out.add(4 * (size_t)n), r_ovf = out.add(16), r_rec = out.add(sizeof(bpsw_smem_t) * (size_t)n * (size_t)stride);
    HIP_TRY(out.reserve(c->h_stage_out, d_out));
    HIP_TRY(hipMemsetAsync(out.dev<int>(r_ovf), 0, 16, c->stream));
    hipLaunchKernelGGL(seed_smem_kernel, dim3((unsigned)waves), dim3(64), 0, c->stream, F, P, n, (const int32_t*)nullptr,
                       in.dev<int32_t>(i_len), in.dev<long long>(i_off), in.dev<uint8_t>(i_pool), (Intv*)d_arena.ptr, list_cap,
                       out.dev<bpsw_smem_t>(r_rec), stride, (const long long*)nullptr, out.dev<int32_t>(r_cnt), out.dev<int>(r_ovf));
    HIP_TRY(hipGetLastError());
    if (plan_dev) {
      // Only the counts and the overflow word come back; the rows stay in d_out for the plan kernels.
      //   d_seed[1] (d_out)    cnt | overflow word | first-pass rows                    until seed_plan_fill_kernel has run
      //   d_seed[4] (d_sa_out) the second pass's rows                                     until seed_plan_fill_kernel has run; then
      //                        seed_sa_kernel's seeds (both plan kernels have been waited for before it is reserved again)
      //   d_seed[3] (d_sa_in)  todo | base (staged) | cnt2 | n_kept[n + 1] n_occ[n + 1] | flags | tile sums | occ_base kept_x0 kept_q
      //                        until seed_sa_kernel has run; nothing is staged over it for the suffix-array pass
      const size_t head = out.at[r_rec];
      HIP_TRY(hipMemcpyAsync(out.h, out.d, head, hipMemcpyDeviceToHost, c->stream));
      t_seed_bytes[1] += (int64_t)head;
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (*out.host<int>(r_ovf)) return fail(BPSW_ERR_DEVICE, "seed: an interval list outgrew read_len + 1 entries");
      const int32_t* cnt = out.host<int32_t>(r_cnt);
      icnt->assign(cnt, cnt + n);  // (the pinned block is reserved again below: cnt is not read after this)
      std::vector<int32_t> todo;
      std::vector<long long> base(1, 0);
      long long n_intv = 0;
      for (int r = 0; r < n; ++r) {
        n_intv += (*icnt)[(size_t)r];
        if ((*icnt)[(size_t)r] > stride) { todo.push_back(r); base.push_back(base.back() + (*icnt)[(size_t)r]); }
      }
      const size_t m = todo.size();
      const int tile = scan_tile_items();
      const long long tiles = scan_tiles(n, tile);
      StageLayout L;
      const size_t o_todo = L.add(4 * m), o_base = L.add(8 * (m + 1)), table_bytes = L.total();
      const size_t o_cnt2 = L.add(4 * m), o_cols = L.add(8 * 2 * ((size_t)n + 1)), o_flags = L.add(16);  // (the flags lie right behind the columns)
      const size_t o_tiles = L.add(8 * 2 * (size_t)tiles), o_occ = L.add(8 * ((size_t)n_intv + 1)), o_x0 = L.add(8 * (size_t)n_intv);
      const size_t o_q = L.add(8 * (size_t)n_intv);
      HIP_TRY(d_sa_in.reserve(L.total()));
      uint8_t* D = (uint8_t*)d_sa_in.ptr;
      int* d_flags = (int*)(D + o_flags);  // [0] a list of the second pass outgrew its room, [1] interval counts changed between two runs
      HIP_TRY(hipMemsetAsync(d_flags, 0, 16, c->stream));
      if (m) {
        HIP_TRY(c->h_stage_in.reserve(table_bytes));  // (the reads have arrived: the stream was waited for)
        uint8_t* hp = (uint8_t*)c->h_stage_in.ptr;
        memcpy(hp + o_todo, todo.data(), 4 * m);
        memcpy(hp + o_base, base.data(), 8 * (m + 1));
        HIP_TRY(hipMemcpyAsync(D, hp, table_bytes, hipMemcpyHostToDevice, c->stream));
        t_seed_bytes[0] += (int64_t)table_bytes;
        HIP_TRY(d_sa_out.reserve(sizeof(bpsw_smem_t) * (size_t)base.back()));
        const int waves2 = seed_resident_waves(c->num_cu, (long long)m);
        hipLaunchKernelGGL(seed_smem_kernel, dim3((unsigned)waves2), dim3(64), 0, c->stream, F, P, (int)m, (const int32_t*)(D + o_todo),
                           in.dev<int32_t>(i_len), in.dev<long long>(i_off), in.dev<uint8_t>(i_pool), (Intv*)d_arena.ptr, list_cap,
                           (bpsw_smem_t*)d_sa_out.ptr, 0, (const long long*)(D + o_base), (int32_t*)(D + o_cnt2), d_flags);
        HIP_TRY(hipGetLastError());
      }
      SeedPlanRows PR;
      PR.cnt = out.dev<int32_t>(r_cnt); PR.first = out.dev<bpsw_smem_t>(r_rec); PR.stride = stride;
      PR.todo = (const int32_t*)(D + o_todo); PR.n_todo = (int)m; PR.base = (const long long*)(D + o_base);
      PR.more = (const bpsw_smem_t*)d_sa_out.ptr;
      long long* cols = (long long*)(D + o_cols);  // n_kept[0 .. n] then n_occ[0 .. n]; after the scan kept_base[] and read_occ[]
      const unsigned plan_blocks = (unsigned)((n + 255) / 256);
      hipLaunchKernelGGL(seed_plan_count_kernel, dim3(plan_blocks), dim3(256), 0, c->stream, PR, n, (const int32_t*)(D + o_cnt2), d_flags, cols,
                         cols + n + 1);
      HIP_TRY(hipGetLastError());
      HIP_TRY(scan_exclusive_i64(c->stream, cols, 2, n, tile, (long long*)(D + o_tiles)));
      hipLaunchKernelGGL(seed_plan_fill_kernel, dim3(plan_blocks), dim3(256), 0, c->stream, PR, n, (const long long*)cols,
                         (const long long*)(cols + n + 1), (long long*)(D + o_occ), (long long*)(D + o_x0), (int32_t*)(D + o_q));
      HIP_TRY(hipGetLastError());
      // back: n_kept | read_occ[0 .. n] | flags, one copy; the rows only for a caller that asked for them
      const size_t tail_bytes = 8 + 8 * ((size_t)n + 1) + 16, rec1_bytes = sizeof(bpsw_smem_t) * (size_t)n * (size_t)stride;
      const size_t rec2_bytes = sizeof(bpsw_smem_t) * (size_t)base.back();
      StageLayout H;
      const size_t h_tail = H.add(tail_bytes), h_rec1 = H.add(want_intv ? rec1_bytes : 0), h_rec2 = H.add(want_intv ? rec2_bytes : 0);
      HIP_TRY(c->h_stage_out.reserve(H.total()));
      const uint8_t* hp = (const uint8_t*)c->h_stage_out.ptr;
      HIP_TRY(hipMemcpyAsync((void*)(hp + h_tail), cols + n, tail_bytes, hipMemcpyDeviceToHost, c->stream));
      t_seed_bytes[1] += (int64_t)tail_bytes;
      if (want_intv) {
        HIP_TRY(hipMemcpyAsync((void*)(hp + h_rec1), PR.first, rec1_bytes, hipMemcpyDeviceToHost, c->stream));
        if (m) HIP_TRY(hipMemcpyAsync((void*)(hp + h_rec2), PR.more, rec2_bytes, hipMemcpyDeviceToHost, c->stream));
        t_seed_bytes[1] += (int64_t)(rec1_bytes + rec2_bytes);
      }
      HIP_TRY(hipStreamSynchronize(c->stream));
      const long long* tail = (const long long*)(hp + h_tail);
      const int* fl = (const int*)(tail + n + 2);
      if (fl[0]) return fail(BPSW_ERR_DEVICE, "seed: an interval list outgrew read_len + 1 entries");
      if (fl[1]) return fail(BPSW_ERR_DEVICE, "seed: interval counts changed between two runs");
      nk = (size_t)tail[0];
      memcpy(read_occ.data(), tail + 1, 8 * ((size_t)n + 1));
      n_occ = read_occ[(size_t)n];
      d_occ_base = (const long long*)(D + o_occ); d_kept_x0 = (const long long*)(D + o_x0); d_kept_q = (const int2*)(D + o_q);
      intv->clear();
      if (want_intv) {
        const bpsw_smem_t *rec = (const bpsw_smem_t*)(hp + h_rec1), *more = (const bpsw_smem_t*)(hp + h_rec2);
        size_t ti = 0;
        for (int r = 0; r < n; ++r) {
          const int k = (*icnt)[(size_t)r];
          if (k <= stride) intv->insert(intv->end(), rec + (size_t)r * (size_t)stride, rec + (size_t)r * (size_t)stride + k);
          else { intv->insert(intv->end(), more + base[ti], more + base[ti] + k); ++ti; }
        }
      }
    } else {
      HIP_TRY(out.fetch(c->stream));
      t_seed_bytes[1] += (int64_t)out.total();
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (*out.host<int>(r_ovf)) return fail(BPSW_ERR_DEVICE, "seed: an interval list outgrew read_len + 1 entries");
      const int32_t* cnt = out.host<int32_t>(r_cnt);
      icnt->assign(cnt, cnt + n);
      std::vector<int32_t> todo;
      std::vector<long long> base(1, 0);
      for (int r = 0; r < n; ++r)
        if (cnt[r] > stride) { todo.push_back(r); base.push_back(base.back() + cnt[r]); }
      std::vector<bpsw_smem_t> first;  // the first pass's rows, taken out of the pinned block before the second pass reuses it
      const bpsw_smem_t* rec = out.host<bpsw_smem_t>(r_rec);
      const bpsw_smem_t* more = nullptr;
      if (!todo.empty()) {
        first.assign(rec, rec + (size_t)n * (size_t)stride);
        rec = first.data();
        const size_t m = todo.size();
        StageIn in2;
        const int i_todo = in2.add(todo.data(), 4 * m), i_base = in2.add(base.data(), 8 * (m + 1));
        StageOut out2;
        const int r2_cnt = out2.add(4 * m), r2_ovf = out2.add(16), r2_rec = out2.add(sizeof(bpsw_smem_t) * (size_t)base.back());
        HIP_TRY(out2.reserve(c->h_stage_out, d_out));
        HIP_TRY(in2.stage(c->h_stage_in, d_sa_in, c->stream));
        t_seed_bytes[0] += (int64_t)in2.total();
        HIP_TRY(hipMemsetAsync(out2.dev<int>(r2_ovf), 0, 16, c->stream));
        const int waves2 = seed_resident_waves(c->num_cu, (long long)m);
        hipLaunchKernelGGL(seed_smem_kernel, dim3((unsigned)waves2), dim3(64), 0, c->stream, F, P, (int)m, in2.dev<int32_t>(i_todo),
                           in.dev<int32_t>(i_len), in.dev<long long>(i_off), in.dev<uint8_t>(i_pool), (Intv*)d_arena.ptr, list_cap,
                           out2.dev<bpsw_smem_t>(r2_rec), 0, in2.dev<long long>(i_base), out2.dev<int32_t>(r2_cnt), out2.dev<int>(r2_ovf));
        HIP_TRY(hipGetLastError());
        HIP_TRY(out2.fetch(c->stream));
        t_seed_bytes[1] += (int64_t)out2.total();
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int32_t* cnt2 = out2.host<int32_t>(r2_cnt);
        for (size_t i = 0; i < m; ++i)
          if (cnt2[i] != (*icnt)[(size_t)todo[i]]) return fail(BPSW_ERR_DEVICE, "seed: interval counts changed between two runs");
        more = out2.host<bpsw_smem_t>(r2_rec);
      }
      intv->clear();
      size_t ti = 0;
      for (int r = 0; r < n; ++r) {
        const int m = (*icnt)[(size_t)r];
        if (m <= stride) intv->insert(intv->end(), rec + (size_t)r * (size_t)stride, rec + (size_t)r * (size_t)stride + m);
        else { intv->insert(intv->end(), more + base[ti], more + base[ti] + m); ++ti; }
      }
    }
  }

  // ---- seeds: one occurrence per lane, offsets from the prefix sum of the kept intervals' x2 ----
  std::vector<long long> occ_base, kept_x0;
  std::vector<int32_t> kept_q;
  if (!plan_dev) {
    size_t at = 0;
    for (int r = 0; r < n; ++r) {
      read_occ[(size_t)r] = n_occ;
      for (int k = 0; k < (*icnt)[(size_t)r]; ++k, ++at) {
        const bpsw_smem_t& e = (*intv)[at];
        if (!e.kept) continue;
        occ_base.push_back(n_occ); kept_x0.push_back(e.x0);
        kept_q.push_back(e.qbeg); kept_q.push_back(e.qend);
        n_occ += e.x2;
      }
    }
    read_occ[(size_t)n] = n_occ;
  }
  scnt->assign((size_t)n, 0);
  seeds->clear();
  if (dev_read_occ) *dev_read_occ = read_occ;
  if (n_occ == 0) return BPSW_OK;
  if (n_occ > 0x3fffffffll) return fail(BPSW_ERR_LIMIT, "seed: more than 2^30 seed occurrences in one batch");
  StageOut sout;
  const int r_seeds = sout.add(sizeof(bpsw_seed_t) * (size_t)n_occ);
  if (dev_read_occ) HIP_TRY(d_sa_out.reserve(sout.total()));
  else HIP_TRY(sout.reserve(c->h_stage_out, d_sa_out));
  StageIn sin;
  if (!plan_dev) {
    nk = occ_base.size();
    occ_base.push_back(n_occ);
    const int i_base = sin.add(occ_base.data(), 8 * (nk + 1)), i_x0 = sin.add(kept_x0.data(), 8 * nk), i_q = sin.add(kept_q.data(), 8 * nk);
    HIP_TRY(sin.stage(c->h_stage_in, d_sa_in, c->stream));
    t_seed_bytes[0] += (int64_t)sin.total();
    d_occ_base = sin.dev<long long>(i_base); d_kept_x0 = sin.dev<long long>(i_x0); d_kept_q = sin.dev<int2>(i_q);
  }
  hipLaunchKernelGGL(seed_sa_kernel, dim3((unsigned)((n_occ + 255) / 256)), dim3(256), 0, c->stream, F, n_occ, (int)nk, d_occ_base, d_kept_x0,
                     d_kept_q, (bpsw_seed_t*)d_sa_out.ptr);
  HIP_TRY(hipGetLastError());
  if (!dev_read_occ) {
    HIP_TRY(sout.fetch(c->stream));
    t_seed_bytes[1] += (int64_t)sout.total();
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (dev_read_occ) return BPSW_OK;
  const bpsw_seed_t* all = sout.host<bpsw_seed_t>(r_seeds);
  seeds->reserve((size_t)n_occ);
  for (int r = 0; r < n; ++r) {
    int m = 0;
    for (long long t = read_occ[(size_t)r]; t < read_occ[(size_t)r + 1]; ++t) {
      const bpsw_seed_t& s = all[t];
      if ((u64)s.rbeg < l_pac && l_pac < (u64)s.rbeg + (u64)s.len) continue;  // bridging the strands, native/bwamem.c:228
      seeds->push_back(s);
      ++m;
    }
    (*scnt)[(size_t)r] = m;
  }
  return BPSW_OK;
}

int check_reads(const char* who, const bpsw_reads_t* R) {
  if (!R || R->n_reads < 0 || (R->n_reads > 0 && (!R->read_len || !R->read_off || (!R->read_pool && R->read_pool_bytes))))
    return fail(BPSW_ERR_ARG, std::string(who) + ": null read arrays");
  return BPSW_OK;
}

}  // namespace

namespace bpsw {

int fmi_adopt(bpsw_ctx* c, DeviceBuffer* bwt, DeviceBuffer* sa, long long primary, const long long L2[5], long long seq_len, int sa_intv) {
  DeviceFmi& fm = device_fmi(c->device);
  RefWriteHold wr(&fm.gate);
  std::lock_guard<std::mutex> g(fm.mu);
  RingPause ring_paused(c->device);
  HIP_TRY(hipDeviceSynchronize());  // nothing in flight may still read the previous index
  std::swap(fm.bwt, *bwt);
  std::swap(fm.sa, *sa);
  FmiDev F;
  F.bwt = (const uint32_t*)fm.bwt.ptr; F.sa = (const long long*)fm.sa.ptr;
  F.primary = (u64)primary; F.seq_len = (u64)seq_len;
  for (int i = 0; i < 5; ++i) F.L2[i] = (u64)L2[i];
  F.sa_shift = 0;
  while ((1 << F.sa_shift) < sa_intv) ++F.sa_shift;
  fm.dev = F;
  fm.seq_len = seq_len;
  return BPSW_OK;
}

}  // namespace bpsw

extern "C" {

int bpsw_fmi_load(bpsw_ctx_t* c, int64_t primary, const int64_t L2[5], int64_t seq_len, const uint32_t* bwt, int64_t bwt_size,
                  int32_t sa_intv, int64_t n_sa, const int64_t* sa) {
  if (!c || !L2 || !bwt || !sa || seq_len < 1) return fail(BPSW_ERR_ARG, "fmi_load: null argument or empty index");
  if (seq_len > (int64_t)1 << 41) return fail(BPSW_ERR_LIMIT, "fmi_load: index longer than 2^41 bases");
  if (bwt_size != (seq_len + 15) / 16 + ((seq_len + 127) / 128 + 1) * 8) return fail(BPSW_ERR_ARG, "fmi_load: bwt_size does not fit seq_len");
  if (sa_intv < 1 || (sa_intv & (sa_intv - 1))) return fail(BPSW_ERR_ARG, "fmi_load: sa_intv is not a power of two");
  if (n_sa != (seq_len + sa_intv) / sa_intv) return fail(BPSW_ERR_ARG, "fmi_load: n_sa is not (seq_len + sa_intv) / sa_intv");
  if (primary < 0 || primary > seq_len || L2[0] != 0 || L2[4] != seq_len) return fail(BPSW_ERR_ARG, "fmi_load: primary or L2 outside the index");
  for (int i = 0; i < 4; ++i)
    if (L2[i] > L2[i + 1]) return fail(BPSW_ERR_ARG, "fmi_load: L2 is not cumulative");
  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  DeviceFmi& fm = device_fmi(c->device);
  RefWriteHold wr(&fm.gate);
  std::lock_guard<std::mutex> g(fm.mu);
  RingPause ring_paused(c->device);
  HIP_TRY(hipDeviceSynchronize());  // nothing in flight may still read the previous index
  fm.dev = FmiDev{};
  fm.seq_len = 0;
  const size_t bwt_bytes = 4 * (size_t)bwt_size;
  HIP_TRY(fm.bwt.reserve(bwt_bytes + 64));  // a whole 64-byte block may be read where the array ends inside one
  HIP_TRY(fm.sa.reserve(8 * (size_t)n_sa));
  HIP_TRY(hipMemset((uint8_t*)fm.bwt.ptr + bwt_bytes, 0, 64));
  HIP_TRY(hipMemcpy(fm.bwt.ptr, bwt, bwt_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(fm.sa.ptr, sa, 8 * (size_t)n_sa, hipMemcpyHostToDevice));
  FmiDev F;
  F.bwt = (const uint32_t*)fm.bwt.ptr; F.sa = (const long long*)fm.sa.ptr;
  F.primary = (u64)primary; F.seq_len = (u64)seq_len;
  for (int i = 0; i < 5; ++i) F.L2[i] = (u64)L2[i];
  F.sa_shift = 0;
  while ((1 << F.sa_shift) < sa_intv) ++F.sa_shift;
  fm.dev = F;
  fm.seq_len = seq_len;
  return BPSW_OK;
}

int bpsw_fmi_unload(bpsw_ctx_t* c) {
  if (!c) return fail(BPSW_ERR_ARG, "null context");
  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  DeviceFmi& fm = device_fmi(c->device);
  RefWriteHold wr(&fm.gate);
  std::lock_guard<std::mutex> g(fm.mu);
  RingPause ring_paused(c->device);
  HIP_TRY(hipDeviceSynchronize());
  fm.bwt.release();
  fm.sa.release();
  fm.dev = FmiDev{};
  fm.seq_len = 0;
  return BPSW_OK;
}

int64_t bpsw_fmi_length(const bpsw_ctx_t* c) {
  if (!c) return 0;
  DeviceFmi& fm = device_fmi(c->device);
  const RefHold hold(&fm.gate);
  std::lock_guard<std::mutex> g(fm.mu);
  return (int64_t)fm.seq_len;
}

int bpsw_seed_batch(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, const bpsw_reads_t* reads, int32_t* intv_cnt, bpsw_smem_t* intv,
                    int64_t intv_cap, int64_t* intv_total, int32_t* seed_cnt, bpsw_seed_t* seeds, int64_t seed_cap, int64_t* seed_total) {
  if (!c || !sopt || !intv_cnt || !intv_total || !seed_cnt || !seed_total) return fail(BPSW_ERR_ARG, "seed_batch: null argument");
  int rc = check_reads("seed_batch", reads);
  if (rc != BPSW_OK) return rc;
  *intv_total = *seed_total = 0;
  if (reads->n_reads == 0) return BPSW_OK;
  std::vector<int32_t> ic, sc;
  std::vector<bpsw_smem_t> iv;
  std::vector<bpsw_seed_t> sv;
  rc = seed_run(c, *sopt, *reads, &ic, &iv, &sc, &sv);
  if (rc != BPSW_OK) return rc;
  *intv_total = (int64_t)iv.size();
  *seed_total = (int64_t)sv.size();
  if ((int64_t)iv.size() > intv_cap || (int64_t)sv.size() > seed_cap || (!iv.empty() && !intv) || (!sv.empty() && !seeds))
    return fail(BPSW_ERR_CAPACITY, "seed_batch: intv / seeds too small (the totals say what is needed)");
  memcpy(intv_cnt, ic.data(), 4 * ic.size());
  memcpy(seed_cnt, sc.data(), 4 * sc.size());
  if (!iv.empty()) memcpy(intv, iv.data(), sizeof(bpsw_smem_t) * iv.size());
  if (!sv.empty()) memcpy(seeds, sv.data(), sizeof(bpsw_seed_t) * sv.size());
  return BPSW_OK;
}

int bpsw_seed_batch_ex(bpsw_ctx_t* c, const bpsw_seed_opt_t* sopt, const bpsw_reads_t* reads, int32_t* intv_cnt, bpsw_smem_t* intv,
                       int64_t intv_cap, int64_t* intv_total, int32_t* seed_cnt, bpsw_seed_t* seeds, int64_t seed_cap, int64_t* seed_total,
                       int flags) {
  if (flags == 0) return bpsw_seed_batch(c, sopt, reads, intv_cnt, intv, intv_cap, intv_total, seed_cnt, seeds, seed_cap, seed_total);
  if (flags & ~BPSW_SEED_PLAN_DEVICE) return fail(BPSW_ERR_ARG, "seed_batch_ex: unknown flag");
  if (!c || !sopt || !intv_cnt || !intv_total || !seed_cnt || !seed_total) return fail(BPSW_ERR_ARG, "seed_batch_ex: null argument");
  int rc = check_reads("seed_batch_ex", reads);
  if (rc != BPSW_OK) return rc;
  *intv_total = *seed_total = 0;
  if (reads->n_reads == 0) return BPSW_OK;
  std::vector<int32_t> ic, sc;
  std::vector<bpsw_smem_t> iv;
  std::vector<bpsw_seed_t> sv;
  rc = seed_run(c, *sopt, *reads, &ic, &iv, &sc, &sv, nullptr, true, intv != nullptr);  // intv null: no interval leaves the device
  if (rc != BPSW_OK) return rc;
  for (const int32_t k : ic) *intv_total += k;
  *seed_total = (int64_t)sv.size();
  if ((intv && *intv_total > intv_cap) || (int64_t)sv.size() > seed_cap || (!sv.empty() && !seeds))
    return fail(BPSW_ERR_CAPACITY, "seed_batch_ex: intv / seeds too small (the totals say what is needed)");
  memcpy(intv_cnt, ic.data(), 4 * ic.size());
  memcpy(seed_cnt, sc.data(), 4 * sc.size());
  if (!iv.empty()) memcpy(intv, iv.data(), sizeof(bpsw_smem_t) * iv.size());
  if (!sv.empty()) memcpy(seeds, sv.data(), sizeof(bpsw_seed_t) * sv.size());
  return BPSW_OK;
}

int bpsw_worker1_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_reads_t* reads, int zdrop_mode,
                       int flags, int32_t* out_cnt, bpsw_alnreg_t* out_regs, int64_t out_cap, int64_t* out_total) {
  if (!c || !opt || !sopt || !out_cnt || !out_total) return fail(BPSW_ERR_ARG, "worker1: null argument");
  int rc = check_reads("worker1", reads);
  if (rc != BPSW_OK) return rc;
  *out_total = 0;
  const int n = reads->n_reads;
  if (n == 0) return BPSW_OK;
  const int64_t l_pac = bpsw_ref_length(c);
  if (l_pac <= 0) return fail(BPSW_ERR_ARG, "worker1: no reference is loaded (bpsw_ref_load)");
  if (bpsw_fmi_length(c) != 2 * l_pac) return fail(BPSW_ERR_ARG, "worker1: no index is loaded, or its seq_len is not 2 * l_pac (bpsw_fmi_load)");
  for (int r = 0; r < n; ++r)
    if (reads->read_len[r] < 1) return fail(BPSW_ERR_ARG, "worker1: empty read");
  const bool chains_resident = (flags & BPSW_W1_CHAINS_RESIDENT) != 0;
  const bool chain_on_device = chains_resident || (flags & BPSW_W1_CHAIN_DEVICE) != 0, plan_on_device = (flags & BPSW_W1_SEED_PLAN_DEVICE) != 0;
  flags &= ~(BPSW_W1_CHAIN_DEVICE | BPSW_W1_SEED_PLAN_DEVICE | BPSW_W1_CHAINS_RESIDENT);
  const double t0 = wall_ms();
  std::vector<int32_t> ic, sc;
  std::vector<bpsw_smem_t> iv;
  std::vector<bpsw_seed_t> sv;
  std::vector<int32_t> chain_cnt((size_t)n), seed_cnt, qbeg, len, cc;
  std::vector<int64_t> rbeg;
  std::vector<bpsw_seed_t> cs;
  double t1;
  if (chain_on_device) {
    // the seeds stay in d_seed[4]; chaining + filter by chain_kernel (bpsw_chain_dev.hip), which drops the bridging ones itself
    ContextEntry entry(c);
    if (entry.rc != BPSW_OK) return entry.rc;
    std::vector<long long> read_occ;
    rc = seed_run(c, *sopt, *reads, &ic, &iv, &sc, &sv, &read_occ, plan_on_device, false);
    if (rc != BPSW_OK) return rc;
    t1 = wall_ms();
    ChainDevJob J;
    J.n_reads = n; J.seed_beg = read_occ.data(); J.d_seeds = (const bpsw_seed_t*)c->d_seed[4].ptr; J.h_seeds = nullptr;
    J.filter = 1; J.drop_bridging = 1;
    if (chains_resident) {
      // the chains stay where chain_tables_kernel left them (d_chain_tab); only the read block is staged for the round loop, whose
      // back half runs under this call's hold on the context.  The seeds are the library's own: not validated again.
      ChainTablesDev T;
      rc = chain_dev_run(c, *sopt, opt->w, l_pac, J, nullptr, &T);
      if (rc != BPSW_OK) return rc;
      const double t2 = wall_ms();
      rc = chain2aln_check(opt, zdrop_mode, n, reads->read_len, reads->read_off, reads->read_pool_bytes);
      if (rc != BPSW_OK) return rc;
      const uint8_t* d_pac = nullptr;
      long long ref_len = 0;
      const RefHold ref_hold = ref_snapshot(c, &d_pac, &ref_len);
      if (ref_len != l_pac) return fail(BPSW_ERR_ARG, "worker1: the reference was replaced during the call");
      StageIn in;
      const int i_rlen = in.add(reads->read_len, 4 * (size_t)n), i_roff = in.add(reads->read_off, 8 * (size_t)n);
      const int i_pool = in.add(reads->read_pool, reads->read_pool_bytes);
      HIP_TRY(in.pack(c->h_stage_in, c->d_sw_in));
      ChainBatchDev B;
      B.n_reads = n;
      B.chain_cnt = T.chain_cnt; B.chain_base = T.chain_base; B.reg_base = T.reg_base;
      B.seed_cnt = T.seed_cnt; B.seed_base = T.seed_base;
      B.seed_rbeg = T.seed_rbeg; B.seed_qbeg = T.seed_qbeg; B.seed_len = T.seed_len;
      B.pac = d_pac; B.l_pac = ref_len;
      rc = chain2aln_back(c, opt, zdrop_mode, flags, B, in, i_rlen, i_roff, i_pool, T.nseeds, T.max_seeds, nullptr, out_cnt, out_regs, out_cap,
                          out_total);
      t_w1_ms[0] = t1 - t0; t_w1_ms[1] = t2 - t1; t_w1_ms[2] = wall_ms() - t2;
      return rc;
    }
    ChainDevResult R;
    rc = chain_dev_run(c, *sopt, opt->w, l_pac, J, &R);
    if (rc != BPSW_OK) return rc;
    chain_cnt.swap(R.chain_cnt);
    seed_cnt.swap(R.chain_seed_cnt);
    rbeg.reserve(R.seeds.size()); qbeg.reserve(R.seeds.size()); len.reserve(R.seeds.size());
    for (const bpsw_seed_t& s : R.seeds) { rbeg.push_back(s.rbeg); qbeg.push_back(s.qbeg); len.push_back(s.len); }
  } else {
    rc = seed_run(c, *sopt, *reads, &ic, &iv, &sc, &sv, nullptr, plan_on_device, false);
    if (rc != BPSW_OK) return rc;
    t1 = wall_ms();
    // chaining + filter per read (bpsw_chain.cpp), into the shape bpsw_chain2aln_batch takes
    size_t at = 0;
    for (int r = 0; r < n; ++r) {
      const int m = sc[(size_t)r];
      cc.resize((size_t)m + 1);
      cs.resize((size_t)m + 1);
      const int nc = bpsw_chain_seeds(sopt, opt->w, l_pac, m, sv.data() + at, 1, cc.data(), m, cs.data());
      if (nc < 0) return nc;
      at += (size_t)m;
      chain_cnt[(size_t)r] = nc;
      size_t k = 0;
      for (int ch = 0; ch < nc; ++ch) {
        seed_cnt.push_back(cc[(size_t)ch]);
        for (int i = 0; i < cc[(size_t)ch]; ++i, ++k) { rbeg.push_back(cs[k].rbeg); qbeg.push_back(cs[k].qbeg); len.push_back(cs[k].len); }
      }
    }
  }
  const double t2 = wall_ms();
  bpsw_chains_t B;
  B.n_reads = n;
  B.read_len = reads->read_len; B.read_off = reads->read_off; B.read_pool = reads->read_pool; B.read_pool_bytes = reads->read_pool_bytes;
  B.chain_cnt = chain_cnt.data(); B.seed_cnt = seed_cnt.data();
  B.seed_rbeg = rbeg.data(); B.seed_qbeg = qbeg.data(); B.seed_len = len.data();
  rc = bpsw_chain2aln_batch(c, opt, &B, zdrop_mode, flags, out_cnt, out_regs, out_cap, out_total);
  t_w1_ms[0] = t1 - t0; t_w1_ms[1] = t2 - t1; t_w1_ms[2] = wall_ms() - t2;
  return rc;
}

void bpsw_seed_set_resident_lanes(int lanes) { g_seed_lanes.store(lanes > 0 ? lanes : 0, std::memory_order_relaxed); }

void bpsw_last_seed_bytes(int64_t b[2]) {
  if (b) memcpy(b, t_seed_bytes, sizeof t_seed_bytes);
}

void bpsw_last_worker1_times(double ms[3]) {
  if (ms) memcpy(ms, t_w1_ms, sizeof t_w1_ms);
}

}  // extern "C"
