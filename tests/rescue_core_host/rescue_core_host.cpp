// csrc/bpsw_rescue_core.h on the host, alone: reads mate-rescue groups (tests/test_rescue_core_host.py writes every group of
// tests/rescue_cases.py, as bytes and as coordinates) and prints, per group and flavour, what the header decides about them -- the
// first-round windows of the per-pair plan (with and without its straight-line fast path), the pairs it touches, the shim's verdict
// per pair (likewise), and the anchors of every end.  Built with
// -fsanitize=address,undefined; every array is a heap block of exactly its length.  The judging is done in Python.
//
// input, whitespace-separated integers:  n_groups, then per group
//   form (0: window lengths shipped, 1: coordinates only)  G  l_pac  flag  max_matesw  pen_unpaired   4 x (low high failed)
//   seq_len[2G]  reg_cnt[2G]  ref_cnt[2G]   n_regs  n_regs x (rb score)   n_windows  ref_rb[n_windows]  ref_re[n_windows]  (form 0: ref_len[n_windows])
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpsw_rescue_core.h"

using namespace bpsw;

static FILE* in;
static long long next_int() {
  long long v;
  if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "rescue_core_host: input ends early\n"); exit(2); }
  return v;
}
template <class T>
static T* read_array(size_t n) {  // exactly n elements on the heap (n == 0: one, never read)
  T* p = (T*)malloc(sizeof(T) * (n ? n : 1));
  for (size_t i = 0; i < n; ++i) p[i] = (T)next_int();
  return p;
}
static void print_list(const char* what, const std::vector<long long>& v) {
  printf("%s %zu", what, v.size());
  for (long long x : v) printf(" %lld", x);
  printf("\n");
}

template <bool Fast>
static void plan(const RescueRules& U, const bpsw_rescue_group_t& g, std::vector<long long>* windows, std::vector<long long>* touched,
                 std::vector<long long>* verdict) {
  int64_t nreg = 0, nref = 0;  // prefix sums of this program's own
  for (int k = 0; k < g.group_size; ++k) {
    const int e = 2 * k;
    const RescuePairCounts p = {{g.reg_cnt[e], g.reg_cnt[e + 1]}, {g.ref_cnt[e], g.ref_cnt[e + 1]}, {g.seq_len[e], g.seq_len[e + 1]}};
    const int64_t base[2] = {nreg, nreg + p.rc[0]}, rowb[2] = {nref, nref + p.fc[0]};
    nreg += p.rc[0] + p.rc[1]; nref += p.fc[0] + p.fc[1];
    if (rescue_plan_pair<Fast>(U, g, k, p, base, rowb, [&](int64_t x, int mate) {
          if (mate != (e | 1) && mate != e) { fprintf(stderr, "rescue_core_host: window %lld of pair %d for end %d\n", (long long)x, k, mate); exit(3); }
          windows->push_back(x);
        }))
      touched->push_back(k);
    // the shim's verdict: blind to windows and mate lengths
    bool may;
    if (Fast) {
      may = rescue_pair_may_need_job(U, g.regs + base[0], g.regs + base[1], p.rc, p.fc);
    } else {
      const RescuePairCounts q = {{p.rc[0], p.rc[1]}, {p.fc[0], p.fc[1]}, {1, 1}};
      may = false;
      rescue_walk_pair<false>(U, g.regs + base[0], g.regs + base[1], q, [&](int, int, int) { return may = true; });
    }
    if (may) verdict->push_back(k);
  }
}

int main(int argc, char** argv) {
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: rescue_core_host GROUPS\n"); return 2; }
  const int n_groups = (int)next_int();
  for (int gi = 0; gi < n_groups; ++gi) {
    bpsw_rescue_group_t g;
    memset(&g, 0, sizeof g);
    bpsw_opt_t opt;
    memset(&opt, 0, sizeof opt);
    const int form = (int)next_int();
    g.group_size = (int32_t)next_int();
    g.l_pac = next_int();
    opt.flag = (int32_t)next_int(); opt.max_matesw = (int32_t)next_int(); opt.pen_unpaired = (int32_t)next_int();
    for (int r = 0; r < 4; ++r) { g.pes[r].low = (int32_t)next_int(); g.pes[r].high = (int32_t)next_int(); g.pes[r].failed = (int32_t)next_int(); }
    const size_t ends = 2 * (size_t)g.group_size;
    int32_t* seq_len = read_array<int32_t>(ends);
    int32_t* reg_cnt = read_array<int32_t>(ends);
    int32_t* ref_cnt = read_array<int32_t>(ends);
    const size_t n_regs = (size_t)next_int();
    bpsw_alnreg_t* regs = (bpsw_alnreg_t*)calloc(n_regs ? n_regs : 1, sizeof(bpsw_alnreg_t));
    for (size_t i = 0; i < n_regs; ++i) { regs[i].rb = next_int(); regs[i].score = (int32_t)next_int(); }
    const size_t n_win = (size_t)next_int();
    int64_t* ref_rb = read_array<int64_t>(n_win);
    int64_t* ref_re = read_array<int64_t>(n_win);
    int64_t* ref_len = form == 0 ? read_array<int64_t>(n_win) : nullptr;
    uint8_t* pool = form == 0 ? (uint8_t*)malloc(1) : nullptr;  // (only whether there is a pool is looked at)
    g.seq_len = seq_len; g.reg_cnt = reg_cnt; g.ref_cnt = ref_cnt; g.regs = regs;
    g.ref_rb = ref_rb; g.ref_re = ref_re; g.ref_len = ref_len; g.ref_pool = pool;
    const bool rescue_on = (opt.flag & 0x20) == 0;  // MEM_F_NO_RESCUE: the callers' switch, not a rule of the header
    for (int mode = BPSW_RESCUE_C; mode <= BPSW_RESCUE_SCALA; ++mode) {
      const RescueRules U = rescue_rules(opt, g.pes, g.l_pac, mode);
      std::vector<long long> w[2], t[2], v[2];
      if (rescue_on) {
        plan<true>(U, g, &w[0], &t[0], &v[0]);
        plan<false>(U, g, &w[1], &t[1], &v[1]);
      }
      printf("group %d %d %d\n", gi, form, mode);
      print_list("windows", w[0]); print_list("windows_walk", w[1]);
      print_list("touched", t[0]); print_list("touched_walk", t[1]);
      print_list("verdict", v[0]); print_list("verdict_walk", v[1]);
      size_t at = 0;
      for (size_t e = 0; e < ends; ++e) {
        std::vector<long long> anchors;
        rescue_walk_anchors(U, regs + at, reg_cnt[e], ref_cnt[e], [&](int j, int ai) {
          if (j != (int)anchors.size()) { fprintf(stderr, "rescue_core_host: rank %d after %zu anchors\n", j, anchors.size()); exit(3); }
          anchors.push_back(ai);
          return true;
        });
        print_list("anchors", anchors);
        at += (size_t)reg_cnt[e];
      }
    }
    free(seq_len); free(reg_cnt); free(ref_cnt); free(regs); free(ref_rb); free(ref_re); free(ref_len); free(pool);
  }
  fclose(in);
  return 0;
}
