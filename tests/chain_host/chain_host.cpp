// chain_host.cpp -- the chain kernel's algorithm (csrc/bpsw_chain_core.h) compiled for the HOST over malloc'd workspaces of exactly
// the size the header asks for, so that tests/test_chain_core_host.py can hold it against bpsw_chain_seeds and the reference's
// recorded chains without a GPU.  Test infrastructure: chain_core_seeds does for one read what a lane of chain_kernel and of
// chain_emit_kernel do (bpsw_chain_dev.hip).  With -DCHAIN_HOST_MAIN it is a program of its own: the core over generated seed lists,
// for a build under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "bpsw_chain_core.h"

namespace cc = bpsw::chaincore;

// node_cap < 0: the bound the header names.  Returns the number of chains, -1 for a bad seed, -3 when chain_cap is too small,
// -100 when a pool was outgrown.
extern "C" int chain_core_seeds_ex(const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_seeds, const bpsw_seed_t* seeds,
                                   int32_t filter, int32_t drop_bridging, int32_t node_cap, int32_t* chain_seed_cnt, int32_t chain_cap,
                                   bpsw_seed_t* out_seeds) {
  if (n_seeds == 0) return 0;
  if (node_cap < 0) node_cap = cc::node_bound(n_seeds);
  uint8_t* mem = (uint8_t*)malloc(cc::work_bytes(n_seeds, node_cap));
  if (!mem) return -2;
  const cc::Work W = cc::work_carve(mem, n_seeds, node_cap);
  int n_tree = 0, n_out = 0;
  int nc = cc::chain_read(*sopt, w, l_pac, n_seeds, seeds, filter, drop_bridging, W, &n_tree, &n_out);
  if (nc == cc::ERR_POOL) nc = -100;
  else if (nc > chain_cap) nc = -3;
  else if (nc > 0) cc::chain_emit(W, cc::result_list(W, filter, n_tree), nc, seeds, chain_seed_cnt, out_seeds);
  free(mem);
  return nc;
}

extern "C" int chain_core_seeds(const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_seeds, const bpsw_seed_t* seeds,
                                int32_t filter, int32_t* chain_seed_cnt, int32_t chain_cap, bpsw_seed_t* out_seeds) {
  return chain_core_seeds_ex(sopt, w, l_pac, n_seeds, seeds, filter, 0, -1, chain_seed_cnt, chain_cap, out_seeds);
}

#ifdef CHAIN_HOST_MAIN
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545f4914f6cdd1dull) >> 33) % n;
}

int main() {
  const int64_t l_pac = 1 << 20;
  long chains = 0, kept = 0;
  for (int it = 0; it < 4000; ++it) {
    bpsw_seed_opt_t o;
    o.min_seed_len = 19; o.max_occ = 10000; o.split_width = 10; o.no_exact = 0; o.split_factor = 1.5f;
    o.max_chain_gap = it % 3 ? 10000 : 30;
    o.chain_drop_ratio = it % 5 ? 0.5f : 0.9f;
    o.mask_level = it % 7 ? 0.5f : 0.2f;
    const int shape = it % 4;
    const int m = it % 50 == 0 ? 2000 + (int)rnd(500) : (int)rnd(shape == 0 ? 20 : 400);
    bpsw_seed_t* seeds = (bpsw_seed_t*)malloc(sizeof(bpsw_seed_t) * (size_t)(m ? m : 1));
    for (int k = 0; k < m; ++k) {
      bpsw_seed_t s;
      s.len = 19 + (int)rnd(shape == 2 ? 1 : 40);  // shape 2: every chain of one seed weighs the same
      s.qbeg = (int)rnd(200);
      if (shape == 1) s.rbeg = (int64_t)rnd(3000) + (rnd(2) ? l_pac : 0) + s.qbeg;  // crowded: merges, equal pos
      else if (shape == 3) s.rbeg = l_pac - 40 + (int64_t)rnd(80);                   // around l_pac, bridging ones among them
      else s.rbeg = (int64_t)rnd(2u << 20);
      seeds[k] = s;
    }
    int32_t* cnt = (int32_t*)malloc(4 * (size_t)(m ? m : 1));
    bpsw_seed_t* out = (bpsw_seed_t*)malloc(sizeof(bpsw_seed_t) * (size_t)(m ? m : 1));
    const int a = chain_core_seeds_ex(&o, it % 2 ? 100 : 5, l_pac, m, seeds, 0, shape == 3, -1, cnt, m, out);
    const int b = chain_core_seeds_ex(&o, it % 2 ? 100 : 5, l_pac, m, seeds, 1, shape == 3, -1, cnt, m, out);
    if (a < 0 || b < 0 || b > a) { fprintf(stderr, "list %d: %d chains, %d kept\n", it, a, b); return 1; }
    chains += a; kept += b;
    free(seeds); free(cnt); free(out);
  }
  printf("chain core: %ld chains, %ld kept\n", chains, kept);
  return chains > kept && kept > 0 ? 0 : 1;
}
#endif
