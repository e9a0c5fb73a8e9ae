// bpsw_chain.cpp -- host side of worker1's seeding: chaining and chain filtering of one read's seeds.
//
// Replaces the tree side of mem_insert_seed + mem_chain (native/bwamem.c:185-304) and mem_chain_flt (:310-379), i.e.
// generateChains / memChainFilter of the Scala driver (worker1/MemChain.scala, MemChainFilter.scala).  Host only: no context, no
// device, like bpsw_mark_primary_se.
//
// Two orders of the reference are properties of klib and not of the data, and both are restated here:
//   * the chains of a read live in a kbtree keyed by pos ALONE (chain_cmp); the tree admits equal keys, and where an equal key
//     lands -- hence which of two equal-pos chains kb_intervalp finds and which comes first in the traversal -- follows from
//     kbtree.h's node search and split (ChainTree below);
//   * mem_chain_flt orders the chains by weight with ks_introsort, which is not stable (bpsw_klib_sort.h).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bpsw_internal.h"
#include "bpsw_klib_sort.h"

using namespace bpsw;

namespace {

struct Chain {
  int64_t pos;
  std::vector<bpsw_seed_t> seeds;
};

// kbtree.h, KBTREE_INIT(chn, mem_chain_t, chain_cmp) with KB_DEFAULT_SIZE = 512: sizeof(mem_chain_t) == 24 gives
// t = ((512 - 4 - 8) / (8 + 24) + 1) >> 1 = 8, so a node holds at most 15 keys.  A key here is (pos, index of the chain): the
// reference keeps the chain itself in the node and grows it in place, which an index into `chains` does as well.
struct ChainTree {
  static constexpr int T = 8, MAXK = 2 * T - 1;
  struct Node {
    bool internal = false;
    int n = 0;
    int64_t pos[MAXK];
    int32_t id[MAXK];
    int32_t child[MAXK + 1];
  };
  std::vector<Node> nodes;
  int root = 0;
  int n_keys = 0;
  ChainTree() { nodes.emplace_back(); }

  // __kb_getp_aux: the first key not below pos, stepped back by one when pos is below it; *r = sign of (pos - that key)
  static int find(const Node& x, int64_t pos, int* r) {
    int begin = 0, end = x.n;
    if (x.n == 0) return -1;
    while (begin < end) {
      const int mid = (begin + end) >> 1;
      if (x.pos[mid] < pos) begin = mid + 1;
      else end = mid;
    }
    if (begin == x.n) { *r = 1; return x.n - 1; }
    *r = (x.pos[begin] < pos) - (pos < x.pos[begin]);
    if (*r < 0) --begin;
    return begin;
  }
  // kb_intervalp's `lower`: the chain with the largest pos <= `pos` as the tree finds it, -1 if none
  int lower(int64_t pos) const {
    int lo = -1, x = root;
    for (;;) {
      const Node& nd = nodes[(size_t)x];
      int r = 0;
      const int i = find(nd, pos, &r);
      if (i >= 0 && r == 0) return nd.id[i];
      if (i >= 0) lo = nd.id[i];
      if (!nd.internal) return lo;
      x = nd.child[i + 1];
    }
  }
  void split(int xi, int i, int yi) {  // __kb_split: y = child i of x is full
    const int zi = (int)nodes.size();
    nodes.emplace_back();
    Node &x = nodes[(size_t)xi], &y = nodes[(size_t)yi], &z = nodes[(size_t)zi];
    z.internal = y.internal;
    z.n = T - 1;
    memcpy(z.pos, y.pos + T, sizeof(int64_t) * (T - 1));
    memcpy(z.id, y.id + T, sizeof(int32_t) * (T - 1));
    if (y.internal) memcpy(z.child, y.child + T, sizeof(int32_t) * T);
    y.n = T - 1;
    memmove(x.child + i + 2, x.child + i + 1, sizeof(int32_t) * (size_t)(x.n - i));
    x.child[i + 1] = zi;
    memmove(x.pos + i + 1, x.pos + i, sizeof(int64_t) * (size_t)(x.n - i));
    memmove(x.id + i + 1, x.id + i, sizeof(int32_t) * (size_t)(x.n - i));
    x.pos[i] = y.pos[T - 1];
    x.id[i] = y.id[T - 1];
    ++x.n;
  }
  void put_nonfull(int xi, int64_t pos, int32_t id) {  // __kb_putp_aux
    for (;;) {
      int r = 0;
      if (!nodes[(size_t)xi].internal) {
        Node& x = nodes[(size_t)xi];
        const int i = find(x, pos, &r);
        if (i != x.n - 1) {
          memmove(x.pos + i + 2, x.pos + i + 1, sizeof(int64_t) * (size_t)(x.n - i - 1));
          memmove(x.id + i + 2, x.id + i + 1, sizeof(int32_t) * (size_t)(x.n - i - 1));
        }
        x.pos[i + 1] = pos;
        x.id[i + 1] = id;
        ++x.n;
        return;
      }
      int i = find(nodes[(size_t)xi], pos, &r) + 1;
      const int ci = nodes[(size_t)xi].child[i];
      if (nodes[(size_t)ci].n == MAXK) {
        split(xi, i, ci);
        if (pos > nodes[(size_t)xi].pos[i]) ++i;
      }
      xi = nodes[(size_t)xi].child[i];
    }
  }
  void put(int64_t pos, int32_t id) {  // kb_putp
    ++n_keys;
    if (nodes[(size_t)root].n == MAXK) {
      const int s = (int)nodes.size();
      nodes.emplace_back();
      nodes[(size_t)s].internal = true;
      nodes[(size_t)s].child[0] = root;
      split(s, 0, root);
      root = s;
    }
    put_nonfull(root, pos, id);
  }
  void in_order(int xi, std::vector<int32_t>* out) const {  // __kb_traverse
    const Node& x = nodes[(size_t)xi];
    for (int i = 0; i < x.n; ++i) {
      if (x.internal) in_order(x.child[i], out);
      out->push_back(x.id[i]);
    }
    if (x.internal) in_order(x.child[x.n], out);
  }
};

// test_and_merge, native/bwamem.c:185-205
bool test_and_merge(const bpsw_seed_opt_t& o, int w, int64_t l_pac, Chain& c, const bpsw_seed_t& p) {
  const bpsw_seed_t& last = c.seeds.back();
  const bpsw_seed_t& first = c.seeds.front();
  const int64_t qend = last.qbeg + last.len, rend = last.rbeg + last.len;
  if (p.qbeg >= first.qbeg && p.qbeg + p.len <= qend && p.rbeg >= first.rbeg && p.rbeg + p.len <= rend) return true;  // contained
  if ((last.rbeg < l_pac || first.rbeg < l_pac) && p.rbeg >= l_pac) return false;                                       // other strand
  const int64_t x = p.qbeg - last.qbeg, y = p.rbeg - last.rbeg;
  if (y >= 0 && x - y <= w && y - x <= w && x - last.len < o.max_chain_gap && y - last.len < o.max_chain_gap) {
    c.seeds.push_back(p);
    return true;
  }
  return false;
}

// mem_chain_weight, native/bwamem.c:244-262, as written: the reference-side loop advances `end` by the QUERY coordinates
int chain_weight(const Chain& c) {
  int64_t end = 0;
  int w = 0;
  for (const bpsw_seed_t& s : c.seeds) {
    if (s.qbeg >= end) w += s.len;
    else if (s.qbeg + s.len > end) w += (int)(s.qbeg + s.len - end);
    end = end > s.qbeg + s.len ? end : s.qbeg + s.len;
  }
  const int tmp = w;
  end = 0;
  for (const bpsw_seed_t& s : c.seeds) {
    if (s.rbeg >= end) w += s.len;
    else if (s.rbeg + s.len > end) w += (int)(s.rbeg + s.len - end);
    end = end > s.qbeg + s.len ? end : s.qbeg + s.len;
  }
  return w < tmp ? w : tmp;
}

struct FltAux {  // flt_aux_t: p / p2 are positions in the list sorted by weight
  int beg, end, w, p, p2;
};
struct FltLt {  // flt_lt
  bool operator()(const FltAux& a, const FltAux& b) const { return a.w > b.w; }
};

// mem_chain_flt, native/bwamem.c:318-379: `order` holds the chains in tree order going in, the kept ones (heaviest first) coming out
void chain_filter(const bpsw_seed_opt_t& o, const std::vector<Chain>& chains, std::vector<int32_t>* order) {
  const int n_chn = (int)order->size();
  if (n_chn <= 1) return;
  std::vector<FltAux> a((size_t)n_chn);
  for (int i = 0; i < n_chn; ++i) {
    const Chain& c = chains[(size_t)(*order)[(size_t)i]];
    a[(size_t)i] = {c.seeds.front().qbeg, c.seeds.back().qbeg + c.seeds.back().len, chain_weight(c), i, -1};
  }
  klib_order_sort((size_t)n_chn, a.data(), FltLt());
  std::vector<int32_t> sorted((size_t)n_chn);
  for (int i = 0; i < n_chn; ++i) {
    sorted[(size_t)i] = (*order)[(size_t)a[(size_t)i].p];
    a[(size_t)i].p = i;
  }
  int n = 1;
  for (int i = 1; i < n_chn; ++i) {
    int j = 0;
    for (; j < n; ++j) {
      const int b_max = a[(size_t)j].beg > a[(size_t)i].beg ? a[(size_t)j].beg : a[(size_t)i].beg;
      const int e_min = a[(size_t)j].end < a[(size_t)i].end ? a[(size_t)j].end : a[(size_t)i].end;
      if (e_min > b_max) {  // overlap
        const int li = a[(size_t)i].end - a[(size_t)i].beg, lj = a[(size_t)j].end - a[(size_t)j].beg;
        const int min_l = li < lj ? li : lj;
        if (e_min - b_max >= min_l * o.mask_level) {  // significant overlap (int * float, compared as float, as in the C)
          if (a[(size_t)j].p2 < 0) a[(size_t)j].p2 = a[(size_t)i].p;
          if (a[(size_t)i].w < a[(size_t)j].w * o.chain_drop_ratio && a[(size_t)j].w - a[(size_t)i].w >= o.min_seed_len << 1) break;
        }
      }
    }
    if (j == n) a[(size_t)n++] = a[(size_t)i];
  }
  std::vector<char> keep((size_t)n_chn, 0);
  for (int i = 0; i < n; ++i) {
    keep[(size_t)a[(size_t)i].p] = 1;
    if (a[(size_t)i].p2 >= 0) keep[(size_t)a[(size_t)i].p2] = 1;  // the chain that shadows it most is kept too
  }
  order->clear();
  for (int i = 0; i < n_chn; ++i)
    if (keep[(size_t)i]) order->push_back(sorted[(size_t)i]);
}

}  // namespace

extern "C" {

void bpsw_seed_opt_default(bpsw_seed_opt_t* s) {  // mem_opt_init, native/bwamem.c:45-74
  if (!s) return;
  s->min_seed_len = 19;
  s->max_occ = 10000;
  s->split_width = 10;
  s->max_chain_gap = 10000;
  s->no_exact = 0;
  s->split_factor = 1.5f;
  s->chain_drop_ratio = 0.50f;
  s->mask_level = 0.50f;
}

int bpsw_chain_seeds(const bpsw_seed_opt_t* sopt, int32_t w, int64_t l_pac, int32_t n_seeds, const bpsw_seed_t* seeds, int32_t filter,
                     int32_t* chain_seed_cnt, int32_t chain_cap, bpsw_seed_t* out_seeds) {
  if (!sopt || n_seeds < 0 || (n_seeds > 0 && (!seeds || !chain_seed_cnt || !out_seeds))) return fail(BPSW_ERR_ARG, "chain_seeds: null argument");
  if (n_seeds == 0) return 0;
  std::vector<Chain> chains;
  ChainTree tree;
  for (int32_t k = 0; k < n_seeds; ++k) {
    const bpsw_seed_t& s = seeds[k];
    if (s.len < 1 || s.qbeg < 0) return fail(BPSW_ERR_ARG, "chain_seeds: seed with a negative start or no length");
    bool add = true;
    if (tree.n_keys) {
      const int lo = tree.lower(s.rbeg);
      if (lo >= 0 && test_and_merge(*sopt, w, l_pac, chains[(size_t)lo], s)) add = false;
    }
    if (add) {
      chains.push_back(Chain{s.rbeg, {s}});
      tree.put(s.rbeg, (int32_t)chains.size() - 1);
    }
  }
  std::vector<int32_t> order;
  order.reserve(chains.size());
  tree.in_order(tree.root, &order);
  if (filter) chain_filter(*sopt, chains, &order);
  if ((int64_t)order.size() > chain_cap) return fail(BPSW_ERR_CAPACITY, "chain_seeds: chain_seed_cnt too small");
  size_t at = 0;
  for (size_t c = 0; c < order.size(); ++c) {
    const Chain& ch = chains[(size_t)order[c]];
    chain_seed_cnt[c] = (int32_t)ch.seeds.size();
    memcpy(out_seeds + at, ch.seeds.data(), sizeof(bpsw_seed_t) * ch.seeds.size());
    at += ch.seeds.size();
  }
  return (int)order.size();
}

}  // extern "C"
