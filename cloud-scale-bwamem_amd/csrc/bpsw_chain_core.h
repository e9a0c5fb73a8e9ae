// bpsw_chain_core.h -- chaining and chain filtering of one read's seeds over flat, caller-provided arrays: the algorithm of
// bpsw_chain.cpp (mem_insert_seed's tree side + mem_chain's traversal, native/bwamem.c:185-304; mem_chain_weight :244-262;
// mem_chain_flt :310-379) once more, for both compilers: __host__ __device__ under hipcc (chain_kernel, bpsw_chain_dev.hip), plain
// inline under g++ (tests/chain_host).  No std::vector, no allocation, no recursion, and no array of its own that is indexed by a
// variable: every list, the B-tree's nodes and the two stacks live in the caller's workspace, so that a lane of the kernel keeps
// nothing in scratch.  bpsw_chain.cpp stays the yardstick and does not include this file.
//
// Workspace of a read of m seeds (work_bytes): the chains as index lists over the read's seed array -- chain_pos / chain_first /
// chain_last / chain_n per chain, next per seed (a seed is only ever appended at a chain's tail) --; the kbtree's node pool (t = 8,
// 15 keys a node, keys compared by pos alone, equal keys admitted: bpsw_chain.cpp's ChainTree) of node_bound(m) = m / 7 + 2 nodes
// (every node but the root holds at least 7 keys, so m keys never take more than m / 7 + 1; a smaller pool is refused); the
// traversal's and the filter's lists (order, sorted, aux); a traversal stack of 16 (node, step) pairs (a tree of 2^30 keys has
// height 12 at most); the introsort's 64 frames (the larger side is pushed: depth <= log2 n).  52 m + 256 (m / 7 + 2) + 896 bytes,
// 88.6 bytes a seed.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "bpsw.h"

#if defined(__HIPCC__)
#define BPSW_CHAIN_HD __host__ __device__ __forceinline__
#else
#define BPSW_CHAIN_HD inline
#endif

namespace bpsw {
namespace chaincore {

constexpr int T = 8, MAXK = 2 * T - 1;
constexpr int TRAV_STACK = 16, SORT_STACK = 64;
constexpr int ERR_SEED = -1;  // a seed with len < 1 or qbeg < 0 (bpsw_chain_seeds: BPSW_ERR_ARG)
constexpr int ERR_POOL = -2;  // the node pool or one of the two stacks was outgrown: nothing is truncated, the read has no result

struct Node {  // 256 bytes
  int32_t n, internal;
  int64_t pos[MAXK];
  int32_t id[MAXK];
  int32_t child[MAXK + 1];
};
struct FltAux {  // flt_aux_t: p / p2 are positions in the list sorted by weight
  int32_t beg, end, w, p, p2;
};
struct Frame {  // ks_isort_stack_t over indices
  int32_t lo, hi, depth;
};

struct Work {
  int64_t* chain_pos;
  Node* nodes;
  int32_t *chain_first, *chain_last, *chain_n, *next, *order, *sorted;
  FltAux* aux;
  int32_t* trav;  // TRAV_STACK pairs
  Frame* frames;  // SORT_STACK
  int32_t node_cap;
};

BPSW_CHAIN_HD int node_bound(int m) { return m / 7 + 2; }
BPSW_CHAIN_HD size_t work_bytes(int m, int node_cap) {
  const size_t b = 8 * (size_t)m + sizeof(Node) * (size_t)node_cap + 24 * (size_t)m + sizeof(FltAux) * (size_t)m + 8 * TRAV_STACK + sizeof(Frame) * SORT_STACK;
  return (b + 15) & ~(size_t)15;
}
BPSW_CHAIN_HD Work work_carve(uint8_t* base, int m, int node_cap) {  // base: 16-byte aligned, work_bytes(m, node_cap) long
  Work W;
  W.chain_pos = (int64_t*)base; base += 8 * (size_t)m;
  W.nodes = (Node*)base; base += sizeof(Node) * (size_t)node_cap;
  W.chain_first = (int32_t*)base; base += 4 * (size_t)m;
  W.chain_last = (int32_t*)base; base += 4 * (size_t)m;
  W.chain_n = (int32_t*)base; base += 4 * (size_t)m;
  W.next = (int32_t*)base; base += 4 * (size_t)m;
  W.order = (int32_t*)base; base += 4 * (size_t)m;
  W.sorted = (int32_t*)base; base += 4 * (size_t)m;
  W.aux = (FltAux*)base; base += sizeof(FltAux) * (size_t)m;
  W.trav = (int32_t*)base; base += 8 * TRAV_STACK;
  W.frames = (Frame*)base;
  W.node_cap = node_cap;
  return W;
}
// where chain_read leaves the chains it returns: ids of chains, in bpsw_chain_seeds' order
BPSW_CHAIN_HD const int32_t* result_list(const Work& W, int filter, int n_tree_chains) { return filter && n_tree_chains > 1 ? W.sorted : W.order; }

// ---- the kbtree (kbtree.h, KBTREE_INIT(chn, mem_chain_t, chain_cmp), t = 8) ------------------------------------------------
struct Tree {
  Node* nodes;
  int cap, n_nodes, root, n_keys;
  bool err;
};
BPSW_CHAIN_HD int tree_alloc(Tree& t) {
  if (t.n_nodes == t.cap) { t.err = true; return -1; }
  Node& z = t.nodes[t.n_nodes];
  z.n = 0; z.internal = 0;
  return t.n_nodes++;
}
// __kb_getp_aux: the first key not below pos, stepped back by one when pos is below it; *r = sign of (pos - that key)
BPSW_CHAIN_HD int tree_find(const Node& x, int64_t pos, int* r) {
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
BPSW_CHAIN_HD int tree_lower(const Tree& t, int64_t pos) {
  int lo = -1, x = t.root;
  for (;;) {
    const Node& nd = t.nodes[x];
    int r = 0;
    const int i = tree_find(nd, pos, &r);
    if (i >= 0 && r == 0) return nd.id[i];
    if (i >= 0) lo = nd.id[i];
    if (!nd.internal) return lo;
    x = nd.child[i + 1];
  }
}
BPSW_CHAIN_HD void tree_split(Tree& t, int xi, int i, int yi) {  // __kb_split: y = child i of x is full
  const int zi = tree_alloc(t);
  if (zi < 0) return;
  Node &x = t.nodes[xi], &y = t.nodes[yi], &z = t.nodes[zi];
  z.internal = y.internal;
  z.n = T - 1;
  for (int k = 0; k < T - 1; ++k) { z.pos[k] = y.pos[T + k]; z.id[k] = y.id[T + k]; }
  if (y.internal)
    for (int k = 0; k < T; ++k) z.child[k] = y.child[T + k];
  y.n = T - 1;
  for (int k = x.n; k >= i + 1; --k) x.child[k + 1] = x.child[k];
  x.child[i + 1] = zi;
  for (int k = x.n - 1; k >= i; --k) { x.pos[k + 1] = x.pos[k]; x.id[k + 1] = x.id[k]; }
  x.pos[i] = y.pos[T - 1];
  x.id[i] = y.id[T - 1];
  ++x.n;
}
BPSW_CHAIN_HD void tree_put_nonfull(Tree& t, int xi, int64_t pos, int32_t id) {  // __kb_putp_aux
  for (;;) {
    int r = 0;
    Node& x = t.nodes[xi];
    if (!x.internal) {
      const int i = tree_find(x, pos, &r);
      for (int k = x.n - 1; k >= i + 1; --k) { x.pos[k + 1] = x.pos[k]; x.id[k + 1] = x.id[k]; }
      x.pos[i + 1] = pos;
      x.id[i + 1] = id;
      ++x.n;
      return;
    }
    int i = tree_find(x, pos, &r) + 1;
    const int ci = x.child[i];
    if (t.nodes[ci].n == MAXK) {
      tree_split(t, xi, i, ci);
      if (t.err) return;
      if (pos > x.pos[i]) ++i;
    }
    xi = x.child[i];
  }
}
BPSW_CHAIN_HD void tree_put(Tree& t, int64_t pos, int32_t id) {  // kb_putp
  ++t.n_keys;
  if (t.nodes[t.root].n == MAXK) {
    const int s = tree_alloc(t);
    if (s < 0) return;
    t.nodes[s].internal = 1;
    t.nodes[s].child[0] = t.root;
    tree_split(t, s, 0, t.root);
    if (t.err) return;
    t.root = s;
  }
  tree_put_nonfull(t, t.root, pos, id);
}
// __kb_traverse without the recursion: an entry of the stack is (node, step); step s of an internal node writes key s - 1 and then
// descends into child s, a leaf writes all its keys at once.  Returns the number of ids written, -1 when the stack is outgrown.
BPSW_CHAIN_HD int tree_in_order(const Tree& t, int32_t* stack, int32_t* out) {
  int sp = 0, n_out = 0;
  stack[0] = t.root; stack[1] = 0;
  sp = 1;
  while (sp > 0) {
    const int xi = stack[2 * (sp - 1)], step = stack[2 * (sp - 1) + 1];
    const Node& x = t.nodes[xi];
    if (!x.internal) {
      for (int i = 0; i < x.n; ++i) out[n_out++] = x.id[i];
      --sp;
      continue;
    }
    if (step > x.n) { --sp; continue; }
    if (step > 0) out[n_out++] = x.id[step - 1];
    stack[2 * (sp - 1) + 1] = step + 1;
    if (sp == TRAV_STACK) return -1;
    stack[2 * sp] = x.child[step]; stack[2 * sp + 1] = 0;
    ++sp;
  }
  return n_out;
}

// ---- ks_introsort(mem_flt, ...) with flt_lt: the comparisons and swaps of bpsw_klib_sort.h, over indices -----------------------
BPSW_CHAIN_HD bool flt_lt(const FltAux& a, const FltAux& b) { return a.w > b.w; }
// (records move field by field: a struct copy through a temporary would be a private-memory object on the device)
BPSW_CHAIN_HD FltAux flt_load(const FltAux* p) {
  FltAux v;
  v.beg = p->beg; v.end = p->end; v.w = p->w; v.p = p->p; v.p2 = p->p2;
  return v;
}
BPSW_CHAIN_HD void flt_store(FltAux* p, const FltAux& v) {
  p->beg = v.beg; p->end = v.end; p->w = v.w; p->p = v.p; p->p2 = v.p2;
}
BPSW_CHAIN_HD void flt_swap(FltAux* a, int i, int j) {
  const FltAux x = flt_load(a + i), y = flt_load(a + j);
  flt_store(a + i, y);
  flt_store(a + j, x);
}
BPSW_CHAIN_HD void flt_insertion_sort(FltAux* a, int first, int last) {
  for (int i = first + 1; i < last; ++i)
    for (int j = i; j > first && flt_lt(a[j], a[j - 1]); --j) flt_swap(a, j, j - 1);
}
BPSW_CHAIN_HD void flt_comb_sort(FltAux* a, int s, int n) {  // native/ksort.h:154-175 on a[s .. s + n)
  const double shrink = 1.2473309501039786540366528676643;
  int gap = n;
  bool swapped;
  do {
    if (gap > 2) {
      gap = (int)(gap / shrink);
      if (gap == 9 || gap == 10) gap = 11;
    }
    swapped = false;
    for (int i = s; i < s + n - gap; ++i)
      if (flt_lt(a[i + gap], a[i])) { flt_swap(a, i, i + gap); swapped = true; }
  } while (swapped || gap > 2);
  if (gap != 1) flt_insertion_sort(a, s, s + n);
}
BPSW_CHAIN_HD bool flt_sort(int n, FltAux* a, Frame* stack) {  // false: the frame stack was outgrown
  if (n < 1) return true;
  if (n == 2) {
    if (flt_lt(a[1], a[0])) flt_swap(a, 0, 1);
    return true;
  }
  int d = 2;
  while ((1ul << d) < (unsigned long)n) ++d;
  int top = 0;
  int s = 0, t = n - 1;
  d <<= 1;
  for (;;) {
    if (s < t) {
      if (--d == 0) { flt_comb_sort(a, s, t - s + 1); t = s; continue; }
      int i = s, j = t, k = i + ((j - i) >> 1) + 1;
      if (flt_lt(a[k], a[i])) { if (flt_lt(a[k], a[j])) k = j; }
      else k = flt_lt(a[j], a[i]) ? i : j;
      const FltAux pivot = flt_load(a + k);
      if (k != t) flt_swap(a, k, t);
      for (;;) {
        do ++i; while (flt_lt(a[i], pivot));
        do --j; while (i <= j && flt_lt(pivot, a[j]));
        if (j <= i) break;
        flt_swap(a, i, j);
      }
      flt_swap(a, i, t);
      if (i - s > t - i) {
        if (i - s > 16) {
          if (top == SORT_STACK) return false;
          stack[top].lo = s; stack[top].hi = i - 1; stack[top].depth = d; ++top;
        }
        s = t - i > 16 ? i + 1 : t;
      } else {
        if (t - i > 16) {
          if (top == SORT_STACK) return false;
          stack[top].lo = i + 1; stack[top].hi = t; stack[top].depth = d; ++top;
        }
        t = i - s > 16 ? i - 1 : s;
      }
    } else {
      if (top == 0) { flt_insertion_sort(a, 0, n); return true; }
      --top;
      s = stack[top].lo; t = stack[top].hi; d = stack[top].depth;
    }
  }
}

// ---- chains ---------------------------------------------------------------------------------------------------------------
// test_and_merge, native/bwamem.c:185-205, on chain c of the index lists
BPSW_CHAIN_HD bool test_and_merge(const bpsw_seed_opt_t& o, int w, int64_t l_pac, const Work& W, const bpsw_seed_t* seeds, int c, int k) {
  const bpsw_seed_t p = seeds[k], last = seeds[W.chain_last[c]], first = seeds[W.chain_first[c]];
  const int64_t qend = last.qbeg + last.len, rend = last.rbeg + last.len;
  if (p.qbeg >= first.qbeg && p.qbeg + p.len <= qend && p.rbeg >= first.rbeg && p.rbeg + p.len <= rend) return true;  // contained
  if ((last.rbeg < l_pac || first.rbeg < l_pac) && p.rbeg >= l_pac) return false;                                       // other strand
  const int64_t x = p.qbeg - last.qbeg, y = p.rbeg - last.rbeg;
  if (y >= 0 && x - y <= w && y - x <= w && x - last.len < o.max_chain_gap && y - last.len < o.max_chain_gap) {
    W.next[W.chain_last[c]] = k;
    W.next[k] = -1;
    W.chain_last[c] = k;
    ++W.chain_n[c];
    return true;
  }
  return false;
}
// mem_chain_weight, native/bwamem.c:244-262, as written: the reference-side loop advances `end` by the QUERY coordinates
BPSW_CHAIN_HD int chain_weight(const Work& W, const bpsw_seed_t* seeds, int c) {
  int64_t end = 0;
  int w = 0;
  for (int k = W.chain_first[c]; k >= 0; k = W.next[k]) {
    const bpsw_seed_t s = seeds[k];
    if (s.qbeg >= end) w += s.len;
    else if (s.qbeg + s.len > end) w += (int)(s.qbeg + s.len - end);
    end = end > s.qbeg + s.len ? end : s.qbeg + s.len;
  }
  const int tmp = w;
  end = 0;
  for (int k = W.chain_first[c]; k >= 0; k = W.next[k]) {
    const bpsw_seed_t s = seeds[k];
    if (s.rbeg >= end) w += s.len;
    else if (s.rbeg + s.len > end) w += (int)(s.rbeg + s.len - end);
    end = end > s.qbeg + s.len ? end : s.qbeg + s.len;
  }
  return w < tmp ? w : tmp;
}
// mem_chain_flt, native/bwamem.c:318-379: W.order holds n_chn chains in tree order; the kept ones (heaviest first) end up in
// W.sorted.  Returns their number, ERR_POOL when the sort's stack is outgrown.
BPSW_CHAIN_HD int chain_filter(const bpsw_seed_opt_t& o, const Work& W, const bpsw_seed_t* seeds, int n_chn) {
  FltAux* a = W.aux;
  for (int i = 0; i < n_chn; ++i) {
    const int c = W.order[i];
    const bpsw_seed_t f = seeds[W.chain_first[c]], l = seeds[W.chain_last[c]];
    FltAux e;
    e.beg = f.qbeg; e.end = l.qbeg + l.len; e.w = chain_weight(W, seeds, c); e.p = i; e.p2 = -1;
    flt_store(a + i, e);
  }
  if (!flt_sort(n_chn, a, W.frames)) return ERR_POOL;
  for (int i = 0; i < n_chn; ++i) {
    W.sorted[i] = W.order[a[i].p];
    a[i].p = i;
  }
  int n = 1;
  for (int i = 1; i < n_chn; ++i) {
    const FltAux ai = flt_load(a + i);
    int j = 0;
    for (; j < n; ++j) {
      const FltAux aj = flt_load(a + j);
      const int b_max = aj.beg > ai.beg ? aj.beg : ai.beg;
      const int e_min = aj.end < ai.end ? aj.end : ai.end;
      if (e_min > b_max) {  // overlap
        const int li = ai.end - ai.beg, lj = aj.end - aj.beg;
        const int min_l = li < lj ? li : lj;
        if ((float)(e_min - b_max) >= (float)min_l * o.mask_level) {  // significant overlap (int * float, compared as float, as in the C)
          if (aj.p2 < 0) a[j].p2 = ai.p;
          if ((float)ai.w < (float)aj.w * o.chain_drop_ratio && aj.w - ai.w >= o.min_seed_len << 1) break;
        }
      }
    }
    if (j == n) flt_store(a + n++, ai);
  }
  int32_t* keep = W.order;  // the tree order is used up
  for (int i = 0; i < n_chn; ++i) keep[i] = 0;
  for (int i = 0; i < n; ++i) {
    keep[a[i].p] = 1;
    if (a[i].p2 >= 0) keep[a[i].p2] = 1;  // the chain that shadows it most is kept too
  }
  int n_kept = 0;
  for (int i = 0; i < n_chn; ++i)
    if (keep[i]) W.sorted[n_kept++] = W.sorted[i];
  return n_kept;
}

// One read: its m seeds in emission order -> chains.  Returns the number of chains (their ids in result_list(W, filter,
// *n_tree_chains)) and in *n_out_seeds the seeds they hold, or ERR_SEED / ERR_POOL.  drop_bridging: a seed with
// rbeg < l_pac < rbeg + len is passed over (native/bwamem.c:228), as bpsw_seed_batch does before it hands the seeds out.
BPSW_CHAIN_HD int chain_read(const bpsw_seed_opt_t& o, int w, int64_t l_pac, int m, const bpsw_seed_t* seeds, int filter, int drop_bridging,
                             const Work& W, int* n_tree_chains, int* n_out_seeds) {
  *n_tree_chains = *n_out_seeds = 0;
  if (m == 0) return 0;
  if (W.node_cap < node_bound(m)) return ERR_POOL;  // refused before anything is written; tree_alloc still guards every node taken
  Tree tree;
  tree.nodes = W.nodes; tree.cap = W.node_cap; tree.n_nodes = 0; tree.root = 0; tree.n_keys = 0; tree.err = false;
  if (tree_alloc(tree) < 0) return ERR_POOL;
  int n_chains = 0;
  for (int k = 0; k < m; ++k) {
    const bpsw_seed_t s = seeds[k];
    if (s.len < 1 || s.qbeg < 0) return ERR_SEED;
    if (drop_bridging && s.rbeg < l_pac && l_pac < s.rbeg + s.len) continue;
    bool add = true;
    if (tree.n_keys) {
      const int lo = tree_lower(tree, s.rbeg);
      if (lo >= 0 && test_and_merge(o, w, l_pac, W, seeds, lo, k)) add = false;
    }
    if (add) {
      const int c = n_chains++;
      W.chain_pos[c] = s.rbeg;
      W.chain_first[c] = W.chain_last[c] = k;
      W.chain_n[c] = 1;
      W.next[k] = -1;
      tree_put(tree, s.rbeg, c);
      if (tree.err) return ERR_POOL;
    }
  }
  if (n_chains == 0) return 0;
  int nc = tree_in_order(tree, W.trav, W.order);
  if (nc < 0) return ERR_POOL;
  *n_tree_chains = nc;
  if (filter && nc > 1) {
    nc = chain_filter(o, W, seeds, nc);
    if (nc < 0) return nc;
  }
  const int32_t* list = result_list(W, filter, *n_tree_chains);
  int total = 0;
  for (int c = 0; c < nc; ++c) total += W.chain_n[list[c]];
  *n_out_seeds = total;
  return nc;
}
// the chains of `list` in the shape of bpsw_chain_seeds' output
BPSW_CHAIN_HD void chain_emit(const Work& W, const int32_t* list, int nc, const bpsw_seed_t* seeds, int32_t* chain_seed_cnt, bpsw_seed_t* out_seeds) {
  size_t at = 0;
  for (int c = 0; c < nc; ++c) {
    const int ch = list[c];
    chain_seed_cnt[c] = W.chain_n[ch];
    for (int k = W.chain_first[ch]; k >= 0; k = W.next[k]) out_seeds[at++] = seeds[k];
  }
}

}  // namespace chaincore
}  // namespace bpsw
