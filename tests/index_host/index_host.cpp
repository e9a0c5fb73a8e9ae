// index_host.cpp -- the host twin of bpsw_index.hip: every kernel of the FM-index construction played serially, lanes and tiles in
// loops, on the functions of bpsw_index_core.h.  A program of its own (tests/test_fmi_build_core_host.py builds it with
// -fsanitize=address,undefined); every array lives in a heap block of exactly its size, so an index one past an end is a report.
//
//   index_host run IN OUT
// IN:  per case  int64 l_pac, int32 sa_intv, int32 first-key bases (0: default), int32 sort tile (0: default), int32 0, then the
//      (l_pac + 3) / 4 pac bytes.
// OUT: per case  int64 primary, L2[5], seq_len, bwt_size, n_sa, rounds, unresolved after the first sort, radix passes, tiles of the
//      first sort; then bwt_size uint32 and n_sa int64.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "bpsw_index_core.h"

namespace xc = bpsw::idxcore;
using xc::i64;
using xc::u64;

template <class T> struct Block {  // exactly n items on the heap
  std::unique_ptr<T[]> p;
  i64 n;
  explicit Block(i64 n_) : p(new T[(size_t)n_]()), n(n_) {}
  T* get() { return p.get(); }
};

// the device scan's contract (bpsw_scan.hip): `cols` columns of n values, column k at data[k (n + 1)], exclusive, the total in entry n
static void scan_cols(i64* data, int cols, i64 n) {
  for (int c = 0; c < cols; ++c) {
    i64* col = data + (i64)c * (n + 1);
    i64 sum = 0;
    for (i64 i = 0; i < n; ++i) { const i64 v = col[i]; col[i] = sum; sum += v; }
    col[n] = sum;
  }
}

static i64 g_passes = 0;

// sort_hist_kernel, the scan, sort_scatter_kernel: one pass of the sort, workgroup by workgroup, step by step, wavefront by wavefront
static void sort_pass(const u64* K, const i64* V, i64 M, int shift, int tile, u64* Ko, i64* Vo) {
  const i64 tiles = (M + tile - 1) / tile;
  Block<i64> table(tiles * xc::kRadix + 1);
  for (i64 b = 0; b < tiles; ++b) {
    int cnt[xc::kRadix] = {0};
    const i64 lo = b * tile, hi = lo + tile < M ? lo + tile : M;
    for (i64 i = lo; i < hi; ++i) ++cnt[xc::digit_of(K[i], shift)];
    for (int t = 0; t < xc::kRadix; ++t) table.get()[(i64)t * tiles + b] = cnt[t];
  }
  scan_cols(table.get(), 1, tiles * xc::kRadix);
  for (i64 b = 0; b < tiles; ++b) {
    i64 base[xc::kRadix];
    int wcnt[xc::kSortWaves][xc::kRadix];
    for (int t = 0; t < xc::kRadix; ++t) {
      base[t] = table.get()[(i64)t * tiles + b];
      for (int w = 0; w < xc::kSortWaves; ++w) wcnt[w][t] = 0;
    }
    const i64 lo = b * tile, hi = lo + tile < M ? lo + tile : M;
    for (i64 i0 = lo; i0 < hi; i0 += xc::kSortThreads) {
      u64 before[xc::kSortThreads];
      int digit[xc::kSortThreads];
      bool valid[xc::kSortThreads];
      for (int t = 0; t < xc::kSortThreads; ++t) {
        valid[t] = i0 + t < hi;
        digit[t] = xc::digit_of(valid[t] ? K[i0 + t] : 0, shift);
      }
      for (int wave = 0; wave < xc::kSortWaves; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
          const int t = wave * 64 + lane;
          u64 same = 0;  // the ballots
          for (int l = 0; l < 64; ++l)
            if (valid[wave * 64 + l] && digit[wave * 64 + l] == digit[t]) same |= 1ull << l;
          before[t] = same & ((1ull << lane) - 1);
          if (valid[t] && before[t] == 0) wcnt[wave][digit[t]] = __builtin_popcountll(same);
        }
      for (int t = 0; t < xc::kSortThreads; ++t) {
        if (!valid[t]) continue;
        i64 pos = base[digit[t]] + __builtin_popcountll(before[t]);
        for (int w = 0; w < t / 64; ++w) pos += wcnt[w][digit[t]];
        Ko[pos] = K[i0 + t];
        Vo[pos] = V[i0 + t];
      }
      for (int t = 0; t < xc::kRadix; ++t)
        for (int w = 0; w < xc::kSortWaves; ++w) { base[t] += wcnt[w][t]; wcnt[w][t] = 0; }
    }
  }
  ++g_passes;
}

struct Result {
  i64 primary, L2[5], seq_len, bwt_size, n_sa, rounds, unresolved_first, passes, tiles;
  std::vector<uint32_t> bwt;
  std::vector<i64> sa;
};

static int build(const uint8_t* pac_in, i64 l_pac, int sa_intv, int k0, int tile, Result* R) {
  if (k0 < 1 || k0 > xc::kMaxFirstKey) k0 = xc::kMaxFirstKey;
  if (tile < 1) tile = xc::kSortTile;
  const xc::Shape S = xc::shape_of(l_pac, sa_intv);
  const i64 seq_len = S.seq_len, N = seq_len + 1;
  const int rank_bits = xc::bits_for((u64)(N - 1));
  Block<uint8_t> pac((l_pac + 3) / 4);
  memcpy(pac.get(), pac_in, (size_t)pac.n);
  const xc::Text T{pac.get(), l_pac};
  Block<i64> rank(N), sa(N);
  for (i64 i = 0; i < N; ++i) rank.get()[i] = sa.get()[i] = -1;
  g_passes = 0;
  R->rounds = 0; R->unresolved_first = 0; R->tiles = (N + tile - 1) / tile;
  std::unique_ptr<Block<i64>> list_suffix, list_group;
  i64 M = N, h = k0;
  for (int round = 0; M > 0; ++round) {
    const int bits = round == 0 ? xc::first_key_bits(k0) : 2 * rank_bits, group_shift = round == 0 ? 64 : rank_bits;
    Block<u64> K0(M), K1(M);
    Block<i64> V0(M), V1(M);
    u64* K[2] = {K0.get(), K1.get()};
    i64* V[2] = {V0.get(), V1.get()};
    for (i64 m = 0; m < M; ++m) {
      if (round == 0) { K[0][m] = xc::first_key(T, m, k0); V[0][m] = m; }
      else {
        const i64 s = list_suffix->get()[m];
        K[0][m] = xc::round_key(rank.get(), seq_len, s, list_group->get()[m], h, rank_bits);
        V[0][m] = s;
      }
    }
    int at = 0;
    for (int p = 0; p < xc::radix_passes(bits) && M > 1; ++p, at ^= 1) sort_pass(K[at], V[at], M, p * xc::kRadixBits, tile, K[at ^ 1], V[at ^ 1]);
    Block<i64> cols(3 * (M + 1));
    for (i64 m = 0; m < M; ++m) xc::flags_write(K[at], M, m, group_shift, cols.get());
    scan_cols(cols.get(), 3, M);
    const i64 runs = cols.get()[M], groups = cols.get()[(M + 1) + M], left = cols.get()[2 * (M + 1) + M];
    Block<i64> run_pos(runs), group_pos(groups);
    for (i64 m = 0; m < M; ++m) xc::heads_write(K[at], M, m, group_shift, cols.get(), run_pos.get(), group_pos.get());
    std::unique_ptr<Block<i64>> next_suffix(new Block<i64>(left)), next_group(new Block<i64>(left));
    for (i64 m = 0; m < M; ++m)
      xc::assign_at(K[at], V[at], M, m, group_shift, cols.get(), run_pos.get(), group_pos.get(), rank.get(), sa.get(), next_suffix->get(),
                    next_group->get());
    if (round == 0) R->unresolved_first = left;
    else { ++R->rounds; h *= 2; }
    if (round > 0 && h > 2 * N) return 1;
    list_suffix = std::move(next_suffix);
    list_group = std::move(next_group);
    M = left;
  }
  for (i64 r = 0; r < N; ++r)
    if (sa.get()[r] < 0 || sa.get()[r] > seq_len || rank.get()[sa.get()[r]] != r) return 2;
  const i64 primary = rank.get()[0];
  Block<uint32_t> words(S.n_words);
  for (i64 w = 0; w < S.n_words; ++w) words.get()[w] = xc::bwt_word(T, sa.get(), primary, w);
  Block<i64> cols(4 * (S.n_blocks + 1));
  for (i64 b = 0; b < S.n_blocks; ++b) xc::block_counts(words.get(), S, b, cols.get());
  scan_cols(cols.get(), 4, S.n_blocks);
  Block<uint32_t> out(S.bwt_size);
  for (i64 b = 0; b <= S.n_blocks; ++b) xc::pack_block(words.get(), S, b, cols.get(), out.get());
  Block<i64> samples(S.n_sa);
  for (i64 k = 0; k < S.n_sa; ++k) samples.get()[k] = xc::sample_at(sa.get(), k, sa_intv);
  R->primary = primary;
  R->L2[0] = 0;
  for (int c = 0; c < 4; ++c) R->L2[c + 1] = R->L2[c] + cols.get()[(i64)c * (S.n_blocks + 1) + S.n_blocks];
  R->seq_len = seq_len; R->bwt_size = S.bwt_size; R->n_sa = S.n_sa; R->passes = g_passes;
  R->bwt.assign(out.get(), out.get() + S.bwt_size);
  R->sa.assign(samples.get(), samples.get() + S.n_sa);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: index_host run IN OUT\n"); return 2; }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  for (int n_case = 0;; ++n_case) {
    i64 l_pac;
    int32_t par[4];
    if (fread(&l_pac, 8, 1, in) != 1) break;
    if (fread(par, 4, 4, in) != 4 || l_pac < 1) { fprintf(stderr, "case %d: short header\n", n_case); return 2; }
    std::vector<uint8_t> pac((size_t)((l_pac + 3) / 4));
    if (fread(pac.data(), 1, pac.size(), in) != pac.size()) { fprintf(stderr, "case %d: short pac\n", n_case); return 2; }
    Result R;
    const int rc = build(pac.data(), l_pac, par[0], par[1], par[2], &R);
    if (rc) { fprintf(stderr, "case %d: the construction failed (%d)\n", n_case, rc); return 1; }
    const i64 head[13] = {R.primary, R.L2[0], R.L2[1], R.L2[2], R.L2[3], R.L2[4], R.seq_len, R.bwt_size, R.n_sa, R.rounds, R.unresolved_first,
                          R.passes, R.tiles};
    fwrite(head, 8, 13, out);
    fwrite(R.bwt.data(), 4, R.bwt.size(), out);
    fwrite(R.sa.data(), 8, R.sa.size(), out);
  }
  fclose(in);
  if (fclose(out)) return 2;
  return 0;
}
