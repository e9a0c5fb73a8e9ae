// bpsw_index_core.h -- the arithmetic of the FM-index construction (bpsw_index.hip), shared with its host twin
// (tests/index_host/index_host.cpp): what one lane computes in every kernel, as functions of the item's index and the arrays.
// The kernels and the twin differ only in who walks the indices.
//
// The text is the doubled sequence read from the forward pac bytes, N = seq_len + 1 suffixes (suffix seq_len is the sentinel alone,
// which sorts below every base).  Every position, rank and count is 64-bit.
//
//   first key   k0 bases two bits each, zero-padded past the end, then min(remaining length, k0) in the low bits: a shorter suffix
//               sorts below a longer one with the same padded bases, and two suffixes with EQUAL keys both have k0 bases or more.
//   list        the suffixes in play: (key, suffix) pairs, groups contiguous and ascending.  Round 0's list is every suffix with
//               the first key; a later round's key is group << rank_bits | rank[suffix + h].
//   after a sort  run heads (key differs from the entry before), group heads (group differs), keep (the entry's run has a second
//               member): three columns, summed by the device scan; two tables give every run and group its first list position.
//               An entry's new rank is its group + (head of its run - head of its group): a group's members stand at consecutive
//               suffix-array rows from the group's rank on, in list order.  A run of one is final: it goes to the suffix array.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BPSW_IDX_HD __host__ __device__ __forceinline__
#else
#define BPSW_IDX_HD inline
#endif

namespace bpsw {
namespace idxcore {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kMaxFirstKey = 29;   // 58 bits of bases + 5 bits of length: as many bases as fit 64 bits
constexpr int kRadixBits = 8, kRadix = 1 << kRadixBits;
constexpr int kSortThreads = 256, kSortWaves = kSortThreads / 64;
constexpr int kSortTile = 4096;    // suffixes per workgroup of the sort: 16 steps of 256

struct Text {
  const uint8_t* pac;
  i64 l_pac;
};

// base i of the doubled text, 0 <= i < 2 l_pac
BPSW_IDX_HD int text_base(const Text& T, i64 i) {
  const bool fwd = i < T.l_pac;
  const i64 k = fwd ? i : 2 * T.l_pac - 1 - i;
  const int b = (T.pac[k >> 2] >> ((~k & 3) << 1)) & 3;
  return fwd ? b : 3 - b;
}

BPSW_IDX_HD int bits_for(u64 max_value) {  // bits that hold 0 .. max_value
  int b = 0;
  while (b < 64 && (max_value >> b)) ++b;
  return b;
}
BPSW_IDX_HD int first_key_bits(int k0) { return 2 * k0 + bits_for((u64)k0); }
BPSW_IDX_HD int radix_passes(int bits) { return (bits + kRadixBits - 1) / kRadixBits; }

// the first key of suffix i, 0 <= i <= seq_len
BPSW_IDX_HD u64 first_key(const Text& T, i64 i, int k0) {
  const i64 rem = 2 * T.l_pac - i;
  u64 k = 0;
  for (int j = 0; j < k0; ++j) k = k << 2 | (u64)(j < rem ? text_base(T, i + j) : 0);
  return k << bits_for((u64)k0) | (u64)(rem < k0 ? rem : k0);
}

// a later round's key: the suffix's group above the rank of the suffix h further on (the sentinel's, 0, where that is the end)
BPSW_IDX_HD u64 round_key(const i64* rank, i64 seq_len, i64 suffix, i64 group, i64 h, int rank_bits) {
  const i64 at = suffix + h;
  const u64 key2 = at <= seq_len ? (u64)rank[at] : 0;
  return (u64)group << rank_bits | key2;
}

BPSW_IDX_HD int digit_of(u64 key, int shift) { return (int)(key >> shift) & (kRadix - 1); }
BPSW_IDX_HD u64 group_of(u64 key, int group_shift) { return group_shift >= 64 ? 0 : key >> group_shift; }

// ---- after a sort: entry m of a list of M -------------------------------------------------------------------------------------
struct Flags {
  int run, group, keep;
};
BPSW_IDX_HD Flags flags_at(const u64* K, i64 M, i64 m, int group_shift) {
  Flags f;
  f.run = m == 0 || K[m] != K[m - 1];
  f.group = m == 0 || group_of(K[m], group_shift) != group_of(K[m - 1], group_shift);
  const int next_run = m == M - 1 || K[m + 1] != K[m];
  f.keep = !(f.run && next_run);
  return f;
}
// the three columns of the scan, each of M + 1 entries
BPSW_IDX_HD void flags_write(const u64* K, i64 M, i64 m, int group_shift, i64* cols) {
  const Flags f = flags_at(K, M, m, group_shift);
  cols[m] = f.run;
  cols[(M + 1) + m] = f.group;
  cols[2 * (M + 1) + m] = f.keep;
}
// ... scanned: the list position of every run's and every group's head
BPSW_IDX_HD void heads_write(const u64* K, i64 M, i64 m, int group_shift, const i64* cols, i64* run_pos, i64* group_pos) {
  const Flags f = flags_at(K, M, m, group_shift);
  if (f.run) run_pos[cols[m]] = m;
  if (f.group) group_pos[cols[(M + 1) + m]] = m;
}
// ... and the entry's new rank; a run of one to the suffix array, the others to the next list
BPSW_IDX_HD void assign_at(const u64* K, const i64* V, i64 M, i64 m, int group_shift, const i64* cols, const i64* run_pos, const i64* group_pos,
                           i64* rank, i64* sa, i64* next_suffix, i64* next_group) {
  const Flags f = flags_at(K, M, m, group_shift);
  const i64 head = run_pos[cols[m] + f.run - 1], ghead = group_pos[cols[(M + 1) + m] + f.group - 1];
  const i64 r = (i64)group_of(K[m], group_shift) + (head - ghead);
  const i64 suffix = V[m];
  rank[suffix] = r;
  if (!f.keep) sa[r] = suffix;
  else {
    const i64 p = cols[2 * (M + 1) + m];
    next_suffix[p] = suffix;
    next_group[p] = r;
  }
}

// ---- the index from the suffix array ------------------------------------------------------------------------------------------
struct Shape {
  i64 seq_len, n_words, n_blocks, bwt_size, n_sa;
};
BPSW_IDX_HD Shape shape_of(i64 l_pac, i64 sa_intv) {
  Shape s;
  s.seq_len = 2 * l_pac;
  s.n_words = (s.seq_len + 15) / 16;
  s.n_blocks = (s.seq_len + 127) / 128;
  s.bwt_size = s.n_words + (s.n_blocks + 1) * 8;
  s.n_sa = (s.seq_len + sa_intv) / sa_intv;
  return s;
}
// word w of the BWT's bases: base p = 16 w + j is T[SA[row] - 1] of row p + (p >= primary), the sentinel's row passed over
BPSW_IDX_HD uint32_t bwt_word(const Text& T, const i64* sa, i64 primary, i64 w) {
  const i64 seq_len = 2 * T.l_pac;
  uint32_t x = 0;
  for (int j = 0; j < 16; ++j) {
    const i64 p = 16 * w + j;
    if (p >= seq_len) break;
    const i64 s = sa[p + (p >= primary)];
    x |= (uint32_t)(s > 0 ? text_base(T, s - 1) : 0) << (30 - 2 * j);  // (s == 0 is the passed-over row's alone)
  }
  return x;
}
// the four counts of block b's bases, into the four columns of n_blocks + 1 entries
BPSW_IDX_HD void block_counts(const uint32_t* words, const Shape& S, i64 b, i64* cols) {
  i64 cnt[4] = {0, 0, 0, 0};
  for (i64 w = 8 * b; w < 8 * b + 8 && w < S.n_words; ++w) {
    const uint32_t x = words[w];
    const i64 left = S.seq_len - 16 * w;
    const int n = left < 16 ? (int)left : 16;
    for (int j = 0; j < n; ++j) ++cnt[(x >> (30 - 2 * j)) & 3];
  }
  for (int c = 0; c < 4; ++c) cols[(i64)c * (S.n_blocks + 1) + b] = cnt[c];
}
// block b of the interleaved array, 0 <= b <= n_blocks (the last: the counts behind the last base word)
BPSW_IDX_HD void pack_block(const uint32_t* words, const Shape& S, i64 b, const i64* cols, uint32_t* out) {
  uint32_t* o = out + (b < S.n_blocks ? 16 * b : 8 * S.n_blocks + S.n_words);
  for (int c = 0; c < 4; ++c) {
    const u64 v = (u64)cols[(i64)c * (S.n_blocks + 1) + b];
    o[2 * c] = (uint32_t)v;
    o[2 * c + 1] = (uint32_t)(v >> 32);
  }
  if (b < S.n_blocks)
    for (i64 w = 8 * b; w < 8 * b + 8 && w < S.n_words; ++w) o[8 + (w - 8 * b)] = words[w];
}
BPSW_IDX_HD i64 sample_at(const i64* sa, i64 k, i64 sa_intv) { return k == 0 ? -1 : sa[k * sa_intv]; }

}  // namespace idxcore
}  // namespace bpsw
