// bpsw_deflate_core.h -- one BGZF block as one dynamic-Huffman deflate block (RFC 1951, BTYPE 10) with LZ77 matches, for the host and
// for the device.  One wavefront of 64 lanes compresses one payload of n <= 65280 bytes; every function here is what one lane does in
// one phase, or what lane 0 does alone, and the caller puts a barrier between the phases.  bgzf_deflate_kernel (bpsw_bam.hip) runs them
// on 64 lanes; block_serial below, the host twin, plays the 64 lanes in a loop.  Both give the same bytes: nothing here depends on which
// lane runs first (the hash tables are a lane's own, the histograms are sums, the shared words of the bit stream are OR-ed into zeros).
//
//   lz_lane          lane l owns payload[l s, l s + s), s = ceil(n / 64) rounded up to four bytes (the CRC's slicing): a greedy search
//                    over a table of its own (kHashSize last positions of a 3-byte hash), warmed over the kWarm bytes in front of the
//                    slice, so a match may begin in earlier slices but never runs past the end of its own.  Tokens go to tok[], two
//                    bytes per payload byte, indexed by position: tok[p] < 256 is the literal at p; else tok[p] - 256 + 3 is a length
//                    and tok[p + 1] + 1 its distance (a match covers three positions at least).  Each token adds to the histograms.
//   rank_lane        the used symbols of an alphabet in ascending (count, symbol) order: a lane ranks the symbols it owns.
//   lengths_serial   lane 0: code lengths from the sorted counts (Moffat & Katajainen in place), limited to max_bits by moving codes
//                    between lengths until the Kraft sum is exact again, handed out longest to rarest.
//   header_serial    lane 0: canonical codes (RFC 1951 3.2.2) of the three alphabets and the number of bits of the block header.  The
//                    length lists are written a length at a time (no run-length symbols 16 / 17 / 18).
//   count_lane       the bits of a lane's tokens; an exclusive scan over the lanes gives where each lane's bits begin.
//   write_lane       header (lane 0), tokens, then (lane 63) the end-of-block code, the padding, CRC-32 and ISIZE, through a BitWriter:
//                    whole 32-bit words are stored, the first and last word of a lane are OR-ed into memory the caller has zeroed.
// When the deflate bytes are not fewer than n + 5 the caller writes the block stored, as bgzf_frame_kernel does.
//
// Plain C++; compiled by hipcc for bgzf_deflate_kernel and by g++ for tests/deflate_host/deflate_host.cpp.  No array of its own is
// indexed outside Work (LDS on the device), so the kernel has no scratch.
#pragma once

#include <stdint.h>

#include "bpsw_bam_core.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define BPSW_DEFL_ADD1(p) atomicAdd((p), 1u)
#define BPSW_DEFL_OR(p, v) atomicOr((p), (v))
#else
#define BPSW_DEFL_ADD1(p) (void)(*(p) += 1u)
#define BPSW_DEFL_OR(p, v) (void)(*(p) |= (v))
#endif

namespace bpsw {
namespace deflcore {

namespace bc = bpsw::bamcore;

constexpr int kLanes = 64;
constexpr int kHashBits = 9, kHashSize = 1 << kHashBits;
constexpr int kWarm = 1024;                               // bytes in front of a slice whose positions a lane enters before it starts
constexpr int kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768;
constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19, kEob = 256;
constexpr int kBitsLL = 15, kBitsCL = 7;
constexpr int kHead = 18;                                 // the BGZF header in front of the deflate bytes
constexpr int kStoredExtra = 5;                           // 01 LEN ~LEN: what a stored block has beside its payload

struct Work {                                             // a block's working memory: 70 892 bytes
  uint16_t hash[kHashSize * kLanes];                      // [h * 64 + lane]: position + 1 of the last entry, 0 for none
  uint32_t crc_tab[256];
  uint32_t ll_freq[288], d_freq[32], cl_freq[20];
  uint32_t key[288];                                      // the alphabet being built: counts in ascending order, then depths
  uint16_t idx[288];                                      //   and their symbols
  uint32_t num_codes[34], next_code[18];
  uint16_t ll_code[288], d_code[32], cl_code[20];         // bit-reversed: a code goes out from its first bit
  uint8_t ll_len[288], d_len[32], cl_len[20];
  int32_t hlit, hdist, hclen;
  uint32_t hdr_bits;
};

BPSW_SAM_HD int slice_of(int n) { return ((n + kLanes - 1) / kLanes + 3) & ~3; }
BPSW_SAM_HD int ilog2(uint32_t x) { return 31 - __builtin_clz(x); }

// ---- the symbols of a length and of a distance (RFC 1951 3.2.5), by arithmetic --------------------------------------------------------
BPSW_SAM_HD int len_extra_bits(int len) { const int l = len - 3; return (l < 8 || len == 258) ? 0 : ilog2((uint32_t)l) - 2; }
BPSW_SAM_HD int len_code(int len) {
  const int l = len - 3;
  if (l < 8) return 257 + l;
  if (len == 258) return 285;
  const int e = ilog2((uint32_t)l) - 2;
  return 261 + 4 * e + ((l >> e) & 3);
}
BPSW_SAM_HD uint32_t len_extra(int len) { return (uint32_t)(len - 3) & ((1u << len_extra_bits(len)) - 1u); }
BPSW_SAM_HD int dist_extra_bits(int dist) { const int d = dist - 1; return d < 4 ? 0 : ilog2((uint32_t)d) - 1; }
BPSW_SAM_HD int dist_code(int dist) {
  const int d = dist - 1;
  if (d < 4) return d;
  const int k = ilog2((uint32_t)d);
  return 2 * k + ((d >> (k - 1)) & 1);
}
BPSW_SAM_HD uint32_t dist_extra(int dist) { return (uint32_t)(dist - 1) & ((1u << dist_extra_bits(dist)) - 1u); }
// the order in which the code-length code's own lengths are written: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
BPSW_SAM_HD int cl_order(int k) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                          5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31);
}

// ---- phase 0: a lane's table, its share of the counts and of the CRC's table ----------------------------------------------------------
BPSW_SAM_HD void init_lane(Work& w, int lane) {
  for (int h = 0; h < kHashSize; ++h) w.hash[h * kLanes + lane] = 0;
  for (int i = lane; i < 288; i += kLanes) w.ll_freq[i] = 0;
  if (lane < 32) w.d_freq[lane] = 0;
  if (lane < 20) w.cl_freq[lane] = 0;
  for (int k = 0; k < 4; ++k) w.crc_tab[4 * lane + k] = bc::crc32_table_entry((uint32_t)(4 * lane + k));
}

// ---- phase 1: tokens ------------------------------------------------------------------------------------------------------------------
// the hash of the three bytes at p; `more`: a fourth byte may be read with them (one load instead of three)
BPSW_SAM_HD uint32_t hash3(const uint8_t* p, bool more) {
  uint32_t v;
  if (more) { __builtin_memcpy(&v, p, 4); v &= 0xffffffu; }  // (both sides are little-endian)
  else v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
  return (v * 0x9E3779B1u) >> (32 - kHashBits);
}
// the length of the match of src[pos ..) against src[cand ..), at most `limit`; 0 when it is shorter than three bytes or further back
// than a deflate distance reaches
BPSW_SAM_HD int match_len(const uint8_t* src, int pos, int cand, int limit) {
  if (cand >= pos || pos - cand > kMaxDist) return 0;
  int len = 0;
  for (; len + 8 <= limit; len += 8) {  // eight bytes a step while eight are left below the limit
    uint64_t a, b;
    __builtin_memcpy(&a, src + cand + len, 8);
    __builtin_memcpy(&b, src + pos + len, 8);
    if (a != b) { len += __builtin_ctzll(a ^ b) >> 3; return len >= kMinMatch ? len : 0; }
  }
  while (len < limit && src[cand + len] == src[pos + len]) ++len;
  return len >= kMinMatch ? len : 0;
}
BPSW_SAM_HD void lz_lane(Work& w, int lane, const uint8_t* src, int n, uint16_t* tok) {
  const int s = slice_of(n);
  const int lo = lane * s < n ? lane * s : n, hi = lo + s < n ? lo + s : n;
  uint16_t* H = w.hash + lane;
  for (int p = lo > kWarm ? lo - kWarm : 0; p < lo; ++p)
    if (p + kMinMatch <= n) H[hash3(src + p, p + 4 <= n) * kLanes] = (uint16_t)(p + 1);
  int pos = lo;
  while (pos < hi) {
    int len = 0, cand = 0;
    if (pos + kMinMatch <= hi) {
      const uint32_t h = hash3(src + pos, pos + 4 <= n);
      cand = (int)H[h * kLanes] - 1;
      H[h * kLanes] = (uint16_t)(pos + 1);
      if (cand >= 0) len = match_len(src, pos, cand, hi - pos < kMaxMatch ? hi - pos : kMaxMatch);
    }
    if (len) {
      const int dist = pos - cand;
      tok[pos] = (uint16_t)(256 + len - kMinMatch);
      tok[pos + 1] = (uint16_t)(dist - 1);
      BPSW_DEFL_ADD1(&w.ll_freq[len_code(len)]);
      BPSW_DEFL_ADD1(&w.d_freq[dist_code(dist)]);
      for (int q = pos + 1; q < pos + len; ++q)
        if (q + kMinMatch <= n) H[hash3(src + q, q + 4 <= n) * kLanes] = (uint16_t)(q + 1);
      pos += len;
    } else {
      tok[pos] = src[pos];
      BPSW_DEFL_ADD1(&w.ll_freq[src[pos]]);
      ++pos;
    }
  }
  if (lane == 0) BPSW_DEFL_ADD1(&w.ll_freq[kEob]);
}

// ---- phase 2: code lengths ------------------------------------------------------------------------------------------------------------
// the used symbols of freq[0, nsym) into key / idx in ascending (count, symbol) order: a lane places the symbols lane, lane + 64, ...
BPSW_SAM_HD void rank_lane(Work& w, const uint32_t* freq, int nsym, int lane) {
  for (int s = lane; s < nsym; s += kLanes) {
    const uint32_t f = freq[s];
    if (!f) continue;
    int r = 0;
    for (int t = 0; t < nsym; ++t) {
      const uint32_t g = freq[t];
      r += g && (g < f || (g == f && t < s));
    }
    w.key[r] = f;
    w.idx[r] = (uint16_t)s;
  }
}
// Lane 0, after rank_lane: len[0, nsym) from the sorted counts, no length above max_bits.  An alphabet with one used symbol gets one code
// of one bit, and one with none declares symbol 0 with one bit (a block without matches still has to name a distance code).
BPSW_SAM_HD void lengths_serial(Work& w, const uint32_t* freq, int nsym, int max_bits, uint8_t* len) {
  int n = 0;
  for (int s = 0; s < nsym; ++s) { len[s] = 0; n += freq[s] != 0; }
  if (n == 0) { len[0] = 1; return; }
  if (n == 1) { len[w.idx[0]] = 1; return; }
  uint32_t* A = w.key;
  // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": counts -> parents -> depths
  A[0] += A[1];
  int root = 0, leaf = 2, next;
  for (next = 1; next < n - 1; ++next) {
    if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
    if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
  }
  A[n - 2] = 0;
  for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
  int avbl = 1, used = 0, dpth = 0;
  root = n - 2; next = n - 1;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
    while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
    avbl = 2 * used; ++dpth; used = 0;
  }
  // the limit: every deeper code to max_bits, then codes moved a level down until the Kraft sum is 2^max_bits again
  for (int i = 0; i < 34; ++i) w.num_codes[i] = 0;
  for (int i = 0; i < n; ++i) ++w.num_codes[A[i] < (uint32_t)max_bits ? A[i] : (uint32_t)max_bits];
  uint32_t total = 0;
  for (int i = max_bits; i > 0; --i) total += w.num_codes[i] << (max_bits - i);
  while (total > (1u << max_bits)) {  // (a whole tree's sum is 2^max_bits before the deep codes are pulled up, so it starts at or above)
    --w.num_codes[max_bits];
    for (int i = max_bits - 1; i > 0; --i)
      if (w.num_codes[i]) { --w.num_codes[i]; w.num_codes[i + 1] += 2; break; }
    --total;
  }
  int j = n;
  for (int i = 1; i <= max_bits; ++i)
    for (uint32_t l = w.num_codes[i]; l > 0; --l) len[w.idx[--j]] = (uint8_t)i;
}
BPSW_SAM_HD uint32_t reverse_bits(uint32_t v, int nb) {
  uint32_t r = 0;
  for (int i = 0; i < nb; ++i) r |= ((v >> i) & 1u) << (nb - 1 - i);
  return r;
}
BPSW_SAM_HD void codes_serial(Work& w, const uint8_t* len, int nsym, uint16_t* code) {
  for (int i = 0; i < 18; ++i) w.num_codes[i] = 0;
  for (int s = 0; s < nsym; ++s) ++w.num_codes[len[s]];
  w.num_codes[0] = 0;
  uint32_t c = 0;
  for (int i = 1; i <= 16; ++i) { c = (c + w.num_codes[i - 1]) << 1; w.next_code[i] = c; }
  for (int s = 0; s < nsym; ++s) code[s] = len[s] ? (uint16_t)reverse_bits(w.next_code[len[s]]++, len[s]) : (uint16_t)0;
}
// lane 0, once both length lists stand: how many of each are declared, and the counts of the code-length alphabet
BPSW_SAM_HD void cl_counts_serial(Work& w) {
  int hlit = kNumLL, hdist = kNumD;
  while (hlit > 257 && !w.ll_len[hlit - 1]) --hlit;
  while (hdist > 1 && !w.d_len[hdist - 1]) --hdist;
  w.hlit = hlit; w.hdist = hdist;
  for (int i = 0; i < hlit; ++i) ++w.cl_freq[w.ll_len[i]];
  for (int i = 0; i < hdist; ++i) ++w.cl_freq[w.d_len[i]];
}

// ---- bits -----------------------------------------------------------------------------------------------------------------------------
struct BitCount {
  uint32_t n = 0;
  BPSW_SAM_HD void put(uint32_t, int nb) { n += (uint32_t)nb; }
};
// bits from position `bit` of words[] on, the first bit of a value first.  A word that is all this writer's is stored; its first word
// when it does not begin on a word, and what is left at finish(), are OR-ed: other writers hold the rest of those words, and the
// memory was zero before any of them began.
struct BitWriter {
  uint32_t* words;
  uint64_t acc = 0;
  int nacc;
  bool shared;
  BPSW_SAM_HD BitWriter(uint32_t* base, uint32_t bit) : words(base + (bit >> 5)), nacc((int)(bit & 31)), shared((bit & 31) != 0) {}
  BPSW_SAM_HD void put(uint32_t v, int nb) {  // nb <= 32, v < 2^nb
    acc |= (uint64_t)v << nacc;
    nacc += nb;
    if (nacc >= 32) {
      if (shared) BPSW_DEFL_OR(words, (uint32_t)acc); else *words = (uint32_t)acc;
      shared = false;
      ++words; acc >>= 32; nacc -= 32;
    }
  }
  BPSW_SAM_HD void finish() { if (acc) BPSW_DEFL_OR(words, (uint32_t)acc); }
};

template <class S> BPSW_SAM_HD void emit_header(S& s, const Work& w) {
  s.put(1u | 2u << 1, 3);  // BFINAL, BTYPE 10
  s.put((uint32_t)(w.hlit - 257), 5);
  s.put((uint32_t)(w.hdist - 1), 5);
  s.put((uint32_t)(w.hclen - 4), 4);
  for (int k = 0; k < w.hclen; ++k) s.put(w.cl_len[cl_order(k)], 3);
  for (int i = 0; i < w.hlit; ++i) s.put(w.cl_code[w.ll_len[i]], w.cl_len[w.ll_len[i]]);
  for (int i = 0; i < w.hdist; ++i) s.put(w.cl_code[w.d_len[i]], w.cl_len[w.d_len[i]]);
}
// lane 0, after the code-length alphabet's lengths: the three canonical codes, HCLEN, the header's bits
BPSW_SAM_HD void header_serial(Work& w) {
  codes_serial(w, w.ll_len, kNumLL, w.ll_code);
  codes_serial(w, w.d_len, kNumD, w.d_code);
  codes_serial(w, w.cl_len, kNumCL, w.cl_code);
  int hclen = kNumCL;
  while (hclen > 4 && !w.cl_len[cl_order(hclen - 1)]) --hclen;
  w.hclen = hclen;
  BitCount c;
  emit_header(c, w);
  w.hdr_bits = c.n;
}
template <class S> BPSW_SAM_HD void emit_tokens(S& s, const Work& w, int lane, int n, const uint16_t* tok) {
  const int sl = slice_of(n);
  const int lo = lane * sl < n ? lane * sl : n, hi = lo + sl < n ? lo + sl : n;
  for (int pos = lo; pos < hi;) {
    const int t = tok[pos];
    if (t < 256) { s.put(w.ll_code[t], w.ll_len[t]); ++pos; continue; }
    const int len = t - 256 + kMinMatch, dist = (int)tok[pos + 1] + 1;
    const int lc = len_code(len), dc = dist_code(dist);
    s.put(w.ll_code[lc], w.ll_len[lc]);
    s.put(len_extra(len), len_extra_bits(len));
    s.put(w.d_code[dc], w.d_len[dc]);
    s.put(dist_extra(dist), dist_extra_bits(dist));
    pos += len;
  }
}
BPSW_SAM_HD uint32_t count_lane(const Work& w, int lane, int n, const uint16_t* tok) {
  BitCount c;
  emit_tokens(c, w, lane, n, tok);
  return c.n;
}
// the bytes of the deflate block whose lanes' tokens take `token_bits` in all
BPSW_SAM_HD uint32_t deflate_bytes(const Work& w, uint32_t token_bits) { return (w.hdr_bits + token_bits + w.ll_len[kEob] + 7) >> 3; }
// A lane's part of the framed block.  words: the block's place + 16, four-byte aligned and zero from there to the block's end
// (18 + dbytes + 8 bytes, rounded up to a word); bytes 0 .. 15 of the block are the caller's (bgzf_deflate_head_byte).  before: the bits
// of the lanes below this one.
BPSW_SAM_HD void write_lane(const Work& w, int lane, int n, const uint16_t* tok, uint32_t* words, uint32_t before, uint32_t token_bits, uint32_t crc) {
  const uint32_t dbytes = deflate_bytes(w, token_bits);
  BitWriter s(words, lane == 0 ? 0u : 16u + w.hdr_bits + before);
  if (lane == 0) {
    s.put((uint32_t)bc::bgzf_deflate_head_byte(16, dbytes) | (uint32_t)bc::bgzf_deflate_head_byte(17, dbytes) << 8, 16);
    emit_header(s, w);
  }
  emit_tokens(s, w, lane, n, tok);
  if (lane == kLanes - 1) {
    s.put(w.ll_code[kEob], w.ll_len[kEob]);
    s.put(0u, (int)(8u * dbytes - (w.hdr_bits + token_bits + w.ll_len[kEob])));
    for (int k = 0; k < bc::kBgzfTail; ++k) s.put(bc::bgzf_tail_byte(k, crc, (uint32_t)n), 8);
  }
  s.finish();
}
// the CRC's share of a lane (bgzf_frame_kernel's fold): XOR the 64 of them
BPSW_SAM_HD uint32_t crc_lane(const Work& w, int lane, const uint8_t* src, int n) {
  const int s = slice_of(n);
  const int lo = lane * s < n ? lane * s : n, hi = lo + s < n ? lo + s : n;
  return bc::crc32_shift(bc::crc32_bytes(w.crc_tab, 0u, src + lo, hi - lo), n - hi);
}

// ---- the host twin: the 64 lanes in a loop ----------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
// One block: src[0, n), 1 <= n <= 65280, framed at dst, which is four-byte aligned and has room for n + 31 bytes rounded up to a word;
// tok has room for n entries.  Returns the framed size: 18 + deflate bytes + 8, or n + 31 for a block written stored.
inline uint32_t block_serial(Work& w, const uint8_t* src, int n, uint16_t* tok, uint8_t* dst) {
  for (int l = 0; l < kLanes; ++l) init_lane(w, l);
  for (int l = 0; l < kLanes; ++l) lz_lane(w, l, src, n, tok);
  for (int l = 0; l < kLanes; ++l) rank_lane(w, w.ll_freq, kNumLL, l);
  lengths_serial(w, w.ll_freq, kNumLL, kBitsLL, w.ll_len);
  for (int l = 0; l < kLanes; ++l) rank_lane(w, w.d_freq, kNumD, l);
  lengths_serial(w, w.d_freq, kNumD, kBitsLL, w.d_len);
  cl_counts_serial(w);
  for (int l = 0; l < kLanes; ++l) rank_lane(w, w.cl_freq, kNumCL, l);
  lengths_serial(w, w.cl_freq, kNumCL, kBitsCL, w.cl_len);
  header_serial(w);
  uint32_t before[kLanes], total = 0, crc = 0;
  for (int l = 0; l < kLanes; ++l) { before[l] = total; total += count_lane(w, l, n, tok); crc ^= crc_lane(w, l, src, n); }
  const uint32_t dbytes = deflate_bytes(w, total);
  if (dbytes >= (uint32_t)n + kStoredExtra) {
    for (int k = 0; k < bc::kBgzfHead; ++k) dst[k] = bc::bgzf_head_byte(k, (uint32_t)n);
    for (int k = 0; k < n; ++k) dst[bc::kBgzfHead + k] = src[k];
    for (int k = 0; k < bc::kBgzfTail; ++k) dst[bc::kBgzfHead + n + k] = bc::bgzf_tail_byte(k, crc, (uint32_t)n);
    return (uint32_t)n + bc::kBgzfAround;
  }
  const uint32_t framed = kHead + dbytes + bc::kBgzfTail;
  uint32_t* words = reinterpret_cast<uint32_t*>(dst + 16);
  for (uint32_t k = 0; k < (framed - 16 + 3) / 4; ++k) words[k] = 0;
  for (int k = 0; k < 16; ++k) dst[k] = bc::bgzf_deflate_head_byte(k, dbytes);
  for (int l = 0; l < kLanes; ++l) write_lane(w, l, n, tok, words, before[l], total, crc);
  return framed;
}
#endif

}  // namespace deflcore
}  // namespace bpsw
