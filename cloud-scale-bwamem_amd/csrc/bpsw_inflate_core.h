// bpsw_inflate_core.h -- BGZF blocks back to their bytes: the header walk of a chunk, and the inflate of one block's deflate data
// (RFC 1951: stored, fixed and dynamic deflate blocks, any number of them) by one wavefront of 64 lanes, for the host and for the device.
//
// Decoding is wave-uniform: every lane holds the same bit reader and walks the same symbols; what differs per lane is which bytes of
// the output it stores.  The lanes meet through an executor X, which says how the 64 lanes run a phase:
//   x.each(f)       f(lane) for every lane, and what the lanes stored to Work is ordered in front of whatever any lane reads next
//   x.barrier()     the same ordering without work (between a uniform store by lane 0 and the reads of all)
//   x.lane0()       whether the caller is the one that stores a uniform value
//   x.fold_xor(f)   the XOR of f(lane) over the lanes
// bgzf_inflate_kernel (bpsw_bgzf_in.hip) passes the wavefront itself (a lane runs f once; the ordering is a wave-scope fence, as the
// LDS executes one wave's accesses in the order they were issued); inflate_serial below, the host twin, passes SerialExec, which
// plays the 64 lanes in a loop.  Both run inflate_member, so both give the same bytes or the same reason.
//
//   bgzf_walk        host: the blocks a chunk wholly holds -- where each begins, where its deflate data lies, ISIZE and CRC-32 from the
//                    trailer, where its bytes go in the output (the prefix sum of ISIZE) -- or the first malformed header
//   BitReader        64 bits of look-ahead over the deflate bytes, filled 32 bits at a time with the next word already on its way;
//                    no load at or past the end of the data (zero bits stand there), and over() says that bits beyond it were used
//   build_tables     from code lengths in Work::len: per alphabet the codes per length, the symbols in canonical order (a lane
//                    ranks the symbols it owns) and a first-level table of 2^10 entries (symbol << 4 | length) filled by all lanes;
//                    a code longer than 10 bits is found by the canonical count walk over its 15 bits
//   inflate_member   the deflate blocks of one member into Work::win, then the length and the CRC-32 (crc32_bytes per lane slice,
//                    crc32_shift, XOR fold).  The first error in stream order is the one returned; length and CRC come last.
//
// Plain C++; compiled by hipcc for the kernel and by g++ for tests/inflate_host/inflate_host.cpp.  Every array is in Work (LDS on the
// device): the kernel has no scratch.
#pragma once

#include <stdint.h>

#include "bpsw_deflate_core.h"  // cl_order, slice_of, kLanes (and bpsw_bam_core.h: the CRC)

#if defined(__HIP_DEVICE_COMPILE__)
#define BPSW_INFL_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))  // a value every lane has: keep it where scalars live
#else
#define BPSW_INFL_UNI(v) ((uint32_t)(v))
#endif

namespace bpsw {
namespace inflcore {

namespace bc = bpsw::bamcore;
namespace dc = bpsw::deflcore;

constexpr int kLanes = dc::kLanes;
constexpr int kMaxIsize = 65536;                 // htslib's BGZF_MAX_BLOCK_SIZE
constexpr int kFastBits = 10, kFastSize = 1 << kFastBits;
constexpr int kClBits = 7, kClFast = 1 << kClBits;
constexpr int kMinBlock = 12 + 6 + 2 + 8;        // gzip header, the BC subfield, an empty fixed block, the trailer

enum Reason {
  R_OK = 0,
  // a block's header (bgzf_walk)
  R_MAGIC = 1, R_NO_BC, R_BSIZE, R_ISIZE,
  // a block's deflate data (inflate_member), in no order that matters: the first met is reported
  R_BTYPE, R_STORED_LEN, R_HLIT, R_HDIST, R_CL_OVER, R_CL_INCOMPLETE, R_REPEAT_FIRST, R_RUN_PAST, R_NO_EOB, R_LL_OVER, R_LL_INCOMPLETE,
  R_D_OVER, R_D_INCOMPLETE, R_BAD_CODE, R_LL_SYMBOL, R_D_SYMBOL, R_DIST_BEFORE, R_DATA_ENDS, R_TOO_LONG,
  // after the last deflate block
  R_TOO_SHORT, R_CRC,
  R_COUNT
};

struct Block {  // one BGZF block of a chunk
  uint32_t coff;               // where it begins in the chunk
  uint32_t data_off, data_len; // its deflate data
  uint32_t isize, crc;         // the trailer's
  uint32_t out_off;            // where its bytes go: the sum of ISIZE of the blocks in front
};

struct Work {                  // a block's working memory: 71 828 bytes
  uint8_t win[kMaxIsize];      // the member's output
  uint32_t crc_tab[256];
  uint16_t ll_fast[kFastSize], d_fast[kFastSize];  // symbol << 4 | code length, 0: the code is longer than kFastBits (or none)
  uint16_t ll_sym[288], d_sym[32];                 // the used symbols in ascending (length, symbol) order
  uint16_t ll_count[16], d_count[16];              // codes per length
  uint8_t len[288 + 32];       // the literal/length lengths, the distance lengths behind them
  uint8_t cl_len[20];
  uint8_t cl_fast[kClFast];    // symbol << 3 | code length (the code-length code is complete: every entry is filled)
};

// ---- the bit reader -----------------------------------------------------------------------------------------------------------------
struct BitReader {
  const uint8_t* p;
  uint32_t len;    // the bytes of the data: nothing at or past p + len is loaded
  uint32_t at;     // bytes taken into acc (it runs past len: zeros stand there)
  uint64_t acc;
  int n;           // bits in acc
  uint32_t ahead;  // the bytes [at, at + 4), loaded when the word before them went into acc
  BPSW_SAM_HD uint32_t load32(uint32_t o) const {
    uint32_t v = 0;
    if (o + 4 <= len && o + 4 > o) __builtin_memcpy(&v, p + o, 4);  // (both sides are little-endian)
    else
      for (int k = 0; k < 4; ++k)
        if (o + k < len && o + k >= o) v |= (uint32_t)p[o + k] << (8 * k);
    return BPSW_INFL_UNI(v);
  }
  BPSW_SAM_HD void seek(uint32_t o) { at = o; acc = 0; n = 0; ahead = load32(o); }
  BPSW_SAM_HD BitReader(const uint8_t* data, uint32_t bytes) : p(data), len(bytes) { seek(0); }
  BPSW_SAM_HD void refill() {  // at least 33 bits afterwards
    if (n <= 32) { acc |= (uint64_t)ahead << n; n += 32; at += 4; ahead = load32(at); }
  }
  BPSW_SAM_HD uint32_t peek(int nb) const { return (uint32_t)(acc & ((1ull << nb) - 1ull)); }
  BPSW_SAM_HD void drop(int nb) { acc >>= nb; n -= nb; }
  BPSW_SAM_HD uint32_t take(int nb) { const uint32_t v = peek(nb); drop(nb); return v; }
  BPSW_SAM_HD uint32_t bits(int nb) { refill(); return take(nb); }  // nb <= 32
  BPSW_SAM_HD bool over() const { return 8ull * at - (unsigned long long)n > 8ull * len; }  // bits beyond the data were used
  BPSW_SAM_HD void align() { drop(n & 7); }
  BPSW_SAM_HD uint32_t byte_pos() const { return at - (uint32_t)(n >> 3); }  // after align()
};

// ---- lengths and distances (RFC 1951 3.2.5) from their symbols, by arithmetic ----------------------------------------------------------
BPSW_SAM_HD int len_extra_bits_of(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
BPSW_SAM_HD int len_base_of(int sym) {
  if (sym < 265) return sym - 254;
  if (sym == 285) return 258;
  return 3 + ((4 + ((sym - 261) & 3)) << ((sym - 261) >> 2));
}
BPSW_SAM_HD int dist_extra_bits_of(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
BPSW_SAM_HD int dist_base_of(int sym) { return sym < 4 ? sym + 1 : 1 + ((2 + (sym & 1)) << ((sym >> 1) - 1)); }

// ---- tables ---------------------------------------------------------------------------------------------------------------------------
// What the codes per length say about a set of `n` lengths: 0, or over / incomplete.  lone_ok: the set may be a single code of one
// bit, or empty (zlib's inflate takes both for distances; a match in such a block meets R_BAD_CODE when it names no code).
BPSW_SAM_HD int kraft_check(const uint16_t* count, int n, bool lone_ok, int r_over, int r_incomplete) {
  int left = 1, used = 0;
  for (int l = 1; l <= 15; ++l) {
    const int c = (int)BPSW_INFL_UNI(count[l]);
    used += c;
    left = 2 * left - c;
    if (left < 0) return r_over;
  }
  if (left == 0) return 0;
  if (lone_ok && (used == 0 || (used == 1 && BPSW_INFL_UNI(count[1]) == 1))) return 0;
  return r_incomplete;
}
// lane `which` (0 .. 15) counts the codes of its length
BPSW_SAM_HD void count_lane(const uint8_t* len, int n, uint16_t* count, int which) {
  int c = 0;
  for (int s = 0; s < n; ++s) c += len[s] == which;
  count[which] = (uint16_t)(which ? c : 0);
}
// a lane's symbols (lane, lane + 64, ...): their place in canonical order, and their entries of the first-level table
BPSW_SAM_HD void rank_fill_lane(const uint8_t* len, int n, const uint16_t* count, uint16_t* sym, uint16_t* fast, int lane) {
  for (int s = lane; s < n; s += kLanes) {
    const int l = len[s];
    if (!l) continue;
    int r = 0, same = 0;
    for (int t = 0; t < n; ++t) {
      const int lt = len[t];
      r += lt && lt < l;
      same += lt == l && t < s;
    }
    sym[r + same] = (uint16_t)s;
    if (l > kFastBits) continue;
    uint32_t code = 0;  // the first code of length l (RFC 1951 3.2.2), then this symbol's
    for (int b = 1; b < l; ++b) code = (code + count[b]) << 1;
    code += (uint32_t)same;
    const uint32_t rev = dc::reverse_bits(code, l);
    for (uint32_t k = rev; k < (uint32_t)kFastSize; k += 1u << l) fast[k] = (uint16_t)(s << 4 | l);
  }
}
// Work::len[0, nll) and [nll, nll + nd) -> the two alphabets' tables; 0 or the refusal
template <class X> BPSW_SAM_HD int build_tables(Work& w, const X& x, int nll, int nd) {
  x.each([&](int lane) {
    for (int k = lane; k < kFastSize; k += kLanes) { w.ll_fast[k] = 0; w.d_fast[k] = 0; }
    if (lane < 16) count_lane(w.len, nll, w.ll_count, lane);
    else if (lane < 32) count_lane(w.len + nll, nd, w.d_count, lane - 16);
  });
  if (!BPSW_INFL_UNI(w.len[256])) return R_NO_EOB;
  int r = kraft_check(w.ll_count, nll, false, R_LL_OVER, R_LL_INCOMPLETE);
  if (!r) r = kraft_check(w.d_count, nd, true, R_D_OVER, R_D_INCOMPLETE);
  if (r) return r;
  x.each([&](int lane) {
    rank_fill_lane(w.len, nll, w.ll_count, w.ll_sym, w.ll_fast, lane);
    rank_fill_lane(w.len + nll, nd, w.d_count, w.d_sym, w.d_fast, lane);
  });
  return 0;
}
// the next symbol of an alphabet (the reader holds 15 bits at least); -1: the bits are no code of it
BPSW_SAM_HD int decode_sym(BitReader& br, const uint16_t* fast, const uint16_t* count, const uint16_t* sym) {
  const uint32_t v = br.peek(15);
  const uint32_t e = BPSW_INFL_UNI(fast[v & (uint32_t)(kFastSize - 1)]);
  if (e) { br.drop((int)(e & 15)); return (int)(e >> 4); }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((v >> (l - 1)) & 1u);
    const int c = (int)BPSW_INFL_UNI(count[l]);
    if (code - c < first) { br.drop(l); return (int)BPSW_INFL_UNI(sym[index + (code - first)]); }
    index += c; first += c;
    first <<= 1; code <<= 1;
  }
  return -1;
}

// the header of a dynamic block: HLIT, HDIST, the code-length code, the two length lists into Work::len
template <class X> BPSW_SAM_HD int read_dynamic(Work& w, const X& x, BitReader& br, int* nll, int* nd) {
  const int hlit = (int)br.bits(5) + 257, hdist = (int)br.take(5) + 1, hclen = (int)br.take(4) + 4;
  if (br.over()) return R_DATA_ENDS;
  if (hlit > 286) return R_HLIT;
  if (hdist > 30) return R_HDIST;
  for (int k = 0; k < 19; ++k) {
    const uint32_t v = k < hclen ? br.bits(3) : 0u;
    if (x.lane0()) w.cl_len[dc::cl_order(k)] = (uint8_t)v;
  }
  if (br.over()) return R_DATA_ENDS;
  x.barrier();
  {
    int left = 1;
    for (int l = 1; l <= kClBits; ++l) {
      int c = 0;
      for (int s = 0; s < 19; ++s) c += BPSW_INFL_UNI(w.cl_len[s]) == (uint32_t)l;
      left = 2 * left - c;
      if (left < 0) return R_CL_OVER;
    }
    if (left > 0) return R_CL_INCOMPLETE;
  }
  x.each([&](int lane) {
    if (lane >= 19) return;
    const int l = w.cl_len[lane];
    if (!l) return;
    uint32_t code = 0;
    for (int b = 1; b < l; ++b) {
      int c = 0;
      for (int s = 0; s < 19; ++s) c += w.cl_len[s] == b;
      code = (code + (uint32_t)c) << 1;
    }
    for (int s = 0; s < lane; ++s) code += w.cl_len[s] == l;
    for (uint32_t k = dc::reverse_bits(code, l); k < (uint32_t)kClFast; k += 1u << l) w.cl_fast[k] = (uint8_t)(lane << 3 | l);
  });
  const int total = hlit + hdist;
  int i = 0, prev = 0;
  while (i < total) {
    br.refill();
    const uint32_t e = BPSW_INFL_UNI(w.cl_fast[br.peek(kClBits)]);
    br.drop((int)(e & 7));
    const int s = (int)(e >> 3);
    int rep = 1, val = s;
    if (s == 16) { rep = 3 + (int)br.take(2); val = prev; }
    else if (s == 17) { rep = 3 + (int)br.take(3); val = 0; }
    else if (s == 18) { rep = 11 + (int)br.take(7); val = 0; }
    if (br.over()) return R_DATA_ENDS;
    if (s == 16 && i == 0) return R_REPEAT_FIRST;
    if (i + rep > total) return R_RUN_PAST;
    if (x.lane0())
      for (int k = 0; k < rep; ++k) w.len[i + k] = (uint8_t)val;
    i += rep;
    prev = val;
  }
  x.barrier();
  *nll = hlit; *nd = hdist;
  return 0;
}

// ---- one member -----------------------------------------------------------------------------------------------------------------------
// data[0, dlen): the deflate data of a block whose trailer says isize (<= kMaxIsize) and crc.  0 and win[0, isize) are its bytes, or the
// first reason met.
template <class X> BPSW_SAM_HD int inflate_member(Work& w, const X& x, const uint8_t* data, uint32_t dlen, uint32_t isize, uint32_t crc) {
  x.each([&](int lane) {
    for (int k = 0; k < 4; ++k) w.crc_tab[4 * lane + k] = bc::crc32_table_entry((uint32_t)(4 * lane + k));
  });
  BitReader br(data, dlen);
  uint32_t pos = 0;
  for (;;) {
    const uint32_t hdr = br.bits(3);
    if (br.over()) return R_DATA_ENDS;
    const int btype = (int)(hdr >> 1);
    if (btype == 3) return R_BTYPE;
    if (btype == 0) {
      br.align();
      const uint32_t v = br.bits(32);
      if (br.over()) return R_DATA_ENDS;
      const uint32_t n = v & 0xffffu;
      if ((n ^ (v >> 16)) != 0xffffu) return R_STORED_LEN;
      const uint32_t from = br.byte_pos(), have = dlen - from, room = isize - pos;
      if (n > have && have <= room) return R_DATA_ENDS;
      if (n > room) return R_TOO_LONG;
      x.each([&](int lane) {
        for (uint32_t i = (uint32_t)lane; i < n; i += kLanes) w.win[pos + i] = data[from + i];
      });
      pos += n;
      br.seek(from + n);
    } else {
      int nll = 288, nd = 32, r = 0;
      if (btype == 1) {  // the fixed code as a list of lengths (its 288 / 32 symbols make both sets complete)
        x.each([&](int lane) {
          for (int k = lane; k < 320; k += kLanes) w.len[k] = (uint8_t)(k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : k < 288 ? 8 : 5);
        });
      } else {
        r = read_dynamic(w, x, br, &nll, &nd);
      }
      if (!r) r = build_tables(w, x, nll, nd);
      if (r) return r;
      for (;;) {
        br.refill();
        const int s = decode_sym(br, w.ll_fast, w.ll_count, w.ll_sym);
        if (br.over()) return R_DATA_ENDS;
        if (s < 0) return R_BAD_CODE;
        if (s < 256) {
          if (pos == isize) return R_TOO_LONG;
          x.each([&](int lane) {
            if (lane == (int)(pos & (kLanes - 1))) w.win[pos] = (uint8_t)s;
          });
          ++pos;
          continue;
        }
        if (s == 256) break;
        if (s > 285) return R_LL_SYMBOL;
        const uint32_t len = (uint32_t)len_base_of(s) + br.take(len_extra_bits_of(s));
        br.refill();
        const int t = decode_sym(br, w.d_fast, w.d_count, w.d_sym);
        if (br.over()) return R_DATA_ENDS;
        if (t < 0) return R_BAD_CODE;
        if (t > 29) return R_D_SYMBOL;
        const uint32_t dist = (uint32_t)dist_base_of(t) + br.take(dist_extra_bits_of(t));
        if (br.over()) return R_DATA_ENDS;
        if (dist > pos) return R_DIST_BEFORE;
        if (len > isize - pos) return R_TOO_LONG;
        x.each([&](int lane) {  // byte i from the `dist` bytes in front of the match, again and again when it is longer than they are
          for (uint32_t i = (uint32_t)lane; i < len; i += kLanes) w.win[pos + i] = w.win[pos - dist + (i < dist ? i : i % dist)];
        });
        pos += len;
      }
    }
    if (hdr & 1u) break;
  }
  if (pos != isize) return R_TOO_SHORT;  // (bits left in the data are ignored, as zlib does)
  const uint32_t got = x.fold_xor([&](int lane) {
    const int n = (int)isize, s = dc::slice_of(n);
    const int lo = lane * s < n ? lane * s : n, hi = lo + s < n ? lo + s : n;
    return bc::crc32_shift(bc::crc32_bytes(w.crc_tab, 0u, w.win + lo, hi - lo), n - hi);
  });
  return got == crc ? 0 : R_CRC;
}

}  // namespace inflcore
}  // namespace bpsw

// ---- host functions: the reasons' texts, the header walk, the twin ----------------------------------------------------------------------
#include <string.h>

#include <vector>

namespace bpsw {
namespace inflcore {

inline const char* inflate_reason_text(int reason) {
  switch (reason) {
    case R_MAGIC: return "the block does not begin with 1f 8b 08 04 (not a BGZF block)";
    case R_NO_BC: return "no BC subfield in the gzip header (plain gzip, not BGZF)";
    case R_BSIZE: return "BSIZE and the extra field are inconsistent";
    case R_ISIZE: return "ISIZE is above 65536";
    case R_BTYPE: return "a deflate block of type 11";
    case R_STORED_LEN: return "a stored block whose LEN is not the complement of NLEN";
    case R_HLIT: return "HLIT above 286";
    case R_HDIST: return "HDIST above 30";
    case R_CL_OVER: return "the code-length code is over-subscribed";
    case R_CL_INCOMPLETE: return "the code-length code is incomplete";
    case R_REPEAT_FIRST: return "a repeat of the previous length with no length in front";
    case R_RUN_PAST: return "a run of lengths past HLIT + HDIST";
    case R_NO_EOB: return "the literal/length code has no end-of-block symbol";
    case R_LL_OVER: return "the literal/length code is over-subscribed";
    case R_LL_INCOMPLETE: return "the literal/length code is incomplete";
    case R_D_OVER: return "the distance code is over-subscribed";
    case R_D_INCOMPLETE: return "the distance code is incomplete";
    case R_BAD_CODE: return "bits that are no code of the block's";
    case R_LL_SYMBOL: return "literal/length symbol 286 or 287";
    case R_D_SYMBOL: return "distance symbol 30 or 31";
    case R_DIST_BEFORE: return "a distance that reaches in front of the block's output";
    case R_DATA_ENDS: return "the deflate data ends early";
    case R_TOO_LONG: return "the output is longer than ISIZE";
    case R_TOO_SHORT: return "the output is shorter than ISIZE";
    case R_CRC: return "the CRC-32 differs from the trailer's";
    default: return "no reason";
  }
}

struct Walk {
  std::vector<Block> blocks;
  long long consumed = 0;   // the offset behind the last whole block
  long long total = 0;      // the sum of ISIZE
  long long bad_block = -1; // a malformed header: its block and reason (the walk stops in front of it)
  int bad_reason = 0;
};

// The blocks in[0, bytes) wholly holds.  A part at the end that is no whole block -- a header cut short, a block whose BSIZE runs past
// the chunk -- ends the walk and is not an error; a header that is whole and wrong is.
inline void bgzf_walk(const uint8_t* in, long long bytes, Walk* W) {
  W->blocks.clear();
  W->consumed = W->total = 0;
  W->bad_block = -1; W->bad_reason = 0;
  long long at = 0;
  auto u16 = [&](long long o) { return (uint32_t)in[o] | (uint32_t)in[o + 1] << 8; };
  auto u32 = [&](long long o) { return u16(o) | u16(o + 2) << 16; };
  auto bad = [&](int reason) { W->bad_block = (long long)W->blocks.size(); W->bad_reason = reason; };
  while (bytes - at >= 12) {
    const uint8_t* h = in + at;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return bad(R_MAGIC);
    if (!(h[3] & 4)) return bad(R_NO_BC);
    if (h[3] != 4) return bad(R_MAGIC);
    const long long xlen = u16(at + 10);
    if (bytes - at < 12 + xlen) break;
    long long x = at + 12, bsize = -1;
    const long long xend = x + xlen;
    bool broken = false;
    while (x < xend) {
      if (xend - x < 4) { broken = true; break; }
      const long long slen = u16(x + 2);
      if (xend - x < 4 + slen) { broken = true; break; }
      if (in[x] == 66 && in[x + 1] == 67) {
        if (slen != 2) { broken = true; break; }
        bsize = u16(x + 4);
      }
      x += 4 + slen;
    }
    if (broken) return bad(R_BSIZE);
    if (bsize < 0) return bad(R_NO_BC);
    const long long size = bsize + 1;
    if (size < 12 + xlen + 8) return bad(R_BSIZE);
    if (bytes - at < size) break;
    Block b;
    b.coff = (uint32_t)at;
    b.data_off = (uint32_t)(at + 12 + xlen);
    b.data_len = (uint32_t)(size - 12 - xlen - 8);
    b.crc = u32(at + size - 8);
    b.isize = u32(at + size - 4);
    b.out_off = (uint32_t)W->total;
    if (b.isize > (uint32_t)kMaxIsize) return bad(R_ISIZE);
    W->blocks.push_back(b);
    W->total += b.isize;
    at += size;
    W->consumed = at;
  }
}

struct SerialExec {  // the 64 lanes in a loop
  template <class F> void each(F&& f) const { for (int l = 0; l < kLanes; ++l) f(l); }
  void barrier() const {}
  bool lane0() const { return true; }
  template <class F> uint32_t fold_xor(F&& f) const {
    uint32_t v = 0;
    for (int l = 0; l < kLanes; ++l) v ^= f(l);
    return v;
  }
};

// The host twin.  The blocks of a walk from in[] into out[0, W.total): 0, or the reason of the lowest block that has one (*bad_block).
// Nothing of `in` outside a block's deflate data is read, nothing outside out[out_off, out_off + isize) written.
inline int inflate_serial(Work& w, const uint8_t* in, const Walk& W, uint8_t* out, long long* bad_block) {
  *bad_block = -1;
  for (size_t b = 0; b < W.blocks.size(); ++b) {
    const Block& B = W.blocks[b];
    const int r = inflate_member(w, SerialExec(), in + B.data_off, B.data_len, B.isize, B.crc);
    if (r) { *bad_block = (long long)b; return r; }
    if (B.isize) memcpy(out + B.out_off, w.win, B.isize);
  }
  return 0;
}

// A BGZF virtual offset for the inflated offset `u` of a walk's output: the first block whose inflated end lies above u, and u
// within it; behind every block: (the offset behind the last whole block, 0).
inline long long virtual_offset(const Walk& W, long long u) {
  for (const Block& B : W.blocks)
    if ((long long)B.out_off + B.isize > u) return (long long)B.coff << 16 | (u - B.out_off);
  return W.consumed << 16;
}

}  // namespace inflcore
}  // namespace bpsw
