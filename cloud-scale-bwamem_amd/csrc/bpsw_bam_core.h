// bpsw_bam_core.h -- the bytes of one BAM record, the CRC-32 of a BGZF block and the bytes around it, for the host and for the device.
//
// The record of line `i` is what the SAM line of the same batch says (bpsw_sam_core.h), in the layout of the SAM specification
// 4.2: both emitters start from the same resolution step (samcore::resolve_line -- the mate copy, the flag bits and their fold, the
// flavours, the hard clips, the SEQ / QUAL window, TLEN), and the SA:Z value is written by the text's own list writer.  As there,
// bam_rec_len counts and bam_rec_write stores through one emitter (emit_rec) over the counting and the checked storing sink, every
// store is checked against `end`, and ST_OVERRUN / ST_MISMATCH are reported through a status word.  Integers are stored a byte at
// a time (a record begins at any offset of the stream); the base codes are packed constants indexed by shifting.  No array of its
// own is indexed, so the kernels that compile this have no scratch; the CRC's table is the caller's (LDS on the device).
//
// Compiled by hipcc for bam_len_kernel / bam_write_kernel / bgzf_frame_kernel (bpsw_bam.hip) and by g++ for
// tests/bam_host/bam_host.cpp.
#pragma once

#include <stdint.h>

#include "bpsw_sam_core.h"

namespace bpsw {
namespace bamcore {

namespace sc = bpsw::samcore;
using sc::CountSink;
using sc::WriteSink;
using sc::SamBatch;
using sc::SamLine;
using sc::SamRead;
using sc::ST_OVERRUN;
using sc::ST_MISMATCH;

constexpr int kMaxName = 254;            // l_read_name is one byte and counts the NUL
constexpr int kBgzfMaxPayload = 65280;   // htslib's BGZF_BLOCK_SIZE: with the 31 bytes around it BSIZE still fits 16 bits
constexpr int kBgzfHead = 23;            // the 18-byte BGZF header, then 01 LEN ~LEN of the one stored deflate block
constexpr int kBgzfTail = 8;             // CRC32, ISIZE
constexpr int kBgzfAround = kBgzfHead + kBgzfTail;
constexpr int kBinUnplaced = 4680;       // reg2bin(-1, 0)

// ---- little-endian stores ---------------------------------------------------------------------------------------------------------
template <class S> BPSW_SAM_HD void put_u8(S& s, uint32_t v) { sc::put_char(s, (char)(uint8_t)v); }
template <class S> BPSW_SAM_HD void put_u16(S& s, uint32_t v) {
  char* d = s.take(2);
  if (d) { d[0] = (char)(uint8_t)v; d[1] = (char)(uint8_t)(v >> 8); }
}
BPSW_SAM_HD void store_u32(char* d, uint32_t v) {
  d[0] = (char)(uint8_t)v; d[1] = (char)(uint8_t)(v >> 8); d[2] = (char)(uint8_t)(v >> 16); d[3] = (char)(uint8_t)(v >> 24);
}
template <class S> BPSW_SAM_HD void put_u32(S& s, uint32_t v) {
  char* d = s.take(4);
  if (d) store_u32(d, v);
}

// reg2bin of the specification (5.3) for the 0-based half-open [beg, end)
BPSW_SAM_HD int reg2bin(long long beg, long long end) {
  --end;
  if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// an integer tag in the narrowest type, as htslib's text parser stores it: C S I for v >= 0, c s i below
template <class S> BPSW_SAM_HD void put_int_tag(S& s, char a, char b, long long v) {
  sc::put_char(s, a);
  sc::put_char(s, b);
  if (v >= 0) {
    if (v <= 0xff) { sc::put_char(s, 'C'); put_u8(s, (uint32_t)v); }
    else if (v <= 0xffff) { sc::put_char(s, 'S'); put_u16(s, (uint32_t)v); }
    else { sc::put_char(s, 'I'); put_u32(s, (uint32_t)v); }
  } else {
    if (v >= -128) { sc::put_char(s, 'c'); put_u8(s, (uint32_t)v); }
    else if (v >= -32768) { sc::put_char(s, 's'); put_u16(s, (uint32_t)v); }
    else { sc::put_char(s, 'i'); put_u32(s, (uint32_t)v); }
  }
}
template <class S> BPSW_SAM_HD void put_z_tag(S& s, char a, char b, const char* src, long long k) {
  sc::put_char(s, a);
  sc::put_char(s, b);
  sc::put_char(s, 'Z');
  if (k > 0) sc::put_bytes(s, src, k);
  sc::put_char(s, '\0');
}

BPSW_SAM_HD uint32_t nib_fwd(int c) { return (0xF8421u >> (4 * (c > 4 ? 4 : c))) & 0xf; }   // A C G T N = 1 2 4 8 15
BPSW_SAM_HD uint32_t nib_rev(int c) { return (0xF1248u >> (4 * (c > 4 ? 4 : c))) & 0xf; }   // their complements

template <class S> BPSW_SAM_HD void emit_rec(S& s, const SamBatch& B, int line) {
  const sc::Resolved v = sc::resolve_line(B, line);
  const SamLine& L = *v.L;
  const SamRead& R = *v.R;
  const bool placed = v.rid >= 0;
  const int n_cig = placed ? v.n_cigar : 0;
  const long long n_seq = v.hidden ? 0 : v.qe > v.qb ? v.qe - v.qb : 0;
  char* block_size = s.take(4);  // (filled in last: the record's length without these four bytes)
  // ---- the fixed part ----------------------------------------------------------------------------------------------------------------
  const long long pos = placed ? v.pos : -1;
  put_u32(s, (uint32_t)(placed ? v.rid : -1));
  put_u32(s, (uint32_t)pos);
  put_u8(s, (uint32_t)R.name_len + 1);
  put_u8(s, (uint32_t)(placed ? L.mapq : 0));
  int bin = kBinUnplaced;
  if (pos >= 0) {
    const int rl = sc::ref_len(v.cig, n_cig);
    bin = reg2bin(pos, pos + (rl > 0 ? rl : 1));
  }
  put_u16(s, (uint32_t)bin);
  put_u16(s, (uint32_t)n_cig);
  put_u16(s, (uint32_t)v.folded);
  put_u32(s, (uint32_t)n_seq);
  put_u32(s, (uint32_t)(v.has_next ? v.m_rid : -1));
  put_u32(s, (uint32_t)(v.has_next ? v.m_pos : -1));
  put_u32(s, (uint32_t)(v.has_next ? v.tlen : 0));
  // ---- name, CIGAR, SEQ, QUAL ------------------------------------------------------------------------------------------------------
  sc::put_bytes(s, B.names + R.name_at, R.name_len);
  sc::put_char(s, '\0');
  for (int i = 0; i < n_cig; ++i) {
    uint32_t op = v.cig[i] & 0xf;                  // MIDSH = 01234 here, MIDNSH = 012345 in a BAM
    if (op == 3 || op == 4) op = v.which ? 5 : 4;  // hard clipping on every line but the read's first
    put_u32(s, (v.cig[i] >> 4) << 4 | op);
  }
  if (n_seq > 0) {
    const long long half = (n_seq + 1) / 2;
    char* d = s.take(half + n_seq);
    if (d) {
      const uint8_t* seq = B.seq + R.seq_at;
      for (long long i = 0; i < n_seq; i += 2) {
        uint32_t hi, lo = 0;
        if (!v.is_rev) { hi = nib_fwd(seq[v.qb + i]); if (i + 1 < n_seq) lo = nib_fwd(seq[v.qb + i + 1]); }
        else { hi = nib_rev(seq[v.qe - 1 - i]); if (i + 1 < n_seq) lo = nib_rev(seq[v.qe - 2 - i]); }
        d[i >> 1] = (char)(uint8_t)(hi << 4 | lo);
      }
      d += half;
      if (!B.qual) {
        for (long long i = 0; i < n_seq; ++i) d[i] = (char)0xff;
      } else {
        const uint8_t* q = B.qual + R.seq_at;
        if (!v.is_rev) for (long long i = 0; i < n_seq; ++i) d[i] = (char)(uint8_t)(q[v.qb + i] - 33);
        else for (long long i = 0; i < n_seq; ++i) d[i] = (char)(uint8_t)(q[v.qe - 1 - i] - 33);
      }
    }
  }
  // ---- the tags, in the text's order and under its conditions --------------------------------------------------------------------------
  if (v.n_cigar > 0) {
    put_int_tag(s, 'N', 'M', L.NM);
    put_z_tag(s, 'M', 'D', B.md + L.md_at, L.md_len);
  }
  if (L.score >= 0) put_int_tag(s, 'A', 'S', L.score);
  if (L.sub >= 0) put_int_tag(s, 'X', 'S', L.sub);
  if (B.rg_len > 0) put_z_tag(s, 'R', 'G', B.rg, B.rg_len);
  if (!v.hidden && sc::has_sa(B, L, v.which)) {
    sc::put_bytes(s, "SAZ", 3);
    sc::put_sa_list(s, B, L, v.which);
    sc::put_char(s, '\0');
  }
  if (block_size) store_u32(block_size, (uint32_t)(s.n - 4));
}

// the number of bytes of the record of line `line`, block_size included
BPSW_SAM_HD long long bam_rec_len(const SamBatch& B, int line) {
  CountSink s;
  emit_rec(s, B, line);
  return s.n;
}

// Writes the record of line `line` at dst and never at or past `end`.  Returns its number of bytes (written or not); *status gets
// ST_OVERRUN when it did not fit [dst, end), and ST_MISMATCH when expected >= 0 and it has another number of bytes.
BPSW_SAM_HD long long bam_rec_write(char* dst, char* end, const SamBatch& B, int line, long long expected, int* status) {
  WriteSink s(dst, end);
  emit_rec(s, B, line);
  int st = 0;
  if (s.over) st |= ST_OVERRUN;
  if (expected >= 0 && s.n != expected) st |= ST_MISMATCH;
  *status = st;
  return s.n;
}

// ---- CRC-32 (the gzip polynomial, reflected: 0xEDB88320) ---------------------------------------------------------------------------
// entry i of the byte table; the caller keeps the 256 of them where it likes
BPSW_SAM_HD uint32_t crc32_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
  return i;
}
// zlib's crc32(crc, p, n): the CRC of A || p[0, n) from crc = the CRC of A (0 for none)
BPSW_SAM_HD uint32_t crc32_bytes(const uint32_t* tab, uint32_t crc, const uint8_t* p, long long n) {
  crc = ~crc;
  for (; n > 0 && ((uintptr_t)p & 3); ++p, --n) crc = tab[(crc ^ *p) & 0xff] ^ (crc >> 8);
  for (; n >= 4; p += 4, n -= 4) {
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    crc ^= w;  // (both sides are little-endian)
    crc = tab[crc & 0xff] ^ (crc >> 8);
    crc = tab[crc & 0xff] ^ (crc >> 8);
    crc = tab[crc & 0xff] ^ (crc >> 8);
    crc = tab[crc & 0xff] ^ (crc >> 8);
  }
  for (; n > 0; ++p, --n) crc = tab[(crc ^ *p) & 0xff] ^ (crc >> 8);
  return ~crc;
}
// a(x) b(x) mod P(x), bit 31 the coefficient of x^0
BPSW_SAM_HD uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m && a; m >>= 1) {
    if (a & m) { p ^= b; a &= ~m; }
    b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// crc(x) x^(8 n) mod P: what the CRC of a slice contributes to the CRC of a whole in which n more bytes follow the slice.  For
// adjacent slices A, B: crc(A || B) == crc32_shift(crc(A), |B|) ^ crc(B) (zlib's crc32_combine; the conditioning cancels).  Over
// many slices every CRC is shifted by the bytes behind its slice and the results are XORed, in any order.  x^(8 n) by squaring:
// a multiplication of 32 shift-xor steps per bit of n, no table.
BPSW_SAM_HD uint32_t crc32_shift(uint32_t crc, long long n) {
  if (crc == 0) return 0;
  uint32_t sq = 0x00800000u;  // x^8
  for (; n > 0; n >>= 1) {
    if (n & 1) crc = gf2_mulmod(sq, crc);
    sq = gf2_mulmod(sq, sq);
  }
  return crc;
}
BPSW_SAM_HD uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, long long len_b) { return crc32_shift(crc_a, len_b) ^ crc_b; }

// ---- the bytes around the payload of a BGZF block: a gzip member with one stored deflate block -----------------------------------------
// byte k (0 .. kBgzfHead - 1) in front of a payload of n bytes (1 <= n <= kBgzfMaxPayload)
BPSW_SAM_HD uint8_t bgzf_head_byte(int k, uint32_t n) {
  if (k < 8) return (uint8_t)(0x0000000004088b1fULL >> (8 * k));          // 1f 8b 08 04, MTIME 0
  if (k < 16) return (uint8_t)(0x000243420006ff00ULL >> (8 * (k - 8)));   // XFL 0, OS ff, XLEN 6, 'B' 'C', SLEN 2
  const uint32_t bsize = n + kBgzfAround - 1;
  if (k < 18) return (uint8_t)(bsize >> (8 * (k - 16)));
  if (k == 18) return 1;                                                  // BFINAL, stored
  if (k < 21) return (uint8_t)(n >> (8 * (k - 19)));
  return (uint8_t)(~n >> (8 * (k - 21)));
}
// byte k (0 .. kBgzfTail - 1) behind it
BPSW_SAM_HD uint8_t bgzf_tail_byte(int k, uint32_t crc, uint32_t n) { return (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3))); }

// ---- the same around a compressed block (bpsw_deflate_core.h): the 18 bytes of the BGZF header in front of `dbytes` deflate bytes ----------
// (what follows them is bgzf_tail_byte's: the CRC and the size are the payload's, however it is coded)
constexpr int kBgzfDeflateHead = 18;
BPSW_SAM_HD uint8_t bgzf_deflate_head_byte(int k, uint32_t dbytes) {
  if (k < 8) return (uint8_t)(0x0000000004088b1fULL >> (8 * k));
  if (k < 16) return (uint8_t)(0x000243420006ff00ULL >> (8 * (k - 8)));
  return (uint8_t)((kBgzfDeflateHead + dbytes + kBgzfTail - 1) >> (8 * (k - 16)));
}

}  // namespace bamcore
}  // namespace bpsw
