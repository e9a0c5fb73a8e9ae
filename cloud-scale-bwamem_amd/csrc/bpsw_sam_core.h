// bpsw_sam_core.h -- the bytes of one SAM line, with or without a mate, for the host and for the device.
//
// memAlnToSAM (worker2/MemRegToADAMSAM.scala:328-560 == mem_aln2sam, native/bwamem.c:726-838), as aln_to_sam (bpsw_tail.cpp)
// writes it on the calling thread; that function stays the yardstick.  A line names its mate by one index (SamLine::mate): the
// FIRST line of the other read of its pair, which is what the paired tail hands memAlnToSAM as `m` in the five fields the line
// reads of it (rid, pos, is_rev, n_cigar and the CIGAR words); 0 is a line without a mate (m == NULL).  Here the same line is a function of a
// LINE RECORD (SamLine) and the batch's tables (SamBatch), so that a kernel can write it: sam_line_len counts the bytes,
// sam_line_write stores them, both through one emitter (emit_line) over a sink that either counts or stores, so the two cannot
// drift apart.  What the line says -- the mate copy, the flag bits and their fold, the clips, TLEN -- is resolved once
// (resolve_line), for this emitter and for the BAM record's (bpsw_bam_core.h).  Every store is checked against `end`; a line that would pass it, or whose byte count differs from what the caller
// expected, is reported through a status word and nothing is written past `end`.
//
// Numbers are formatted by counting their digits first and storing straight into the destination; the letter tables are packed
// constants indexed by shifting.  No array of its own is indexed, so the kernels that compile this have no scratch.
//
// Compiled by hipcc for sam_len_kernel / sam_write_kernel (bpsw_sam_se.hip) and by g++ for tests/sam_host/sam_host.cpp and
// tests/sam_pe_host/sam_pe_host.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BPSW_SAM_HD __host__ __device__ inline
#else
#define BPSW_SAM_HD inline
#endif

namespace bpsw {
namespace samcore {

constexpr int FLAVOUR_SCALA = 0, FLAVOUR_C = 1;  // == BPSW_TAIL_SCALA / BPSW_TAIL_C
constexpr int ST_OVERRUN = 1;   // a store would have passed `end` (nothing was written there)
constexpr int ST_MISMATCH = 2;  // the line has another number of bytes than the caller expected

struct SamLine {  // one line: the mem_aln_t of memRegToAln after memRegToSAMSe's bookkeeping (flag unfolded, no 0x4 / 0x10 yet)
  long long pos;       // 0-based
  long long cig_at;    // its CIGAR words in SamBatch::cig (n_cigar of them: len << 4 | op, op MIDSH = 01234)
  long long md_at;     // its MD bytes in SamBatch::md (md_len of them)
  int32_t read;        // the read it belongs to (SamBatch::reads)
  int32_t first;       // the first line of that read in SamBatch::lines ...
  int32_t n_list;      // ... and how many it has (the SA:Z list runs over them)
  int32_t rid, flag, is_rev, mapq, NM, n_cigar, md_len, score, sub;
  int32_t mate;        // the first line of the other read of its pair in SamBatch::lines, + 1; 0: no mate
};
static_assert(sizeof(SamLine) == 80, "the line record is staged as it is");

struct SamRead {
  long long seq_at;   // bases in SamBatch::seq (codes 0..4), qualities at the same place in SamBatch::qual
  long long name_at;  // in SamBatch::names
  int32_t len, name_len;
};
static_assert(sizeof(SamRead) == 24, "the read record is staged as it is");

struct SamBatch {
  const SamLine* lines;
  const SamRead* reads;
  const uint32_t* cig;
  const char* md;
  const uint8_t* seq;
  const uint8_t* qual;     // null: '*'
  const char* names;
  const int32_t* ctg_at;   // n_ctg + 1 offsets into ctg_names; an empty name (or rid >= n_ctg) prints as ctg<rid + 1>
  const char* ctg_names;
  const char* rg;          // rg_len bytes; 0: no RG:Z tag
  int32_t n_ctg, rg_len, flavour;
};

// ---- sinks ---------------------------------------------------------------------------------------------------------------
struct CountSink {
  long long n = 0;
  BPSW_SAM_HD char* take(long long k) { n += k; return nullptr; }
};
struct WriteSink {
  char* p;
  char* end;
  long long n = 0;
  int over = 0;
  BPSW_SAM_HD WriteSink(char* dst, char* e) : p(dst), end(e) {}
  BPSW_SAM_HD char* take(long long k) {  // k more bytes for the caller to store, or null when they would pass `end` (they still count)
    n += k;
    if (over || end - p < k) { over = 1; return nullptr; }
    char* d = p;
    p += k;
    return d;
  }
};

BPSW_SAM_HD char op_letter(int c) { return (char)((0x485344494DULL >> (8 * (c > 4 ? 4 : c))) & 0xff); }       // "MIDSH"
BPSW_SAM_HD char base_fwd(int c) { return (char)((0x4E54474341ULL >> (8 * (c > 4 ? 4 : c))) & 0xff); }       // "ACGTN"
BPSW_SAM_HD char base_rev(int c) { return (char)((0x4E41434754ULL >> (8 * (c > 4 ? 4 : c))) & 0xff); }       // "TGCAN"

template <class S> BPSW_SAM_HD void put_char(S& s, char c) {
  char* d = s.take(1);
  if (d) *d = c;
}
template <class S> BPSW_SAM_HD void put_bytes(S& s, const char* src, long long k) {
  char* d = s.take(k);
  if (d) for (long long i = 0; i < k; ++i) d[i] = src[i];
}
template <class S> BPSW_SAM_HD void put_num(S& s, long long v) {
  const bool neg = v < 0;
  unsigned long long x = neg ? 0ULL - (unsigned long long)v : (unsigned long long)v;
  int digits = 1;
  for (unsigned long long y = x; y >= 10; y /= 10) ++digits;
  char* d = s.take(digits + (neg ? 1 : 0));
  if (!d) return;
  if (neg) *d++ = '-';
  for (int i = digits - 1; i >= 0; --i) { d[i] = (char)('0' + (int)(x % 10)); x /= 10; }
}
template <class S> BPSW_SAM_HD void put_contig(S& s, const SamBatch& B, int rid) {
  if (rid >= 0 && rid < B.n_ctg && B.ctg_at[rid + 1] > B.ctg_at[rid]) {
    put_bytes(s, B.ctg_names + B.ctg_at[rid], B.ctg_at[rid + 1] - B.ctg_at[rid]);
  } else {
    put_bytes(s, "ctg", 3);
    put_num(s, (long long)rid + 1);
  }
}

BPSW_SAM_HD bool is_clip(uint32_t w) { return (w & 0xf) == 3 || (w & 0xf) == 4; }
BPSW_SAM_HD int ref_len(const uint32_t* cig, int n) {  // getRlen: the bases of the reference under M and D
  int l = 0;
  for (int k = 0; k < n; ++k) { const int op = (int)(cig[k] & 0xf); if (op == 0 || op == 2) l += (int)(cig[k] >> 4); }
  return l;
}

// What a line says once memAlnToSAM's rules are applied: the one resolution step under both emitters, the text here and the binary
// record of bpsw_bam_core.h.  Scalars and pointers into the batch only.
struct Resolved {
  const SamLine* L;
  const SamRead* R;
  const uint32_t* cig;   // the line's CIGAR words (n_cigar of them count; a clip prints as H when `which` > 0, else as S)
  int which;             // its place in its read's list
  int rid, is_rev, n_cigar;   // after the mate copy: rid < 0 prints "*\t0\t0\t*"; n_cigar == 0 prints '*' and drops NM / MD
  long long pos;
  int folded;            // the flag as it is printed: 0x10000 folded into 0x100
  bool hidden;           // SEQ and QUAL are '*' and there is no SA list (0x100 as the flavour sees it)
  bool has_next;         // the mate columns are filled: m_rid, m_pos, tlen; else "*\t0\t0"
  int m_rid;
  long long m_pos, tlen;
  int qb, qe;            // SEQ / QUAL are the read's bases [qb, qe), read backwards and complemented when is_rev (qe <= qb: none)
};

BPSW_SAM_HD Resolved resolve_line(const SamBatch& B, int line) {
  Resolved v;
  const SamLine& L = B.lines[line];
  v.L = &L;
  v.R = &B.reads[L.read];
  v.which = line - L.first;
  const uint32_t* cig = B.cig + L.cig_at;
  v.cig = cig;
  int flag = L.flag;
  // the line's and the mate's place; an unmapped one of the two is put where the other is
  int rid = L.rid, is_rev = L.is_rev, n_cigar = L.n_cigar;
  long long pos = L.pos;
  const bool has_m = L.mate > 0;
  int m_rid = -1, m_is_rev = 0, m_n_cigar = 0;
  long long m_pos = -1;
  const uint32_t* m_cig = B.cig;
  if (has_m) {
    const SamLine& M = B.lines[L.mate - 1];
    m_rid = M.rid; m_is_rev = M.is_rev; m_n_cigar = M.n_cigar; m_pos = M.pos;
    m_cig = B.cig + M.cig_at;
    flag |= 0x1;
  }
  if (rid < 0) flag |= 0x4;
  if (has_m && m_rid < 0) flag |= 0x8;
  if (rid < 0 && has_m && m_rid >= 0) { rid = m_rid; pos = m_pos; is_rev = m_is_rev; n_cigar = 0; }
  if (has_m && m_rid < 0 && rid >= 0) { m_rid = rid; m_pos = pos; m_is_rev = is_rev; m_n_cigar = 0; }
  if (is_rev) flag |= 0x10;
  if (has_m && m_is_rev) flag |= 0x20;
  v.folded = (flag & 0xffff) | ((flag & 0x10000) ? 0x100 : 0);
  if (B.flavour == FLAVOUR_SCALA) flag = v.folded;  // the Scala assigns the folded flag, the C only prints it
  v.hidden = (flag & 0x100) != 0;
  v.rid = rid; v.is_rev = is_rev; v.n_cigar = n_cigar; v.pos = pos;
  v.has_next = has_m && m_rid >= 0;
  v.m_rid = m_rid; v.m_pos = m_pos;
  v.tlen = 0;
  if (v.has_next && rid == m_rid && m_n_cigar > 0 && n_cigar > 0) {  // the distance between the two 5' ends
    const long long p0 = pos + (is_rev ? ref_len(cig, n_cigar) - 1 : 0);
    const long long p1 = m_pos + (m_is_rev ? ref_len(m_cig, m_n_cigar) - 1 : 0);
    v.tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
  }
  int qb = 0, qe = v.R->len;
  const int nc = n_cigar;
  const bool clip_first = nc > 0 && is_clip(cig[0]), clip_last = nc > 0 && is_clip(cig[nc - 1]);
  if (!is_rev) {
    if (v.which && clip_first) qb += (int)(cig[0] >> 4);
    if (v.which && clip_last) qe -= (int)(cig[nc - 1] >> 4);
  } else {
    if (v.which && clip_first) qe -= (int)(cig[0] >> 4);
    if (v.which && clip_last) qb += (int)(cig[nc - 1] >> 4);
  }
  v.qb = qb; v.qe = qe;
  return v;
}

// the SA list of a line: its read's other lines that are not 0x100
BPSW_SAM_HD bool has_sa(const SamBatch& B, const SamLine& L, int which) {
  for (int i = 0; i < L.n_list; ++i)
    if (i != which && !(B.lines[L.first + i].flag & 0x100)) return true;
  return false;
}
template <class S> BPSW_SAM_HD void put_sa_list(S& s, const SamBatch& B, const SamLine& L, int which) {
  for (int i = 0; i < L.n_list; ++i) {
    const SamLine& r = B.lines[L.first + i];
    if (i == which || (r.flag & 0x100)) continue;
    put_contig(s, B, r.rid);
    put_char(s, ',');
    put_num(s, r.pos + 1);
    put_char(s, ',');
    put_char(s, r.is_rev ? '-' : '+');
    put_char(s, ',');
    const uint32_t* rc = B.cig + r.cig_at;
    for (int k = 0; k < r.n_cigar; ++k) { put_num(s, (long long)(rc[k] >> 4)); put_char(s, op_letter((int)(rc[k] & 0xf))); }
    put_char(s, ',');
    put_num(s, r.mapq);
    put_char(s, ',');
    put_num(s, r.NM);
    put_char(s, ';');
  }
}

template <class S> BPSW_SAM_HD void emit_line(S& s, const SamBatch& B, int line) {
  const Resolved v = resolve_line(B, line);
  const SamLine& L = *v.L;
  const SamRead& R = *v.R;
  put_bytes(s, B.names + R.name_at, R.name_len);
  put_char(s, '\t');
  put_num(s, v.folded);
  put_char(s, '\t');
  if (v.rid >= 0) {
    put_contig(s, B, v.rid);
    put_char(s, '\t');
    put_num(s, v.pos + 1);
    put_char(s, '\t');
    put_num(s, L.mapq);
    put_char(s, '\t');
    if (v.n_cigar > 0) {
      for (int i = 0; i < v.n_cigar; ++i) {
        int c = (int)(v.cig[i] & 0xf);
        if (c == 3 || c == 4) c = v.which ? 4 : 3;  // hard clipping on every line but the read's first
        put_num(s, (long long)(v.cig[i] >> 4));
        put_char(s, op_letter(c));
      }
    } else {
      put_char(s, '*');
    }
  } else {
    put_bytes(s, "*\t0\t0\t*", 7);
  }
  put_char(s, '\t');
  if (v.has_next) {
    if (v.rid == v.m_rid) put_char(s, '='); else put_contig(s, B, v.m_rid);
    put_char(s, '\t');
    put_num(s, v.m_pos + 1);
    put_char(s, '\t');
    put_num(s, v.tlen);
  } else {
    put_bytes(s, "*\t0\t0", 5);
  }
  put_char(s, '\t');
  if (v.hidden) {
    put_bytes(s, "*\t*", 3);
  } else {
    const int qb = v.qb, qe = v.qe;
    const uint8_t* seq = B.seq + R.seq_at;
    const long long n = qe > qb ? qe - qb : 0;
    char* d = s.take(n + 1 + (B.qual ? n : 1));  // bases, tab, qualities
    if (d) {
      if (!v.is_rev) for (long long i = 0; i < n; ++i) d[i] = base_fwd(seq[qb + i]);
      else for (long long i = 0; i < n; ++i) d[i] = base_rev(seq[qe - 1 - i]);
      d[n] = '\t';
      if (!B.qual) {
        d[n + 1] = '*';
      } else {
        const uint8_t* q = B.qual + R.seq_at;
        if (!v.is_rev) for (long long i = 0; i < n; ++i) d[n + 1 + i] = (char)q[qb + i];
        else for (long long i = 0; i < n; ++i) d[n + 1 + i] = (char)q[qe - 1 - i];
      }
    }
  }
  if (v.n_cigar > 0) {
    put_bytes(s, "\tNM:i:", 6);
    put_num(s, L.NM);
    put_bytes(s, "\tMD:Z:", 6);
    if (L.md_len > 0) put_bytes(s, B.md + L.md_at, L.md_len);
  }
  if (L.score >= 0) { put_bytes(s, "\tAS:i:", 6); put_num(s, L.score); }
  if (L.sub >= 0) { put_bytes(s, "\tXS:i:", 6); put_num(s, L.sub); }
  if (B.rg_len > 0) { put_bytes(s, "\tRG:Z:", 6); put_bytes(s, B.rg, B.rg_len); }
  if (!v.hidden && has_sa(B, L, v.which)) {
    put_bytes(s, "\tSA:Z:", 6);
    put_sa_list(s, B, L, v.which);
  }
  put_char(s, '\n');
}

// the number of bytes of line `line`
BPSW_SAM_HD long long sam_line_len(const SamBatch& B, int line) {
  CountSink s;
  emit_line(s, B, line);
  return s.n;
}

// Writes line `line` at dst and never at or past `end`.  Returns the line's number of bytes (written or not); *status gets
// ST_OVERRUN when the line did not fit [dst, end), and ST_MISMATCH when expected >= 0 and the line has another number of bytes.
BPSW_SAM_HD long long sam_line_write(char* dst, char* end, const SamBatch& B, int line, long long expected, int* status) {
  WriteSink s(dst, end);
  emit_line(s, B, line);
  int st = 0;
  if (s.over) st |= ST_OVERRUN;
  if (expected >= 0 && s.n != expected) st |= ST_MISMATCH;
  *status = st;
  return s.n;
}

}  // namespace samcore
}  // namespace bpsw
