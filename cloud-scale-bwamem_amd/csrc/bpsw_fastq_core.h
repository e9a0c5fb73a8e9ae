// bpsw_fastq_core.h -- the rules of one four-line FASTQ record, for the host and for the device, and the serial parse built on them.
//
// The accepted form is the one the reference's loader reads (fastq/FASTQLocalFileLoader.scala:79-126): header, sequence, a line
// that is ignored, qualities.  What a field IS follows the reference's C (kseq_read, native/kseq.h:175-215, and bseq_read with
// trim_readno, native/bwa.c:25-62), which the SAM text of this library is held against:
//   lines   a line ends at '\n'; one '\r' directly in front of it is not part of the line when the line has more than one byte
//           (kseq.h:140, its l > 1 included: a line that is a lone '\r' keeps it).  Position alone decides what a line is: line 4r is
//           the header and begins with '@', line 4r + 2 begins with '+' and the rest of it is ignored, line 4r + 3 is as long as
//           line 4r + 1, which is not empty.  A '@' or '+' at the start of a quality line means nothing.
//   name    the bytes after '@' up to the first byte for which C's isspace holds; the comment behind it is dropped.  Then
//           trim_readno: a name of more than 2 bytes whose second-to-last byte is '/' and whose last byte is a decimal digit loses
//           both.  This is the C rule.  The Scala loader trims only "/1" and "/2" and fails on names shorter than two bytes; there
//           is no switch for it.  An empty name is refused.
//   bases   nst_nt4_table (native/bntseq.c:44-61) without the table: Aa Cc Gg Tt are 0..3, everything else is 4.  Two inputs are
//           refused instead of translated: '-', which the table maps to 5, outside the pools' 0..4; and bytes below 4, which
//           mem_align1_core (native/bwamem.c:914) would pass through as codes.  (That line compares a plain char, so on the
//           reference's platform bytes of 0x80 and above pass through as well; here they are 4 like every other letter.)
//   quals   copied as they are.
// A record that breaks a rule has a reason code, checked in the order of the codes; a parse reports the LOWEST read index with a
// reason, which is what makes a parse by many lanes and a serial one agree.
//
// __host__ __device__: fastq_record_kernel and fastq_emit_kernel (bpsw_fastq.hip) call fq_record, fq_same_name and fq_base_code;
// parse_serial below -- BPSW_FASTQ_HOST, and the yardstick of tests/fastq_host/fastq_host.cpp under g++ -- calls the same functions.
// Nothing here indexes an array of its own, so the kernels that compile it have no scratch.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BPSW_FQ_HD __host__ __device__ inline
#else
#define BPSW_FQ_HD inline
#endif

namespace bpsw {
namespace fqcore {

constexpr int FINAL = 1, INTERLEAVED = 2, PAIR_NAMES = 4, HOST = 8;  // == BPSW_FASTQ_*
constexpr int R_NO_AT = 1, R_NO_PLUS = 2, R_EMPTY_READ = 3, R_LEN_DIFF = 4, R_EMPTY_NAME = 5, R_DASH = 6, R_LOW_BYTE = 7, R_PAIR_NAME = 8,
              R_TRUNCATED = 9, R_TABLE = 10;
constexpr long long kMinRecordBytes = 8;  // "@x\nA\n+\nI": no well-formed record is shorter

// a text below 2^31 bytes: every position, and bytes + 1, fits
typedef uint32_t pos_t;

struct Record {
  pos_t name_beg, seq_beg, qual_beg;
  int32_t name_len, seq_len;
};

BPSW_FQ_HD bool fq_is_space(unsigned char b) { return b == ' ' || (b >= 9 && b <= 13); }
BPSW_FQ_HD int fq_base_code(unsigned char b) {
  const unsigned char u = b & 0xdf;  // (only 'A' and 'a' give 'A', and so on)
  return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}
// the end of the line [beg, next - 1) whose '\n' is at next - 1
BPSW_FQ_HD pos_t fq_line_end(const char* t, pos_t beg, pos_t next) {
  pos_t e = next - 1;
  if (e - beg > 1 && t[e - 1] == '\r') --e;
  return e;
}

// Record r of a text: ls[0 .. 4] are the starts of its four lines and of the line behind them (ls[k + 1] - 1 is where line k's
// '\n' is, or would be for a last line without one).  0, or the first rule broken.
BPSW_FQ_HD int fq_record(const char* t, const pos_t* ls, long long bytes, Record* R) {
  const pos_t l0 = ls[0], l1 = ls[1], l2 = ls[2], l3 = ls[3], l4 = ls[4];
  R->name_beg = R->seq_beg = R->qual_beg = 0;
  R->name_len = R->seq_len = 0;
  if (!(l0 < l1 && l1 < l2 && l2 < l3 && l3 < l4 && (long long)l4 <= bytes + 1)) return R_TABLE;
  if (l1 - 1 == l0 || t[l0] != '@') return R_NO_AT;
  if (l3 - 1 == l2 || t[l2] != '+') return R_NO_PLUS;
  const pos_t e1 = fq_line_end(t, l1, l2), e3 = fq_line_end(t, l3, l4);
  if (e1 == l1) return R_EMPTY_READ;
  if (e3 - l3 != e1 - l1) return R_LEN_DIFF;
  pos_t q = l0 + 1;
  while (q < l1 - 1 && !fq_is_space((unsigned char)t[q])) ++q;
  int32_t nl = (int32_t)(q - (l0 + 1));
  if (nl > 2 && t[q - 2] == '/' && t[q - 1] >= '0' && t[q - 1] <= '9') nl -= 2;
  if (nl == 0) return R_EMPTY_NAME;
  bool dash = false, low = false;
  for (pos_t p = l1; p < e1; ++p) {
    const unsigned char b = (unsigned char)t[p];
    dash |= b == '-';
    low |= b < 4;
  }
  if (dash) return R_DASH;
  if (low) return R_LOW_BYTE;
  R->name_beg = l0 + 1; R->name_len = nl;
  R->seq_beg = l1; R->seq_len = (int32_t)(e1 - l1);
  R->qual_beg = l3;
  return 0;
}

BPSW_FQ_HD bool fq_same_name(const char* ta, const Record& a, const char* tb, const Record& b) {
  if (a.name_len != b.name_len) return false;
  for (int32_t k = 0; k < a.name_len; ++k)
    if (ta[a.name_beg + k] != tb[b.name_beg + k]) return false;
  return true;
}

// How many records of a text with `lines` lines a parse looks at.  Records are whole groups of four lines; as no well-formed record
// has fewer than kMinRecordBytes bytes, a text with more records than bytes / kMinRecordBytes + 1 has a malformed one among the
// first that many, and looking further cannot change the lowest bad index: the line table never needs more room than that.
BPSW_FQ_HD long long fq_records_to_parse(long long lines, long long bytes) {
  const long long r = lines / 4, most = bytes / kMinRecordBytes + 1;
  return r < most ? r : most;
}

// What the line counts decide: how read i maps to (text, record), how many reads there are, and, under FINAL, the read index at which
// a trailing part that is no whole record would stand (-1: none).
struct Shape {
  int two, pair_names;
  long long n_reads, used[2], trunc_read;
};
BPSW_FQ_HD Shape fq_shape(int n_texts, int flags, const long long lines[2], const long long bytes[2]) {
  Shape S;
  S.two = n_texts == 2;
  S.pair_names = S.two || (flags & PAIR_NAMES) != 0;
  const long long r0 = fq_records_to_parse(lines[0], bytes[0]), r1 = S.two ? fq_records_to_parse(lines[1], bytes[1]) : 0;
  if (S.two) {
    const long long k = r0 < r1 ? r0 : r1;
    S.used[0] = S.used[1] = k; S.n_reads = 2 * k;
  } else {
    S.n_reads = (flags & INTERLEAVED) ? (r0 & ~1ll) : r0;
    S.used[0] = S.n_reads; S.used[1] = 0;
  }
  S.trunc_read = -1;
  if (flags & FINAL) {
    for (int t = 0; t < n_texts; ++t) {
      if (lines[t] % 4 == 0) continue;
      const long long rec = lines[t] / 4, at = S.two ? 2 * rec + t : rec;
      if (S.trunc_read < 0 || at < S.trunc_read) S.trunc_read = at;
    }
  }
  return S;
}
BPSW_FQ_HD int fq_text_of(const Shape& S, long long i) { return S.two ? (int)(i & 1) : 0; }
BPSW_FQ_HD long long fq_record_of(const Shape& S, long long i) { return S.two ? i >> 1 : i; }

// Read i of a parse: its record by the rules, and for the second end of a pair with one name the comparison with the first end's
// (a first end that is malformed itself is reported under its own, lower index).  lt[t]: text t's line starts.
// entry t of a pair of values, by selection (a kernel's arguments are not indexed by a lane's value)
template <class V> BPSW_FQ_HD V fq_pick(const V a[2], int t) { return t ? a[1] : a[0]; }

BPSW_FQ_HD int fq_read(const Shape& S, const char* const text[2], const pos_t* const lt[2], const long long bytes[2], long long i, Record* R) {
  // (one loop, so that a kernel holds one copy of fq_record: the first end's record, when it is needed, then the read's own)
  const bool second = S.pair_names && (i & 1);
  Record F;
  int reason = 0, first_reason = 0;
  for (long long j = second ? i - 1 : i; j <= i; ++j) {
    const int t = fq_text_of(S, j);
    const int r = fq_record(fq_pick(text, t), fq_pick(lt, t) + 4 * fq_record_of(S, j), fq_pick(bytes, t), R);
    if (j < i) { F = *R; first_reason = r; }
    else reason = r;
  }
  if (reason || !second || first_reason) return reason;
  if (fq_same_name(fq_pick(text, fq_text_of(S, i - 1)), F, fq_pick(text, fq_text_of(S, i)), *R)) return 0;
  R->name_len = R->seq_len = 0;
  return R_PAIR_NAME;
}

}  // namespace fqcore
}  // namespace bpsw

// ---- the serial parse (host functions) ------------------------------------------------------------------------------------------
#include <vector>

namespace bpsw {
namespace fqcore {

inline const char* fq_reason_text(int reason) {
  switch (reason) {
    case R_NO_AT: return "the header line does not begin with '@' (not four-line FASTQ)";
    case R_NO_PLUS: return "the third line does not begin with '+' (not four-line FASTQ)";
    case R_EMPTY_READ: return "the read is empty";
    case R_LEN_DIFF: return "the quality line is not as long as the read";
    case R_EMPTY_NAME: return "the name is empty";
    case R_DASH: return "'-' in the read";
    case R_LOW_BYTE: return "a byte below 4 in the read";
    case R_PAIR_NAME: return "the name differs from the first end's";
    case R_TRUNCATED: return "the text ends inside the record (not four-line FASTQ)";
    default: return "the line table is inconsistent";
  }
}

struct Outputs {
  int32_t* read_len;
  int64_t* read_off;
  uint8_t* read_pool;
  uint8_t* qual_pool;
  int64_t* name_off;
  char* name_pool;
};
struct Result {
  long long n_reads, consumed[2], needed[3];
  long long bad_read;  // -1: none
  int bad_reason;
};
enum { PARSE_OK = 0, PARSE_BAD = 1, PARSE_CAPACITY = 2 };

// the number of lines of a text as a parse counts them, and whether the last one has no '\n'
inline long long fq_count_lines(const char* t, long long bytes, int flags, bool* open_line) {
  long long n = 0;
  for (long long p = 0; p < bytes; ++p) n += t[p] == '\n';
  *open_line = (flags & FINAL) && bytes > 0 && t[bytes - 1] != '\n';
  return n + *open_line;
}

// The whole parse on the calling thread.  `room` is asked once, when the sizes are known (needed[] filled): it returns the outputs, or
// false when they do not fit.  Nothing is written before that.
template <class Room>
int parse_serial(const char* const text[2], const long long bytes[2], int n_texts, int flags, Room&& room, Result* res) {
  std::vector<pos_t> table[2];
  long long lines[2] = {0, 0};
  for (int t = 0; t < n_texts; ++t) {
    bool open_line = false;
    lines[t] = fq_count_lines(text[t], bytes[t], flags, &open_line);
    const long long keep = 4 * fq_records_to_parse(lines[t], bytes[t]) + 1;
    table[t].assign((size_t)keep, 0);
    long long L = 0;
    for (long long p = 0; p < bytes[t] && L + 1 < keep; ++p)
      if (text[t][p] == '\n') table[t][(size_t)++L] = (pos_t)(p + 1);
    if (open_line && L + 1 < keep && L + 1 == lines[t]) table[t][(size_t)++L] = (pos_t)(bytes[t] + 1);
  }
  const Shape S = fq_shape(n_texts, flags, lines, bytes);
  const pos_t* lt[2] = {table[0].data(), table[1].data()};
  const long long n = S.n_reads;
  res->n_reads = n;
  res->bad_read = -1; res->bad_reason = 0;
  for (int t = 0; t < 2; ++t) {
    const long long at = t < n_texts ? (long long)table[t][(size_t)(4 * S.used[t])] : 0;
    res->consumed[t] = t < n_texts && at > bytes[t] ? bytes[t] : at;
  }
  std::vector<Record> recs((size_t)n);
  long long bases = 0, names = 0;
  for (long long i = 0; i < n; ++i) {
    const int reason = fq_read(S, text, lt, bytes, i, &recs[(size_t)i]);
    if (reason) { res->bad_read = i; res->bad_reason = reason; break; }
    bases += recs[(size_t)i].seq_len;
    if (!S.pair_names || !(i & 1)) names += recs[(size_t)i].name_len;
  }
  if (res->bad_read < 0 && S.trunc_read >= 0) { res->bad_read = S.trunc_read; res->bad_reason = R_TRUNCATED; }
  res->needed[0] = n; res->needed[1] = bases; res->needed[2] = names;
  if (res->bad_read >= 0) return PARSE_BAD;
  Outputs o;
  if (!room(*res, &o)) return PARSE_CAPACITY;
  long long at = 0, name_at = 0, k = 0;
  for (long long i = 0; i < n; ++i) {
    const Record& r = recs[(size_t)i];
    const char* t = text[fq_text_of(S, i)];
    o.read_len[i] = r.seq_len;
    o.read_off[i] = at;
    for (int32_t j = 0; j < r.seq_len; ++j) {
      o.read_pool[at + j] = (uint8_t)fq_base_code((unsigned char)t[r.seq_beg + j]);
      o.qual_pool[at + j] = (uint8_t)t[r.qual_beg + j];
    }
    at += r.seq_len;
    if (S.pair_names && (i & 1)) continue;
    o.name_off[k++] = name_at;
    for (int32_t j = 0; j < r.name_len; ++j) o.name_pool[name_at + j] = t[r.name_beg + j];
    name_at += r.name_len;
  }
  o.name_off[k] = name_at;
  return PARSE_OK;
}

}  // namespace fqcore
}  // namespace bpsw
