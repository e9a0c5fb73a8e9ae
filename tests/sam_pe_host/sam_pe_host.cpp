// sam_pe_host.cpp -- csrc/bpsw_sam_core.h with a mate (what sam_len_kernel / sam_write_kernel compile for the paired tail) on the
// host, against an independent writer of the same line made of std::string and snprintf, written from the reference's
// mem_aln2sam with m != NULL (native/bwamem.c:726-838).
//
// A program of its own (tests/test_sam_pe_core_host.py builds it with -fsanitize=address,undefined): seeded random batches of
// PAIRS of reads whose line lists run from 1 to 100 -- mapped and unmapped lines beside mapped and unmapped mates, both strands,
// the same contig, another one and a rid past the table, an empty CIGAR on either side, clips, 0x100 / 0x800 / 0x10000,
// positions past 2^32, both flavours, qualities present and absent.  Per line: sam_line_len == the bytes sam_line_write wrote ==
// the independent writer's, the bytes are equal, the line is written into a heap block of exactly its length (an overrun is a
// sanitizer report), and a too-small `end` is refused with the status and nothing is written past it.
//
// HOW A LINE FINDS ITS MATE.  The core reads the mate from the line table: SamLine::mate names the FIRST line of the pair's other
// read.  The paired tail (pe_lines, bpsw_tail.cpp) hands memAlnToSAM a record of its own instead, h[1 - i]: the region the pair
// was placed with, or region 0, or the unmapped record.  The lists here are built the same way -- a generated h[2] per pair, each
// read's list starting with the line of h[i] plus the bookkeeping the tail adds (flag bits, capped mapQ, sub cleared) that a mate
// is never asked for -- the independent writer prints against h[1 - i], the core against the index, and the program asserts that
// the five fields read of a mate (rid, pos, is_rev, n_cigar, the CIGAR words) agree between the two for every read.
//
// Compiled by hipcc (--offload-arch=gfx950 -x hip -c) the same file instantiates the core in two kernels of the shape of the
// library's: the test fails when the header does not build for the device.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "bpsw_sam_core.h"

namespace sc = bpsw::samcore;

#if defined(__HIPCC__)
__global__ __launch_bounds__(64) void sam_len_kernel(sc::SamBatch B, int n_lines, int32_t* len) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i < n_lines) len[i] = (int32_t)sc::sam_line_len(B, i);
}
__global__ __launch_bounds__(64) void sam_write_kernel(sc::SamBatch B, int n_lines, const long long* line_off, char* text, int* status) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  int st = 0;
  sc::sam_line_write(text + line_off[i], text + line_off[i + 1], B, i, line_off[i + 1] - line_off[i], &st);
  if (st) atomicOr(status, st);
}
#endif

namespace {

struct Place {  // where an end lies: the five fields a line reads of its mate
  int rid = -1, is_rev = 0;
  long long pos = -1;
  std::vector<uint32_t> cig;
};

struct Batch {
  std::vector<sc::SamLine> lines;
  std::vector<sc::SamRead> reads;
  std::vector<uint32_t> cig;
  std::string md, names, ctg_names, rg;
  std::vector<uint8_t> seq, qual;
  std::vector<int32_t> ctg_at;
  std::vector<Place> mates;  // per read: h[1 - i], what the tail hands memAlnToSAM as the mate
  bool have_qual = true;
  int flavour = 0;
  sc::SamBatch view() const {
    sc::SamBatch B;
    B.lines = lines.data(); B.reads = reads.data(); B.cig = cig.data(); B.md = md.data(); B.seq = seq.data();
    B.qual = have_qual ? qual.data() : nullptr;
    B.names = names.data(); B.ctg_at = ctg_at.data(); B.ctg_names = ctg_names.data(); B.rg = rg.data();
    B.n_ctg = (int32_t)ctg_at.size() - 1; B.rg_len = (int32_t)rg.size(); B.flavour = flavour;
    return B;
  }
};

std::string num(long long v) {
  char b[32];
  snprintf(b, sizeof b, "%lld", v);
  return b;
}

// ---- the independent writer: the SAM columns of the line, joined by tabs ----------------------------------------------------------
std::string contig_of(const Batch& b, int rid) {
  if (rid >= 0 && rid + 1 < (int)b.ctg_at.size() && b.ctg_at[(size_t)rid + 1] > b.ctg_at[(size_t)rid])
    return b.ctg_names.substr((size_t)b.ctg_at[(size_t)rid], (size_t)(b.ctg_at[(size_t)rid + 1] - b.ctg_at[(size_t)rid]));
  return "ctg" + num(rid + 1);
}
std::string cigar_of(const Batch& b, const sc::SamLine& L, int clip_as) {  // clip_as < 0: the letters as they are
  std::string s;
  for (int k = 0; k < L.n_cigar; ++k) {
    const uint32_t w = b.cig[(size_t)L.cig_at + (size_t)k];
    int op = (int)(w & 0xf);
    if (clip_as >= 0 && (op == 3 || op == 4)) op = clip_as;
    s += num(w >> 4);
    s += "MIDSH"[op];
  }
  return s;
}
int rlen_of(const std::vector<uint32_t>& cig) {  // get_rlen
  int l = 0;
  for (uint32_t w : cig) if ((w & 0xf) == 0 || (w & 0xf) == 2) l += (int)(w >> 4);
  return l;
}
std::string ref_line(const Batch& b, int line) {
  const sc::SamLine& L = b.lines[(size_t)line];
  const sc::SamRead& R = b.reads[(size_t)L.read];
  const bool later = line != L.first;
  // mem_aln2sam works on copies of p and m
  Place p, m = b.mates[(size_t)L.read];
  p.rid = L.rid; p.pos = L.pos; p.is_rev = L.is_rev;
  p.cig.assign(b.cig.begin() + L.cig_at, b.cig.begin() + L.cig_at + L.n_cigar);
  int raw = L.flag | 0x1;
  if (p.rid < 0) raw |= 0x4;
  if (m.rid < 0) raw |= 0x8;
  if (p.rid < 0 && m.rid >= 0) { p.rid = m.rid; p.pos = m.pos; p.is_rev = m.is_rev; p.cig.clear(); }   // copy mate to alignment
  if (m.rid < 0 && p.rid >= 0) { m.rid = p.rid; m.pos = p.pos; m.is_rev = p.is_rev; m.cig.clear(); }   // copy alignment to mate
  if (p.is_rev) raw |= 0x10;
  if (m.is_rev) raw |= 0x20;
  const int printed = (raw & 0xffff) | ((raw & 0x10000) ? 0x100 : 0);
  const bool hidden = ((b.flavour == sc::FLAVOUR_SCALA ? printed : raw) & 0x100) != 0;
  std::vector<std::string> col;
  col.push_back(b.names.substr((size_t)R.name_at, (size_t)R.name_len));
  col.push_back(num(printed));
  if (p.rid >= 0) {
    col.push_back(contig_of(b, p.rid));
    col.push_back(num(p.pos + 1));
    col.push_back(num(L.mapq));
    std::string cg;
    for (uint32_t w : p.cig) {
      int op = (int)(w & 0xf);
      if (op == 3 || op == 4) op = later ? 4 : 3;
      cg += num(w >> 4);
      cg += "MIDSH"[op];
    }
    col.push_back(p.cig.empty() ? "*" : cg);
  } else {
    col.push_back("*"); col.push_back("0"); col.push_back("0"); col.push_back("*");
  }
  if (m.rid >= 0) {
    col.push_back(p.rid == m.rid ? std::string("=") : contig_of(b, m.rid));
    col.push_back(num(m.pos + 1));
    long long tlen = 0;
    if (p.rid == m.rid && !m.cig.empty() && !p.cig.empty()) {
      const long long p0 = p.pos + (p.is_rev ? rlen_of(p.cig) - 1 : 0), p1 = m.pos + (m.is_rev ? rlen_of(m.cig) - 1 : 0);
      tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
    }
    col.push_back(num(tlen));
  } else {
    col.push_back("*"); col.push_back("0"); col.push_back("0");
  }
  if (hidden) {
    col.push_back("*"); col.push_back("*");
  } else {
    int head = 0, tail = 0;  // bases cut off the ALIGNED strand's front and back on later lines
    if (later && !p.cig.empty()) {
      const uint32_t f = p.cig.front(), l = p.cig.back();
      if ((f & 0xf) == 3 || (f & 0xf) == 4) head = (int)(f >> 4);
      if ((l & 0xf) == 3 || (l & 0xf) == 4) tail = (int)(l >> 4);
    }
    std::string bases, quals;
    for (int i = 0; i < R.len; ++i) {  // the whole read on the strand it is printed on, then the cut
      const int at = p.is_rev ? R.len - 1 - i : i;
      const int c = b.seq[(size_t)R.seq_at + (size_t)at] > 4 ? 4 : b.seq[(size_t)R.seq_at + (size_t)at];
      bases += p.is_rev ? "TGCAN"[c] : "ACGTN"[c];
      if (b.have_qual) quals += (char)b.qual[(size_t)R.seq_at + (size_t)at];
    }
    const int keep = R.len - head - tail > 0 ? R.len - head - tail : 0;
    col.push_back(keep ? bases.substr((size_t)head, (size_t)keep) : "");
    col.push_back(b.have_qual ? (keep ? quals.substr((size_t)head, (size_t)keep) : "") : "*");
  }
  if (!p.cig.empty()) {
    col.push_back("NM:i:" + num(L.NM));
    col.push_back("MD:Z:" + (L.md_len > 0 ? b.md.substr((size_t)L.md_at, (size_t)L.md_len) : std::string()));
  }
  if (L.score >= 0) col.push_back("AS:i:" + num(L.score));
  if (L.sub >= 0) col.push_back("XS:i:" + num(L.sub));
  if (!b.rg.empty()) col.push_back("RG:Z:" + b.rg);
  if (!hidden) {  // the list runs over the read's own lines as they are: the copy above is none of its business
    std::string sa;
    for (int i = 0; i < L.n_list; ++i) {
      const sc::SamLine& o = b.lines[(size_t)(L.first + i)];
      if (L.first + i == line || (o.flag & 0x100)) continue;
      sa += contig_of(b, o.rid) + "," + num(o.pos + 1) + "," + (o.is_rev ? "-" : "+") + "," + cigar_of(b, o, -1) + "," + num(o.mapq) + "," +
            num(o.NM) + ";";
    }
    if (!sa.empty()) col.push_back("SA:Z:" + sa);
  }
  std::string out;
  for (size_t k = 0; k < col.size(); ++k) { if (k) out += '\t'; out += col[k]; }
  return out + "\n";
}

// ---- generated batches -----------------------------------------------------------------------------------------------------------
typedef std::mt19937_64 Rng;
int pick(Rng& g, int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }

long long a_pos(Rng& g) {
  return pick(g, 0, 3) == 0 ? (long long)(g() % (1ull << 40)) : pick(g, 0, 3) == 0 ? (long long)pick(g, 0, 10) : (long long)(g() % 3000000000ull);
}
void a_cigar(Rng& g, int read_len, int n, std::vector<uint32_t>* out) {
  out->clear();
  int budget = read_len;  // the clips of a line stay inside the read
  for (int k = 0; k < n; ++k) {
    int op = pick(g, 0, 2), len = pick(g, 1, pick(g, 0, 3) == 0 ? 100000 : 150);
    const bool edge = k == 0 || k == n - 1;
    if (edge && n > 1 && pick(g, 0, 1) && budget > 0) { op = pick(g, 0, 4) == 0 ? 4 : 3; len = pick(g, 1, budget); budget -= len; }
    out->push_back((uint32_t)len << 4 | (uint32_t)op);
  }
  if (n == 1 && pick(g, 0, 15) == 0) out->back() = (uint32_t)pick(g, 1, read_len) << 4 | 3u;  // a line that is one clip
}

// one read: its list starts with the line of `h` (the tail's h[i]: the unmapped record when h.rid < 0)
void add_read(Batch& b, Rng& g, int n_list, const Place& h, int read_len, int end) {
  sc::SamRead R;
  R.len = read_len;
  R.name_len = pick(g, 0, 5) == 0 ? (pick(g, 0, 1) ? 1 : 254) : pick(g, 1, 254);
  R.seq_at = (long long)b.seq.size();
  R.name_at = (long long)b.names.size();
  for (int i = 0; i < R.len; ++i) { b.seq.push_back((uint8_t)(pick(g, 0, 19) == 0 ? 4 : pick(g, 0, 3))); b.qual.push_back((uint8_t)pick(g, 33, 126)); }
  for (int i = 0; i < R.name_len; ++i) b.names += (char)pick(g, 33, 126);
  const int read = (int)b.reads.size(), first = (int)b.lines.size();
  b.reads.push_back(R);
  const int xf = (end ? 0x81 : 0x41) | (pick(g, 0, 1) ? 2 : 0);
  for (int x = 0; x < n_list; ++x) {
    sc::SamLine L;
    memset(&L, 0, sizeof L);
    L.read = read; L.first = first; L.n_list = n_list;
    const bool unmapped = x == 0 ? h.rid < 0 : pick(g, 0, 11) == 0;
    std::vector<uint32_t> cig;
    if (unmapped) {
      L.rid = -1; L.pos = -1;
    } else {
      if (x == 0) {
        L.rid = h.rid; L.pos = h.pos; L.is_rev = h.is_rev; cig = h.cig;
      } else {
        L.rid = pick(g, 0, (int)b.ctg_at.size() + 1);  // (also past the table)
        L.pos = a_pos(g);
        L.is_rev = pick(g, 0, 1);
        a_cigar(g, R.len, pick(g, 0, 19) == 0 ? 0 : pick(g, 0, 7) == 0 ? pick(g, 1, 64) : pick(g, 1, 6), &cig);
      }
      L.mapq = pick(g, 0, 60);
      L.NM = pick(g, 0, 40);
      L.n_cigar = (int)cig.size();
      L.cig_at = (long long)b.cig.size();
      b.cig.insert(b.cig.end(), cig.begin(), cig.end());
      L.md_len = L.n_cigar > 0 ? pick(g, 0, 80) : 0;
      L.md_at = (long long)b.md.size();
      for (int k = 0; k < L.md_len; ++k) b.md += "0123456789ACGT^"[pick(g, 0, 14)];
    }
    L.score = unmapped ? 0 : pick(g, 0, 9) == 0 ? -1 : pick(g, 0, 1100);
    L.sub = unmapped ? 0 : pick(g, 0, 3) == 0 ? -1 : pick(g, 0, 1100);
    const int kind = pick(g, 0, 5);
    L.flag = xf | (kind == 0 && x ? 0x100 : kind == 1 && x ? 0x800 : kind == 2 && x ? 0x10000 : 0);   // (line 0 is a primary hit in the tail)
    b.lines.push_back(L);
  }
}

Place a_place(Rng& g, const Batch& b, int read_len) {
  Place h;
  if (pick(g, 0, 3) == 0) return h;  // the unmapped record
  h.rid = pick(g, 0, (int)b.ctg_at.size() + 1);
  h.pos = a_pos(g);
  h.is_rev = pick(g, 0, 1);
  a_cigar(g, read_len, pick(g, 0, 7) == 0 ? 0 : pick(g, 0, 7) == 0 ? pick(g, 1, 64) : pick(g, 1, 6), &h.cig);
  return h;
}

int a_read_len(Rng& g) { return pick(g, 0, 9) == 0 ? pick(g, 1, 3) : pick(g, 0, 3) == 0 ? pick(g, 1, 1024) : pick(g, 30, 260); }
int a_list(Rng& g) {
  const int shape = pick(g, 0, 39);
  return shape == 0 ? 100 : shape < 4 ? pick(g, 5, 40) : shape < 16 ? pick(g, 2, 4) : 1;
}

void add_pair(Batch& b, Rng& g) {
  const int len[2] = {a_read_len(g), a_read_len(g)};
  Place h[2];
  h[0] = a_place(g, b, len[0]);
  h[1] = a_place(g, b, len[1]);
  if (h[0].rid >= 0 && h[1].rid >= 0 && pick(g, 0, 2)) {  // the same contig, near or at the same place, before or behind
    h[1].rid = h[0].rid;
    const long long d = pick(g, 0, 5) == 0 ? 0 : pick(g, -700, 700);
    h[1].pos = h[0].pos + d < 0 ? 0 : h[0].pos + d;
  }
  const int first[2] = {(int)b.lines.size(), 0};
  int n_list[2];
  for (int i = 0; i < 2; ++i) n_list[i] = h[i].rid < 0 && pick(g, 0, 3) ? 1 : a_list(g);   // (the tail prints an unplaced end as one line)
  add_read(b, g, n_list[0], h[0], len[0], 0);
  const int first1 = (int)b.lines.size();
  add_read(b, g, n_list[1], h[1], len[1], 1);
  for (int x = 0; x < n_list[0]; ++x) b.lines[(size_t)(first[0] + x)].mate = first1 + 1;
  for (int x = 0; x < n_list[1]; ++x) b.lines[(size_t)(first1 + x)].mate = first[0] + 1;
  b.mates.push_back(h[1]);
  b.mates.push_back(h[0]);
}

Batch make_batch(Rng& g, int variant, int n_lines_min) {
  Batch b;
  b.flavour = variant & 1;
  b.have_qual = !(variant & 2);
  if (variant & 4) for (int i = pick(g, 1, 63); i > 0; --i) b.rg += (char)pick(g, 33, 126);
  const int n_ctg = (variant & 8) ? pick(g, 1, 40) : 0;
  b.ctg_at.push_back(0);
  for (int k = 0; k < n_ctg; ++k) {
    const int l = pick(g, 0, 4) == 0 ? 0 : pick(g, 1, 40);  // (an empty name prints as ctgN)
    for (int i = 0; i < l; ++i) b.ctg_names += (char)pick(g, 48, 122);
    b.ctg_at.push_back((int32_t)b.ctg_names.size());
  }
  while ((int)b.lines.size() < n_lines_min) add_pair(b, g);
  return b;
}

// what the core relies on: the record the tail prints a read's lines against equals, in the five fields a line reads of a mate,
// the first line of the pair's other read
int check_mates(const Batch& b) {
  for (int r = 0; r < (int)b.reads.size(); ++r) {
    const Place& m = b.mates[(size_t)r];
    int first_other = -1;
    for (int i = 0; i < (int)b.lines.size(); ++i) if (b.lines[(size_t)i].read == (r ^ 1)) { first_other = b.lines[(size_t)i].first; break; }
    if (first_other < 0) { fprintf(stderr, "read %d: the other read has no line\n", r); return 1; }
    const sc::SamLine& f = b.lines[(size_t)first_other];
    bool same = m.rid == f.rid && m.pos == f.pos && m.is_rev == f.is_rev && (int)m.cig.size() == f.n_cigar;
    for (int k = 0; same && k < f.n_cigar; ++k) same = m.cig[(size_t)k] == b.cig[(size_t)f.cig_at + (size_t)k];
    if (!same) { fprintf(stderr, "read %d: h[1 - i] is not the first line of the other read\n", r); return 1; }
    for (int i = 0; i < (int)b.lines.size(); ++i)
      if (b.lines[(size_t)i].read == r && b.lines[(size_t)i].mate != first_other + 1) { fprintf(stderr, "line %d names another mate\n", i); return 1; }
  }
  return 0;
}

struct Census {
  long long mix[2][2] = {{0, 0}, {0, 0}};  // [line unmapped][mate unmapped]
  long long tlen_pos = 0, tlen_neg = 0, other_ctg = 0, past_table = 0, no_cigar_line = 0, no_cigar_mate = 0, supp = 0, sec = 0, multi = 0, far = 0;
  long long rev[2][2] = {{0, 0}, {0, 0}};
};
void count(const Batch& b, Census* c) {
  for (const sc::SamLine& L : b.lines) {
    const Place& m = b.mates[(size_t)L.read];
    ++c->mix[L.rid < 0][m.rid < 0];
    if (L.rid >= 0 && m.rid >= 0) {
      ++c->rev[L.is_rev != 0][m.is_rev != 0];
      if (L.rid != m.rid) ++c->other_ctg;
      else if (L.n_cigar > 0 && !m.cig.empty()) { if (L.pos <= m.pos) ++c->tlen_pos; else ++c->tlen_neg; }
      if (m.rid >= (int)b.ctg_at.size() - 1) ++c->past_table;
      if (L.n_cigar == 0) ++c->no_cigar_line;
      if (m.cig.empty()) ++c->no_cigar_mate;
    }
    if (L.flag & 0x800) ++c->supp;
    if (L.flag & 0x100) ++c->sec;
    if (L.flag & 0x10000) ++c->multi;
    if (m.pos >= (1ll << 32) || L.pos >= (1ll << 32)) ++c->far;
  }
}

int check_batch(const Batch& b, Rng& g, long long* bytes) {
  const sc::SamBatch B = b.view();
  for (int i = 0; i < (int)b.lines.size(); ++i) {
    const std::string want = ref_line(b, i);
    const long long len = sc::sam_line_len(B, i);
    if (len != (long long)want.size()) { fprintf(stderr, "line %d: sam_line_len %lld, the independent writer %zu\n", i, len, want.size()); return 1; }
    char* blk = (char*)malloc((size_t)len);  // exactly the line: a store past it is a sanitizer report
    int st = -1;
    const long long wrote = sc::sam_line_write(blk, blk + len, B, i, len, &st);
    if (wrote != len || st != 0) { fprintf(stderr, "line %d: wrote %lld of %lld, status %d\n", i, wrote, len, st); return 1; }
    if (memcmp(blk, want.data(), (size_t)len) != 0) {
      fprintf(stderr, "line %d differs:\n got %.*s want %s", i, (int)len, blk, want.c_str());
      return 1;
    }
    free(blk);
    *bytes += len;
    // a too-small end: refused with the status, and the block of `room` bytes is all it may touch
    const long long room = pick(g, 0, 2) == 0 ? len - 1 : (long long)(g() % (uint64_t)len);
    char* small = (char*)malloc((size_t)room + 1);
    small[room] = 0x5a;
    st = -1;
    const long long n2 = sc::sam_line_write(small, small + room, B, i, len, &st);
    if (n2 != len || !(st & sc::ST_OVERRUN) || small[room] != 0x5a) { fprintf(stderr, "line %d: a short end gave %lld, status %d\n", i, n2, st); return 1; }
    free(small);
    if ((i & 63) == 0) {  // another length than expected is reported, with room to spare
      char* big = (char*)malloc((size_t)len + 8);
      sc::sam_line_write(big, big + len + 8, B, i, len + 1, &st);
      if (st != sc::ST_MISMATCH) { fprintf(stderr, "line %d: an unexpected length gave status %d\n", i, st); return 1; }
      free(big);
    }
  }
  return 0;
}

}  // namespace

int main() {
  Rng g(20261019);
  long long lines = 0, bytes = 0, reads = 0, longest_list = 0;
  Census c;
  for (int variant = 0; variant < 32; ++variant) {
    const Batch b = make_batch(g, variant, 700);
    if (check_mates(b) || check_batch(b, g, &bytes)) { fprintf(stderr, "(variant %d)\n", variant); return 1; }
    count(b, &c);
    lines += (long long)b.lines.size();
    reads += (long long)b.reads.size();
    for (const sc::SamLine& L : b.lines) if (L.n_list > longest_list) longest_list = L.n_list;
  }
  if (lines < 20000 || longest_list != 100) { fprintf(stderr, "only %lld lines, longest list %lld\n", lines, longest_list); return 1; }
  const long long least[] = {c.mix[0][0], c.mix[0][1], c.mix[1][0], c.mix[1][1], c.rev[0][0], c.rev[0][1], c.rev[1][0], c.rev[1][1], c.tlen_pos, c.tlen_neg,
                             c.other_ctg, c.past_table, c.no_cigar_line, c.no_cigar_mate, c.supp, c.sec, c.multi, c.far};
  for (long long v : least)
    if (v < 50) { fprintf(stderr, "a case of the mix has only %lld lines\n", v); return 1; }
  printf("sam core with a mate: %lld lines of %lld reads, %lld bytes, both flavours: equal to the independent writer\n", lines, reads, bytes);
  printf("  mapped/mapped %lld, mapped beside unmapped %lld, unmapped at its mate %lld, both unmapped %lld; same contig with TLEN %lld+%lld, "
         "another contig %lld, mate past the table %lld, no CIGAR %lld / mate's %lld, 0x800 %lld, 0x100 %lld, 0x10000 %lld, past 2^32 %lld\n",
         c.mix[0][0], c.mix[0][1], c.mix[1][0], c.mix[1][1], c.tlen_pos, c.tlen_neg, c.other_ctg, c.past_table, c.no_cigar_line, c.no_cigar_mate, c.supp,
         c.sec, c.multi, c.far);
  return 0;
}
