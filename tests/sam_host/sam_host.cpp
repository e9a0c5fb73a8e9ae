// sam_host.cpp -- csrc/bpsw_sam_core.h (the bytes of a SAM line without a mate, what sam_len_kernel / sam_write_kernel compile)
// on the host, against an independent writer of the same line made of std::string and snprintf.
//
// A program of its own (tests/test_sam_core_host.py builds it with -fsanitize=address,undefined): seeded random batches of line
// records -- names of 1-254 bytes, positions up to 2^40, reads of 1-1 024 bases, CIGARs of 1-64 operations with and without
// clips, first and later lines, both strands, secondary / supplementary / unmapped, with and without qualities, read group and
// contig names, SA lists of 0-100 entries, both flavours.  Per line: sam_line_len == the bytes sam_line_write wrote == the
// independent writer's, the bytes are equal, the line is written into a heap block of exactly its length (an overrun is a
// sanitizer report), and a too-small `end` is refused with the status and nothing is written past it.
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

struct Batch {
  std::vector<sc::SamLine> lines;
  std::vector<sc::SamRead> reads;
  std::vector<uint32_t> cig;
  std::string md, names, ctg_names, rg;
  std::vector<uint8_t> seq, qual;
  std::vector<int32_t> ctg_at;
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
std::string ref_line(const Batch& b, int line) {
  const sc::SamLine& L = b.lines[(size_t)line];
  const sc::SamRead& R = b.reads[(size_t)L.read];
  const bool later = line != L.first;
  const int raw = L.flag | (L.rid < 0 ? 0x4 : 0) | (L.is_rev ? 0x10 : 0);
  const int printed = (raw & 0xffff) | ((raw & 0x10000) ? 0x100 : 0);
  const bool hidden = ((b.flavour == sc::FLAVOUR_SCALA ? printed : raw) & 0x100) != 0;
  std::vector<std::string> col;
  col.push_back(b.names.substr((size_t)R.name_at, (size_t)R.name_len));
  col.push_back(num(printed));
  if (L.rid >= 0) {
    col.push_back(contig_of(b, L.rid));
    col.push_back(num(L.pos + 1));
    col.push_back(num(L.mapq));
    col.push_back(L.n_cigar > 0 ? cigar_of(b, L, later ? 4 : 3) : "*");
  } else {
    col.push_back("*"); col.push_back("0"); col.push_back("0"); col.push_back("*");
  }
  col.push_back("*"); col.push_back("0"); col.push_back("0");
  if (hidden) {
    col.push_back("*"); col.push_back("*");
  } else {
    int head = 0, tail = 0;  // bases cut off the ALIGNED strand's front and back on later lines
    if (later && L.n_cigar > 0) {
      const uint32_t f = b.cig[(size_t)L.cig_at], l = b.cig[(size_t)L.cig_at + (size_t)L.n_cigar - 1];
      if ((f & 0xf) == 3 || (f & 0xf) == 4) head = (int)(f >> 4);
      if ((l & 0xf) == 3 || (l & 0xf) == 4) tail = (int)(l >> 4);
    }
    std::string bases, quals;
    for (int i = 0; i < R.len; ++i) {  // the whole read on the aligned strand, then the cut
      const int at = L.is_rev ? R.len - 1 - i : i;
      const int c = b.seq[(size_t)R.seq_at + (size_t)at] > 4 ? 4 : b.seq[(size_t)R.seq_at + (size_t)at];
      bases += L.is_rev ? "TGCAN"[c] : "ACGTN"[c];
      if (b.have_qual) quals += (char)b.qual[(size_t)R.seq_at + (size_t)at];
    }
    const int keep = R.len - head - tail > 0 ? R.len - head - tail : 0;
    col.push_back(keep ? bases.substr((size_t)head, (size_t)keep) : "");
    col.push_back(b.have_qual ? (keep ? quals.substr((size_t)head, (size_t)keep) : "") : "*");
  }
  if (L.n_cigar > 0) {
    col.push_back("NM:i:" + num(L.NM));
    col.push_back("MD:Z:" + (L.md_len > 0 ? b.md.substr((size_t)L.md_at, (size_t)L.md_len) : std::string()));
  }
  if (L.score >= 0) col.push_back("AS:i:" + num(L.score));
  if (L.sub >= 0) col.push_back("XS:i:" + num(L.sub));
  if (!b.rg.empty()) col.push_back("RG:Z:" + b.rg);
  if (!hidden) {
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

void add_read(Batch& b, Rng& g, int n_list) {
  sc::SamRead R;
  R.len = pick(g, 0, 9) == 0 ? pick(g, 1, 3) : pick(g, 0, 3) == 0 ? pick(g, 1, 1024) : pick(g, 30, 260);
  R.name_len = pick(g, 0, 5) == 0 ? (pick(g, 0, 1) ? 1 : 254) : pick(g, 1, 254);
  R.seq_at = (long long)b.seq.size();
  R.name_at = (long long)b.names.size();
  for (int i = 0; i < R.len; ++i) { b.seq.push_back((uint8_t)(pick(g, 0, 19) == 0 ? 4 : pick(g, 0, 3))); b.qual.push_back((uint8_t)pick(g, 33, 126)); }
  for (int i = 0; i < R.name_len; ++i) b.names += (char)pick(g, 33, 126);
  const int read = (int)b.reads.size(), first = (int)b.lines.size();
  b.reads.push_back(R);
  for (int x = 0; x < n_list; ++x) {
    sc::SamLine L;
    memset(&L, 0, sizeof L);
    L.read = read; L.first = first; L.n_list = n_list;
    const bool unmapped = pick(g, 0, 11) == 0;
    if (unmapped) {
      L.rid = -1; L.pos = -1;
    } else {
      L.rid = pick(g, 0, (int)b.ctg_at.size() + 1);  // (also past the table)
      L.pos = pick(g, 0, 3) == 0 ? (long long)(g() % (1ull << 40)) : pick(g, 0, 3) == 0 ? (long long)pick(g, 0, 10) : (long long)(g() % 3000000000ull);
      L.is_rev = pick(g, 0, 1);
      L.mapq = pick(g, 0, 60);
      L.NM = pick(g, 0, 40);
      L.n_cigar = pick(g, 0, 19) == 0 ? 0 : pick(g, 0, 7) == 0 ? pick(g, 1, 64) : pick(g, 1, 6);
      L.cig_at = (long long)b.cig.size();
      int budget = R.len;  // the clips of a line stay inside the read
      for (int k = 0; k < L.n_cigar; ++k) {
        int op = pick(g, 0, 2), len = pick(g, 1, pick(g, 0, 3) == 0 ? 100000 : 150);
        const bool edge = k == 0 || k == L.n_cigar - 1;
        if (edge && L.n_cigar > 1 && pick(g, 0, 1) && budget > 0) { op = pick(g, 0, 4) == 0 ? 4 : 3; len = pick(g, 1, budget); budget -= len; }
        b.cig.push_back((uint32_t)len << 4 | (uint32_t)op);
      }
      if (L.n_cigar == 1 && pick(g, 0, 15) == 0) b.cig.back() = (uint32_t)pick(g, 1, R.len) << 4 | 3u;  // a line that is one clip
      L.md_len = L.n_cigar > 0 ? pick(g, 0, 80) : 0;
      L.md_at = (long long)b.md.size();
      for (int k = 0; k < L.md_len; ++k) b.md += "0123456789ACGT^"[pick(g, 0, 14)];
    }
    L.score = unmapped ? 0 : pick(g, 0, 9) == 0 ? -1 : pick(g, 0, 1100);
    L.sub = unmapped ? 0 : pick(g, 0, 3) == 0 ? -1 : pick(g, 0, 1100);
    const int kind = pick(g, 0, 5);
    L.flag = kind == 0 ? 0x100 : kind == 1 && x ? 0x800 : kind == 2 && x ? 0x10000 : 0;
    b.lines.push_back(L);
  }
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
  while ((int)b.lines.size() < n_lines_min) {
    const int shape = pick(g, 0, 39);
    add_read(b, g, shape == 0 ? 101 : shape < 4 ? pick(g, 5, 40) : shape < 16 ? pick(g, 2, 4) : 1);
  }
  return b;
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
  Rng g(20261018);
  long long lines = 0, bytes = 0, reads = 0, longest_list = 0;
  for (int variant = 0; variant < 32; ++variant) {
    const Batch b = make_batch(g, variant, 700);
    if (check_batch(b, g, &bytes)) { fprintf(stderr, "(variant %d)\n", variant); return 1; }
    lines += (long long)b.lines.size();
    reads += (long long)b.reads.size();
    for (const sc::SamLine& L : b.lines) if (L.n_list > longest_list) longest_list = L.n_list;
  }
  if (lines < 20000 || longest_list != 101) { fprintf(stderr, "only %lld lines, longest list %lld\n", lines, longest_list); return 1; }
  printf("sam core: %lld lines of %lld reads, %lld bytes, both flavours: equal to the independent writer\n", lines, reads, bytes);
  return 0;
}
