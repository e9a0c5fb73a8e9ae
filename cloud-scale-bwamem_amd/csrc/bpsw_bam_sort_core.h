// bpsw_bam_sort_core.h -- the rules of bpsw_bam_sort: how a stream of BAM records is walked, what is asked of a record, the key it is
// sorted by, and the BAI that says where the sorted records went.  For the host and for the device.
//
// A record is read a byte at a time: it begins at any offset of its stream.  Of its fixed part (specification 4.2) the rules use
//   +0 block_size   +4 refID   +8 pos   +12 l_read_name   +16 n_cigar_op (u16)   +18 flag (u16)   +20 l_seq
// and the CIGAR behind the name, at +36 + l_read_name.
//
// The walk: from a segment's first byte follow block_size; a length field that is cut by the segment's end, or a record that runs past
// it, is a broken chain (walk_step).  The checks (check_record), in the order the entry documents them, give the reason of a record; the
// lowest bad record of a stream is the one reported.  The key (check_record):
//   refID' << (pos_bits + 1) | (pos + 1) << 1 | rev        refID' = refID, or n_seqs for -1;  rev = flag bit 0x10
//   pos_bits = the width of the longest contig's length (pos + 1 lies in 0 .. length);  refID' has the width of n_seqs
// so that a stable sort by the key's low key_bits bits is the order (refID with -1 last, pos, strand, input order).
//
// The BAI (build_bai) is assembled on the calling thread from one Entry per record in sorted order, by the specification's 5.2 and
// these rules: a chunk is a maximal run of consecutive records with the same (refID, bin), bin = reg2bin(pos, end) recomputed; the
// pseudo-bin 37450 comes last per contig; a linear window's entry is the start of the first record that overlaps it, a window that none
// overlaps takes the next window's, n_intv is the last overlapped window + 1; a contig without records has n_bin = n_intv = 0.
//
// Compiled by hipcc for bam_walk_kernel / bam_key_kernel / bam_gather_kernel (bpsw_bam_sort.hip) and by g++ for
// tests/bam_sort_host/bam_sort_host.cpp.
#pragma once

#include <stdint.h>

#include "bpsw_bam_core.h"

namespace bpsw {
namespace bamsort {

namespace bc = bpsw::bamcore;

constexpr long long kMaxContig = 1ll << 29;   // the longest contig a BAI's bins hold
constexpr int kFixed = 32;                    // the bytes of a record's fixed part behind block_size
constexpr int kWindowDefault = 4096;          // bam_walk_kernel's window: the bytes of the stream a wavefront holds in LDS
constexpr int kWindowMin = 64, kWindowMax = 16384;
constexpr int kPseudoBin = 37450;
constexpr int kLinearShift = 14;

enum Reason {
  R_OK = 0,
  R_BLOCK_SIZE = 1,  // block_size below 32 + l_read_name + 4 n_cigar_op + ceil(l_seq / 2) + l_seq
  R_REF_ID = 2,      // refID outside [-1, n_seqs)
  R_POS = 3,         // pos below -1, or at or above its contig's length (a record without a contig has none: its pos is -1)
};

BPSW_SAM_HD uint32_t rd_u16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
BPSW_SAM_HD uint32_t rd_u32(const uint8_t* p) { return rd_u16(p) | rd_u16(p + 2) << 16; }
BPSW_SAM_HD int32_t rd_i32(const uint8_t* p) { return (int32_t)rd_u32(p); }

BPSW_SAM_HD int width_of(unsigned long long max_value) {  // bits that hold 0 .. max_value
  int b = 0;
  while (b < 64 && (max_value >> b)) ++b;
  return b;
}

struct KeyShape {
  int32_t n_seqs;
  int pos_bits, ref_bits;
};
BPSW_SAM_HD KeyShape key_shape(int32_t n_seqs, long long longest) {
  KeyShape k;
  k.n_seqs = n_seqs;
  k.pos_bits = width_of((unsigned long long)longest);
  k.ref_bits = width_of((unsigned long long)n_seqs);
  return k;
}
BPSW_SAM_HD int key_bits(const KeyShape& k) { return k.ref_bits + k.pos_bits + 1; }  // (31 + 30 + 1 at the most)

// One step of the walk: the record at `at` of a segment that ends at `end`, its length field read from `len4` (the four bytes at `at`).
// -> the offset behind the record, or -1: the chain is broken here.
BPSW_SAM_HD long long walk_step(long long at, long long end, const uint8_t* len4) {
  if (at + 4 > end) return -1;
  const long long next = at + 4 + (long long)rd_u32(len4);
  return next > end ? -1 : next;
}

// What the key, the index and the gather need of a record
struct Meta {
  int32_t ref, pos, end;   // end: pos + the reference bases of the CIGAR (M D N = X), pos + 1 without any or at pos -1; at most 2^30
  uint32_t len_unmapped;   // the record's bytes with block_size's four | flag bit 4 << 31
};
// A record in sorted order, as the calling thread gets it
struct Entry {
  int32_t ref, pos, end;
  uint32_t off_unmapped;   // the record's offset in the sorted stream | flag bit 4 << 31
};

// The record at r (its 4 + block_size bytes lie inside the stream: the walk's verdict), contig lengths len[n_seqs] -> the reason, or 0
// with *key and *m filled.
BPSW_SAM_HD int check_record(const uint8_t* r, const KeyShape& ks, const int32_t* len, unsigned long long* key, Meta* m) {
  const uint32_t bs = rd_u32(r);
  if (bs < (uint32_t)kFixed) return R_BLOCK_SIZE;
  const int32_t ref = rd_i32(r + 4), pos = rd_i32(r + 8);
  const uint32_t l_name = r[12], n_cigar = rd_u16(r + 16), flag = rd_u16(r + 18), l_seq = rd_u32(r + 20);
  const unsigned long long least = (unsigned long long)kFixed + l_name + 4ull * n_cigar + ((unsigned long long)l_seq + 1) / 2 + l_seq;
  if (bs < least) return R_BLOCK_SIZE;
  if (ref < -1 || ref >= ks.n_seqs) return R_REF_ID;
  const long long room = ref < 0 ? 0 : (long long)len[ref];
  if (pos < -1 || (pos >= 0 && (long long)pos >= room)) return R_POS;
  long long ref_len = 0;
  const uint8_t* cig = r + 4 + kFixed + l_name;
  for (uint32_t k = 0; k < n_cigar; ++k) {
    const uint32_t w = rd_u32(cig + 4 * k), op = w & 0xf;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (long long)(w >> 4);
  }
  long long end = (long long)pos + (pos >= 0 && ref_len > 0 ? ref_len : 1);
  if (end > (1ll << 30)) end = 1ll << 30;
  m->ref = ref; m->pos = pos; m->end = (int32_t)end;
  m->len_unmapped = (bs + 4u) | ((flag >> 2) & 1u) << 31;
  const unsigned long long r1 = ref < 0 ? (unsigned long long)ks.n_seqs : (unsigned long long)ref;
  *key = r1 << (ks.pos_bits + 1) | (unsigned long long)(pos + 1) << 1 | ((flag >> 4) & 1u);
  return R_OK;
}

}  // namespace bamsort
}  // namespace bpsw

// ---- the calling thread's part: the BAI ---------------------------------------------------------------------------------------------
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace bpsw {
namespace bamsort {

inline const char* reason_text(int reason) {
  switch (reason) {
    case R_BLOCK_SIZE: return "block_size is below 32 + l_read_name + 4 n_cigar_op + ceil(l_seq / 2) + l_seq";
    case R_REF_ID: return "refID is outside [-1, n_seqs)";
    case R_POS: return "pos is below -1, or at or above its contig's length";
    default: return "no reason";
  }
}

// Where the blocks of the output begin: block b of the sorted stream (P bytes each, the last one shorter) is at coff[b], coff[blocks] is
// the output's size.  The virtual offset of stream offset o: (file_off + coff[o / P]) << 16 | o % P.
struct Blocks {
  const long long* coff;
  long long P, file_off;
  unsigned long long voff(long long o) const { return (unsigned long long)(file_off + coff[o / P]) << 16 | (unsigned long long)(o % P); }
};

inline void put_le(std::vector<uint8_t>& out, unsigned long long v, int bytes) {
  for (int k = 0; k < bytes; ++k) out.push_back((uint8_t)(v >> (8 * k)));
}

// e[0, n) in sorted order (refID ascending, -1 last), S: the sorted stream's size (the last record's end) -> the BAI's bytes
inline void build_bai(const Entry* e, long long n, long long S, int32_t n_ref, const Blocks& B, std::vector<uint8_t>* bai) {
  typedef std::pair<unsigned long long, unsigned long long> Chunk;
  const unsigned long long kNone = ~0ull;   // (no virtual offset: the low 16 bits stay below 65536 - 256)
  std::vector<uint8_t>& out = *bai;
  out.clear();
  out.push_back('B'); out.push_back('A'); out.push_back('I'); out.push_back(1);
  put_le(out, (uint32_t)n_ref, 4);
  auto start_of = [&](long long i) { return (long long)(e[i].off_unmapped & 0x7fffffffu); };
  auto end_of = [&](long long i) { return i + 1 < n ? start_of(i + 1) : S; };
  long long at = 0;
  for (int32_t ref = 0; ref < n_ref; ++ref) {
    const long long first = at;
    std::map<uint32_t, std::vector<Chunk>> bins;
    std::vector<unsigned long long> linear;
    unsigned long long mapped = 0, unmapped = 0;
    int last_bin = -1;
    for (; at < n && e[at].ref == ref; ++at) {
      const long long beg = e[at].pos, end = e[at].end;
      const int bin = bc::reg2bin(beg, end);
      const unsigned long long v0 = B.voff(start_of(at)), v1 = B.voff(end_of(at));
      if (bin == last_bin) bins[(uint32_t)bin].back().second = v1;
      else bins[(uint32_t)bin].push_back(Chunk(v0, v1));
      last_bin = bin;
      if (e[at].off_unmapped >> 31) ++unmapped; else ++mapped;
      const long long w0 = (beg < 0 ? 0 : beg) >> kLinearShift, w1 = (end < 1 ? 0 : end - 1) >> kLinearShift;
      if ((long long)linear.size() <= w1) linear.resize((size_t)w1 + 1, kNone);
      for (long long w = w0; w <= w1; ++w)
        if (linear[(size_t)w] == kNone) linear[(size_t)w] = v0;   // (sorted: the first record to reach a window has the lowest start)
    }
    if (at == first) { put_le(out, 0, 4); put_le(out, 0, 4); continue; }
    put_le(out, (uint32_t)bins.size() + 1, 4);
    for (const auto& b : bins) {
      put_le(out, b.first, 4);
      put_le(out, (uint32_t)b.second.size(), 4);
      for (const Chunk& c : b.second) { put_le(out, c.first, 8); put_le(out, c.second, 8); }
    }
    put_le(out, (uint32_t)kPseudoBin, 4);
    put_le(out, 2, 4);
    put_le(out, B.voff(start_of(first)), 8); put_le(out, B.voff(end_of(at - 1)), 8);
    put_le(out, mapped, 8); put_le(out, unmapped, 8);
    for (size_t w = linear.size(); w-- > 1;)
      if (linear[w - 1] == kNone) linear[w - 1] = linear[w];
    put_le(out, (uint32_t)linear.size(), 4);
    for (unsigned long long v : linear) put_le(out, v, 8);
  }
  put_le(out, (unsigned long long)(n - at), 8);   // n_no_coor: what is left has refID -1
}

}  // namespace bamsort
}  // namespace bpsw
