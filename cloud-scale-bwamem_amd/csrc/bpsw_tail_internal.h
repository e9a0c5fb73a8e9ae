// bpsw_tail_internal.h -- the pieces of worker2's tail (bpsw_tail.cpp) that the single-end tail (bpsw_sam_se.hip) uses as they
// are: the contig table's snapshot, memMarkPrimarySe, the reg2aln launches with their resubmission, the mem_aln_t of a job and
// the SAM line on the calling thread.  Defined in bpsw_tail.cpp; not installed.
#pragma once

#include <string.h>

#include <string>
#include <vector>

#include "bpsw_internal.h"

namespace bpsw {

struct BnsView {
  long long l_pac = 0;
  const uint8_t* d_pac = nullptr;
  int n_seqs = 0;
  const long long* d_off = nullptr;
  const int32_t* d_len = nullptr;
  std::vector<long long> off;
  std::vector<int32_t> len;
  std::vector<std::string> name;
  RefHold hold;  // the reference and the contig table stay put while this view lives
};
int snapshot_bns(const bpsw_ctx* c, BnsView* v);

struct JobResult {
  Reg2AlnOut k;
  size_t cig_at = 0, md_at = 0;  // its CIGAR words / MD bytes in JobResults::cig / ::md (k.n_cigar, k.md_len of them)
};
struct JobResults {  // one allocation per kind and call, not two per job
  std::vector<JobResult> r;
  std::vector<uint32_t> cig;
  std::vector<char> md;
};
// All jobs of a call, re-submitting the few whose CIGAR or MD did not fit the first, small, per-job room.  Caller holds c->mu and
// has set the device.
int run_jobs(bpsw_ctx* c, const SwScoring& sc, const bpsw_opt_t* opt, int flavour, const BnsView& bns, const std::vector<int32_t>& read_len,
             const std::vector<int64_t>& read_off, const uint8_t* read_pool, size_t read_pool_bytes,
             const std::vector<bpsw_alnreg_t>& regs, JobResults* res);

// memMarkPrimarySe: sorts `a` and fills sub / sub_n / secondary / hash
void mark_primary(const bpsw_opt_t& o, const bpsw_tail_opt_t& t, std::vector<bpsw_alnreg_t>& a, int64_t id);

struct Aln {  // a mem_aln_t under construction
  bpsw_aln_t a;
  const uint32_t* cigar = nullptr;  // a.n_cigar words
  const char* md = nullptr;         // a.md_len bytes
};
// the mem_aln_t of memRegToAln: kernel result + the fields that need no sequence (ar or jr null: the unmapped record)
Aln make_aln(const bpsw_opt_t& o, const bpsw_tail_opt_t& t, const bpsw_alnreg_t* ar, const JobResult* jr, const JobResults& R);

// The text of a call is written straight into the caller's buffer.  Past the capacity it only counts, so that *out_needed comes out right.
struct Text {
  char* buf;
  size_t cap, n = 0;
  Text(char* b, size_t c) : buf(b), cap(b ? c : 0) {}
  size_t size() const { return n; }
  char* grow(size_t len) {  // len more bytes, to be written by the caller; nullptr when they do not fit (they still count)
    char* p = n + len <= cap ? buf + n : nullptr;
    n += len;
    return p;
  }
  void push_back(char c) { if (n < cap) buf[n] = c; ++n; }
  void append(const char* p, size_t len) { char* d = grow(len); if (d) memcpy(d, p, len); }
  Text& operator+=(const char* z) { append(z, strlen(z)); return *this; }
  Text& operator+=(const std::string& z) { append(z.data(), z.size()); return *this; }
};

// memAlnToSAM: line `which` of a read's `list`; mate_in null: a single-end line
void aln_to_sam(const BnsView& bns, int flavour, Text& s, const char* name, size_t name_len, int l_seq, const uint8_t* seq,
                const uint8_t* qual, const Aln* list, const size_t n_list, int which, const Aln* mate_in, const char* rg_id);

}  // namespace bpsw
