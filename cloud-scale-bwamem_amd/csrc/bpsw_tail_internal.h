// bpsw_tail_internal.h -- the pieces of worker2's tail (bpsw_tail.cpp) that the single-end tail (bpsw_sam_se.hip) and the paired
// entries with a flags argument (bpsw_sam_pe.hip) use as they are: the contig table's snapshot, memMarkPrimarySe, the reg2aln
// launches with their resubmission, the mem_aln_t of a job, the SAM line on the calling thread, the paired tail in its pieces
// (checks, plan + jobs + line lists, printing, the end) and worker2's prepare-and-rescue half.  Defined in bpsw_tail.cpp, except
// text_on_device (bpsw_sam_se.hip, beside its kernels); not installed.
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


// ---- the paired tail in pieces: bpsw_sam_pe_batch is pe_check, pe_lines, pe_print, pe_finish ----------------------------------------
struct PeLines {  // what pe_lines leaves: the lines of every read of the group, in read order (2k + i)
  std::vector<Aln> aa;                // the lines
  std::vector<int32_t> line_read;     // the read of each
  std::vector<int32_t> read_first;    // 2 G + 1: read r has lines aa[read_first[r] .. read_first[r + 1])
  std::vector<Aln> mate;              // per read: the record its lines are printed against (memAlnToSAM's m: h[1 - i])
  const JobResults* R = nullptr;      // the CIGAR and MD pools the lines point into (the calling thread's, valid until its next tail call)
  const std::vector<bpsw_alnreg_t>* regs = nullptr;  // 2 G lists as the tail leaves them (out_regs)
  double t_plan = 0., t_dev = 0., t_emit = 0.;
};
int pe_check(const char* who, const bpsw_pairs_t* g, size_t* n_regs);
// mark-primary, memPair and the single-end fallback, the jobs through run_jobs, then every read's lines.  Caller holds c->mu.
int pe_lines(bpsw_ctx* c, const SwScoring& sc, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, const BnsView& bns,
             PeLines* out);
// the text on the calling thread; returns its size (counted past text_cap, never written there); fills out_off (2 G + 1)
size_t pe_print(const PeLines& L, const BnsView& bns, const bpsw_tail_opt_t& t, const bpsw_pairs_t* g, char* out_text, size_t text_cap,
                int64_t* out_off);
// out_regs, the host times, *out_needed and the capacity verdict
int pe_finish(bpsw_ctx* c, const PeLines& L, const bpsw_pairs_t* g, const char* out_text, size_t text_cap, size_t total, size_t* out_needed,
              bpsw_alnreg_t* out_regs);
// worker2's first half: anchors, their windows, bpsw_matesw_group with its capacity retry; the lists after the rescue
int pe_rescue(bpsw_ctx_t* c, const char* who, const bpsw_opt_t* opt, const bpsw_pairs_t* g, int rescue_mode, std::vector<int32_t>* out_cnt,
              std::vector<bpsw_alnreg_t>* out_regs, int64_t* out_total);

// ---- the text on the device (bpsw_sam_se.hip) ----------------------------------------------------------------------------------------
struct TextReads {  // reads with names: read r has name r >> name_shift (0: a name per read; 1: a name per pair)
  int n = 0, name_shift = 0;
  const int32_t* read_len = nullptr;
  const int64_t* read_off = nullptr;
  const uint8_t* read_pool = nullptr;
  const uint8_t* qual_pool = nullptr;
  size_t read_pool_bytes = 0;
  const int64_t* name_off = nullptr;
  const char* name_pool = nullptr;
};
// The text of the lines in `aa` (per read: aa[read_first[r] .. read_first[r + 1])) through sam_len_kernel and sam_write_kernel.
// mate: null, or per read the record its lines are printed against -- the kernels read the first line of the pair's other read
// instead, so the five fields memAlnToSAM reads of a mate must agree between the two (checked here; BPSW_ERR_DEVICE if not).
// times[4]: sam_len_kernel, sam_write_kernel, building and staging the tables, the round trip (ms).  Caller holds c->mu.
int text_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const std::vector<Aln>& aa,
                   const std::vector<int32_t>& line_read, const std::vector<int32_t>& read_first, const Aln* mate, const JobResults& R,
                   char* out_text, size_t text_cap, int64_t* out_off, size_t* total_out, double times[4]);

}  // namespace bpsw
