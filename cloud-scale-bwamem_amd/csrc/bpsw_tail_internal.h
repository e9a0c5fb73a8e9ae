// bpsw_tail_internal.h -- worker2's tail as its entries share it: the contig table's snapshot, memMarkPrimarySe, the reg2aln launches
// with their resubmission, the mem_aln_t of a job, the SAM line on the calling thread, reads with names as one view (TextReads) with
// the one check of a read against its pool, the line list of a batch (SamLines: se_lines / pe_lines), sam_batch -- the one body of
// bpsw_sam_se_batch, bpsw_sam_pe_batch and bpsw_sam_pe_batch_ex -- and worker2's prepare-and-rescue half.  Defined in bpsw_tail.cpp,
// which compiles and links without any .hip object; text_on_device and worker1_lists are bpsw_sam_se.hip's, and the entries there and
// in bpsw_sam_pe.hip hand the former to sam_batch as a pointer.  Not installed.
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


// ---- reads with names: what both modes print from -------------------------------------------------------------------------------------
struct TextReads {  // read r has name r >> name_shift (0: a name per read; 1: a name per pair)
  int n = 0, name_shift = 0;
  const int32_t* read_len = nullptr;
  const int64_t* read_off = nullptr;
  const uint8_t* read_pool = nullptr;
  const uint8_t* qual_pool = nullptr;
  size_t read_pool_bytes = 0;
  const int64_t* name_off = nullptr;
  const char* name_pool = nullptr;
};
template <class Reads>  // bpsw_se_reads_t and bpsw_pairs_t name these fields alike
inline TextReads text_reads(const Reads* g, int n, int name_shift) {
  TextReads v;
  v.n = n; v.name_shift = name_shift;
  v.read_len = g->read_len; v.read_off = g->read_off; v.read_pool = g->read_pool; v.qual_pool = g->qual_pool;
  v.read_pool_bytes = g->read_pool_bytes; v.name_off = g->name_off; v.name_pool = g->name_pool;
  return v;
}
inline TextReads text_reads(const bpsw_se_reads_t* g) { return text_reads(g, g->n_reads, 0); }
inline TextReads text_reads(const bpsw_pairs_t* g) { return text_reads(g, 2 * g->group_size, 1); }
// Per read, in this order: a negative region count (reg_cnt given), a read outside its pool or empty, and (names_ascend: a name per
// read) name offsets that do not ascend.  *n_regs: the sum of reg_cnt.  The arrays themselves are the caller's to check for null.
int check_reads(const char* who, const TextReads& g, const int32_t* reg_cnt, bool names_ascend, size_t* n_regs);
// what a mode checks of its batch before anything runs (the batch is not empty)
int se_check(const char* who, const bpsw_se_reads_t* g, bool need_regs, size_t* n_regs);
int pe_check(const char* who, const bpsw_pairs_t* g, size_t* n_regs);

// ---- the tail in pieces: sam_batch is a mode's check, se_lines or pe_lines, the text, finish -------------------------------------------
struct SamLines {  // the lines of every read of a batch, in read order
  std::vector<Aln> aa;                // the lines
  std::vector<int32_t> line_read;     // the read of each
  std::vector<int32_t> read_first;    // n + 1: read r has lines aa[read_first[r] .. read_first[r + 1])
  std::vector<Aln> mate;              // paired: per read the record its lines are printed against (memAlnToSAM's m: h[1 - i]); else empty
  const JobResults* R = nullptr;      // the CIGAR and MD pools the lines point into (the calling thread's, valid until its next tail call)
  const std::vector<bpsw_alnreg_t>* regs = nullptr;  // the n lists as the tail leaves them (out_regs)
  double t_plan = 0., t_dev = 0., t_emit = 0.;
};
// The text of `L` through sam_len_kernel and sam_write_kernel (bpsw_sam_se.hip).  With mates the kernels read the first line of the
// pair's other read instead of L.mate, so the five fields memAlnToSAM reads of a mate must agree between the two (checked there;
// BPSW_ERR_DEVICE if not).  times[4]: sam_len_kernel, sam_write_kernel, building and staging the tables, the round trip (ms).  Fills
// out_off (n + 1) and *total_out; a total past text_cap ends the call after the lengths.  Caller holds c->mu.
typedef int (*TextOnDevice)(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& L,
                            char* out_text, size_t text_cap, int64_t* out_off, size_t* total_out, double times[4]);
int text_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& L,
                   char* out_text, size_t text_cap, int64_t* out_off, size_t* total_out, double times[4]);
struct SamCall {  // what an entry hands to sam_batch besides its arguments
  bool paired = false;                // the batch is `pe` (else `se`)
  TextOnDevice on_device = nullptr;   // who writes the text; null: the calling thread (aln_to_sam)
  double* times = nullptr;            // null, or the entry's n_times times: zeroed once the checks are passed; on_device's times[4]
  int n_times = 0;
};
// The one body of the tail's entries: null checks, scoring, the empty batch, the mode's checks, the context and the contig table, the
// line list, the text, then out_regs, the host times, *out_needed and the capacity verdict.
int sam_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* se, const bpsw_pairs_t* pe,
              const SamCall& m, char* out_text, size_t text_cap, int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs);
// worker2's first half: anchors, their windows, bpsw_matesw_group with its capacity retry; the lists after the rescue
int pe_rescue(bpsw_ctx_t* c, const char* who, const bpsw_opt_t* opt, const bpsw_pairs_t* g, int rescue_mode, std::vector<int32_t>* out_cnt,
              std::vector<bpsw_alnreg_t>* out_regs, int64_t* out_total);
// worker1 in front of a tail (bpsw_sam_se.hip): bpsw_worker1_batch with BPSW_C2A_SORT_DEDUP on the reads of `g`, its lists sized
// 4 n + 64 regions and, when they do not fit, once more at the size it names
int worker1_lists(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const TextReads& g, int zdrop_mode, int w1_flags,
                  std::vector<int32_t>* cnt, std::vector<bpsw_alnreg_t>* regs);

// ---- what the BAM entries (bpsw_bam.hip) share with the text's ----------------------------------------------------------------------
// The first half of text_on_device (bpsw_sam_se.hip): the line table of `L` with its mate assertion, the read records and pools, the
// contig names and the read group, as one block staged on c->stream; *B points into it on the device.
namespace samcore { struct SamBatch; }
int stage_lines(bpsw_ctx* c, const std::string& who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& L,
                StageIn* staged, samcore::SamBatch* B);
// bam_on_device (bpsw_bam.hip), the second writer: the records of `L` through bam_len_kernel and bam_write_kernel, their stream cut into
// BGZF blocks by bgzf_frame_kernel.  A TextOnDevice: *total_out is the framed size, out_off gets the records' offsets in the
// unframed stream (the entries keep them to themselves), times[5]: the three kernels, the tables, the round trip.
int bam_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& L,
                  char* out, size_t cap, int64_t* out_off, size_t* total_out, double times[5]);
// The bodies of bpsw_align_se_batch (bpsw_sam_se.hip) and bpsw_align_pe_batch (bpsw_sam_pe.hip) with the tail they end in as an
// argument: bpsw_sam_se_batch / bpsw_sam_pe_batch_ex for the text, the BAM tails for bpsw_align_bam_*.
typedef int (*SeTail)(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g, int flags, char* out,
                      size_t cap, int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs);
typedef int (*PeTail)(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, int flags, char* out, size_t cap,
                      int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs);
int align_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g,
             int zdrop_mode, int w1_flags, int flags, SeTail tail, char* out_text, size_t text_cap, int64_t* out_off, size_t* out_needed);
int align_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g,
             const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, PeTail tail, char* out_text, size_t text_cap,
             int64_t* out_off, size_t* out_needed, bpsw_pestat_t* out_pes);

}  // namespace bpsw
