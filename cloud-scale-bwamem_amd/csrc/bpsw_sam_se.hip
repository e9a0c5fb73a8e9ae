// bpsw_sam_se.hip -- the single-end worker2 behind the C ABI: bpsw_sam_se_batch, bpsw_align_se_batch; the SAM text written on the
// device (BPSW_SAM_TEXT_DEVICE), for both modes; worker1 in front of a tail (worker1_lists), for both modes.
//
// bpsw_sam_se_batch is sam_batch (bpsw_tail.cpp, bpsw_tail_internal.h) on a bpsw_se_reads_t: singleEndBwaMemWorker2
// (worker2/BWAMemWorker2.scala:49-58 == native/bwamem.c:1052-1056) for a batch, with the selection and the line rules of
// mem_reg2sam_se that the paired tail's single-end fallback uses.  What this file adds is the choice of who writes the text.
//
// With BPSW_SAM_TEXT_DEVICE the entries here and in bpsw_sam_pe.hip hand sam_batch text_on_device: two kernels over
// bpsw_sam_core.h, the byte definition of a line (in a pair every line names its mate):
//   sam_len_kernel    one line per lane: the line's number of bytes; the host sums them to line offsets, per-read out_off and
//                     the total (a total past text_cap ends the call there);
//   sam_write_kernel  one line per lane: the line's bytes at its offset in one device block, which comes back with one copy.
// A line depends on its read's lines (the SA:Z list) and, in a pair, on the first line of the other read; it reads both from the table.  Into the kernels go, as one
// staged block, the line table built on the host from make_aln's results (fixed-size records, each line's CIGAR words and MD
// bytes), the read records with the base, quality and name pools, the contig names and the read-group ID.  Building and staging that
// block is stage_lines, which the BAM writer (bam_on_device, bpsw_bam.hip) calls too; align_se is bpsw_align_se_batch's body with the
// tail it ends in as an argument, so that bpsw_align_bam_se_batch is the same body with the other writer.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "bpsw_tail_internal.h"
#include "bpsw_sam_core.h"

using namespace bpsw;
namespace sc = bpsw::samcore;

namespace {

__global__ __launch_bounds__(64) void sam_len_kernel(sc::SamBatch B, int n_lines, int32_t* __restrict__ len) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  len[i] = (int32_t)sc::sam_line_len(B, i);
}

// line i goes to text[line_off[i] .. line_off[i + 1]); status: the OR of every line's sam_line_write status
__global__ __launch_bounds__(64) void sam_write_kernel(sc::SamBatch B, int n_lines, const long long* __restrict__ line_off, char* text,
                                                       int* status) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  const long long at = line_off[i], len = line_off[i + 1] - at;
  int st = 0;
  sc::sam_line_write(text + at, text + at + len, B, i, len, &st);
  if (st) atomicOr(status, st);
}

thread_local double t_last[6] = {0., 0., 0., 0., 0., 0.};

}  // namespace

int bpsw::stage_lines(bpsw_ctx* c, const std::string& w, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& sl,
                      StageIn* staged, sc::SamBatch* batch) {
  const std::vector<Aln>& aa = sl.aa;
  const std::vector<int32_t>& line_read = sl.line_read;
  const std::vector<int32_t>& read_first = sl.read_first;
  const Aln* mate = sl.mate.empty() ? nullptr : sl.mate.data();
  const JobResults& R = *sl.R;
  const int n = g.n, n_lines = (int)aa.size(), n_names = g.n >> g.name_shift;
  StageIn& in = *staged;
  // ---- the line table -------------------------------------------------------------------------------------------------------
  std::vector<sc::SamLine> lines((size_t)n_lines);
  for (int i = 0; i < n_lines; ++i) {
    const Aln& x = aa[(size_t)i];
    sc::SamLine& L = lines[(size_t)i];
    memset(&L, 0, sizeof L);
    const int r = line_read[(size_t)i];
    L.pos = x.a.pos;
    L.cig_at = x.a.n_cigar > 0 ? (long long)(x.cigar - R.cig.data()) : 0;
    L.md_at = x.a.md_len > 0 ? (long long)(x.md - R.md.data()) : 0;
    L.read = r; L.first = read_first[(size_t)r]; L.n_list = read_first[(size_t)r + 1] - read_first[(size_t)r];
    L.rid = x.a.rid; L.flag = x.a.flag; L.is_rev = x.a.is_rev; L.mapq = x.a.mapq; L.NM = x.a.NM; L.n_cigar = x.a.n_cigar;
    L.md_len = x.a.md_len; L.score = x.a.score; L.sub = x.a.sub;
    if (mate) L.mate = read_first[(size_t)(r ^ 1)] + 1;
  }
  if (mate) {  // a line finds its mate as the first line of the other read: what it reads of it must be what the tail would hand over
    for (int r = 0; r < n; ++r) {
      const Aln& m = mate[r];
      const Aln& f = aa[(size_t)read_first[(size_t)(r ^ 1)]];
      const bool same_cigar = m.a.n_cigar == f.a.n_cigar && (m.a.n_cigar <= 0 || m.cigar == f.cigar || !memcmp(m.cigar, f.cigar, 4 * (size_t)m.a.n_cigar));
      if (m.a.rid != f.a.rid || m.a.pos != f.a.pos || m.a.is_rev != f.a.is_rev || !same_cigar)
        return fail(BPSW_ERR_DEVICE, w + ": a read's mate record is not the first line of the other read");
    }
  }
  // the reads' bytes: the covering span of the base pool (and of the quality pool, same offsets), the names' span
  long long lo = (long long)g.read_pool_bytes, hi = 0;
  for (int r = 0; r < n; ++r) { lo = std::min<long long>(lo, g.read_off[r]); hi = std::max<long long>(hi, g.read_off[r] + g.read_len[r]); }
  const long long name_lo = g.name_off[0], name_hi = g.name_off[n_names];
  std::vector<sc::SamRead> reads((size_t)n);
  for (int r = 0; r < n; ++r) {
    const int k = r >> g.name_shift;
    reads[(size_t)r].seq_at = g.read_off[r] - lo;
    reads[(size_t)r].name_at = g.name_off[k] - name_lo;
    reads[(size_t)r].len = g.read_len[r];
    reads[(size_t)r].name_len = (int32_t)(g.name_off[k + 1] - g.name_off[k]);
  }
  std::vector<int32_t> ctg_at(bns.name.size() + 1, 0);
  std::vector<char> ctg_names;
  for (size_t k = 0; k < bns.name.size(); ++k) {
    ctg_names.insert(ctg_names.end(), bns.name[k].begin(), bns.name[k].end());
    ctg_at[k + 1] = (int32_t)ctg_names.size();
  }
  const size_t rg_len = t.rg_id[0] ? strnlen(t.rg_id, sizeof t.rg_id) : 0;

  const int i_lines = in.add(lines.data(), sizeof(sc::SamLine) * (size_t)n_lines), i_reads = in.add(reads.data(), sizeof(sc::SamRead) * (size_t)n);
  const int i_cig = in.add(R.cig.data(), 4 * R.cig.size()), i_md = in.add(R.md.data(), R.md.size());
  const int i_seq = in.add(g.read_pool + lo, (size_t)(hi - lo));
  const int i_qual = g.qual_pool ? in.add(g.qual_pool + lo, (size_t)(hi - lo)) : -1;
  const int i_names = in.add(g.name_pool + name_lo, (size_t)(name_hi - name_lo));
  const int i_cat = in.add(ctg_at.data(), 4 * ctg_at.size()), i_cnm = in.add(ctg_names.data(), ctg_names.size());
  const int i_rg = in.add(t.rg_id, rg_len);
  HIP_TRY(in.stage(c->h_stage_in, c->d_sw_in, c->stream));
  sc::SamBatch& B = *batch;
  B.lines = in.dev<sc::SamLine>(i_lines); B.reads = in.dev<sc::SamRead>(i_reads);
  B.cig = in.dev<uint32_t>(i_cig); B.md = in.dev<char>(i_md);
  B.seq = in.dev<uint8_t>(i_seq); B.qual = i_qual >= 0 ? in.dev<uint8_t>(i_qual) : nullptr;
  B.names = in.dev<char>(i_names);
  B.ctg_at = in.dev<int32_t>(i_cat); B.ctg_names = in.dev<char>(i_cnm);
  B.rg = in.dev<char>(i_rg);
  B.n_ctg = (int32_t)bns.name.size(); B.rg_len = (int32_t)rg_len; B.flavour = t.flavour;
  return BPSW_OK;
}

int bpsw::text_on_device(bpsw_ctx* c, const char* who, const BnsView& bns, const bpsw_tail_opt_t& t, const TextReads& g, const SamLines& sl,
                         char* out_text, size_t text_cap, int64_t* out_off, size_t* total_out, double times[4]) {
  const std::vector<int32_t>& read_first = sl.read_first;
  const int n = g.n, n_lines = (int)sl.aa.size();
  const std::string w(who);
  const double t0 = wall_ms();
  StageOut lens;
  const int r_len = lens.add(4 * (size_t)n_lines);
  HIP_TRY(lens.reserve(c->h_stage_out, c->d_sw_out));
  StageIn in;
  sc::SamBatch B;
  const int rc = stage_lines(c, w, bns, t, g, sl, &in, &B);
  if (rc != BPSW_OK) return rc;
  const dim3 grid((unsigned)((n_lines + 63) / 64));
  const double t1 = wall_ms();
  // ---- lengths ---------------------------------------------------------------------------------------------------------------
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  hipLaunchKernelGGL(sam_len_kernel, grid, dim3(64), 0, c->stream, B, n_lines, lens.dev<int32_t>(r_len));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(lens.fetch(c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms_len = 0.f;
  (void)hipEventElapsedTime(&ms_len, c->ev[6], c->ev[7]);
  std::vector<long long> line_off((size_t)n_lines + 1, 0);
  const int32_t* hl = lens.host<int32_t>(r_len);
  for (int i = 0; i < n_lines; ++i) {
    if (hl[i] < 1) return fail(BPSW_ERR_DEVICE, w + ": a line came back with no length");
    line_off[(size_t)i + 1] = line_off[(size_t)i] + hl[i];
  }
  for (int r = 0; r <= n; ++r) out_off[r] = (int64_t)line_off[(size_t)read_first[(size_t)r]];
  const size_t total = (size_t)line_off[(size_t)n_lines];
  *total_out = total;
  times[0] = ms_len; times[1] = 0.; times[2] = t1 - t0;
  const double t2 = wall_ms();
  if (!out_text || total > text_cap) { times[3] = t2 - t1; return BPSW_OK; }  // (the caller reports the capacity)
  // ---- text ------------------------------------------------------------------------------------------------------------------
  // (the pinned input block is free again: its copy has been waited for; the line table stays where it is on the device)
  StageIn io;
  const int i_off = io.add(line_off.data(), 8 * ((size_t)n_lines + 1));
  StageOut txt;
  const int r_text = txt.add(total), r_status = txt.add(16);
  HIP_TRY(txt.reserve(c->h_stage_out, c->d_gl_z));  // (the backtrack scratch of run_jobs: free by now)
  HIP_TRY(io.stage(c->h_stage_in, c->d_sw_out, c->stream));  // (the lengths have come back)
  HIP_TRY(hipMemsetAsync(txt.dev<int>(r_status), 0, 16, c->stream));
  HIP_TRY(hipEventRecord(c->ev[6], c->stream));
  hipLaunchKernelGGL(sam_write_kernel, grid, dim3(64), 0, c->stream, B, n_lines, io.dev<long long>(i_off), txt.dev<char>(r_text),
                     txt.dev<int>(r_status));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[7], c->stream));
  HIP_TRY(txt.fetch(c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms_write = 0.f;
  (void)hipEventElapsedTime(&ms_write, c->ev[6], c->ev[7]);
  times[1] = ms_write;
  if (*txt.host<int>(r_status)) return fail(BPSW_ERR_DEVICE, w + ": a line's bytes differ in number from its length (sam_line_write's status)");
  memcpy(out_text, txt.host<char>(r_text), total);
  times[3] = wall_ms() - t1;
  return BPSW_OK;
}

int bpsw::worker1_lists(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const TextReads& g, int zdrop_mode, int w1_flags,
                        std::vector<int32_t>* cnt, std::vector<bpsw_alnreg_t>* regs) {
  bpsw_reads_t rd;
  rd.n_reads = g.n; rd.read_len = g.read_len; rd.read_off = g.read_off; rd.read_pool = g.read_pool; rd.read_pool_bytes = g.read_pool_bytes;
  cnt->assign((size_t)g.n, 0);
  regs->resize((size_t)(4 * (int64_t)g.n + 64));
  int64_t total = 0;
  auto run = [&]() {
    return bpsw_worker1_batch(c, opt, sopt, &rd, zdrop_mode, w1_flags | BPSW_C2A_SORT_DEDUP, cnt->data(), regs->data(), (int64_t)regs->size(), &total);
  };
  int rc = run();
  if (rc == BPSW_ERR_CAPACITY && total > (int64_t)regs->size()) {
    regs->resize((size_t)total);
    rc = run();
  }
  return rc;
}

int bpsw::align_se(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g,
                   int zdrop_mode, int w1_flags, int flags, SeTail tail, char* out_text, size_t text_cap, int64_t* out_off, size_t* out_needed) {
  if (!c || !opt || !sopt || !topt || !g || !out_off) return fail(BPSW_ERR_ARG, "align_se: null argument");
  const int n = g->n_reads;
  if (n < 0) return fail(BPSW_ERR_ARG, "align_se: negative number of reads");
  if (n == 0) { out_off[0] = 0; if (out_needed) *out_needed = 0; return BPSW_OK; }
  size_t none = 0;
  int rc = se_check("align_se", g, false, &none);
  if (rc != BPSW_OK) return rc;
  // ---- worker1: reads -> region lists (FastMap.scala:624) ---------------------------------------------------------------------
  const double t0 = wall_ms();
  std::vector<int32_t> cnt;
  std::vector<bpsw_alnreg_t> regs;
  rc = worker1_lists(c, opt, sopt, text_reads(g), zdrop_mode, w1_flags, &cnt, &regs);
  if (rc != BPSW_OK) return rc;
  // ---- worker2: the lists -> text (FastMap.scala:625) ---------------------------------------------------------------------------
  const double t1 = wall_ms();
  bpsw_se_reads_t s = *g;
  s.reg_cnt = cnt.data();
  s.regs = regs.data();
  rc = tail(c, opt, topt, &s, flags, out_text, text_cap, out_off, out_needed, nullptr);
  t_last[4] = t1 - t0; t_last[5] = wall_ms() - t1;
  return rc;
}

extern "C" {

int bpsw_sam_se_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_se_reads_t* g, int flags,
                      char* out_text, size_t text_cap, int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs) {
  if (c && topt && g && out_off && (flags & ~BPSW_SAM_TEXT_DEVICE)) return fail(BPSW_ERR_ARG, "sam_se: unknown flag");  // (after the null checks)
  SamCall m;
  m.on_device = (flags & BPSW_SAM_TEXT_DEVICE) ? text_on_device : nullptr;
  m.times = t_last; m.n_times = 6;
  return sam_batch(c, opt, topt, g, nullptr, m, out_text, text_cap, out_off, out_needed, out_regs);
}

int bpsw_align_se_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt,
                        const bpsw_se_reads_t* g, int zdrop_mode, int w1_flags, int flags, char* out_text, size_t text_cap, int64_t* out_off,
                        size_t* out_needed) {
  return align_se(c, opt, sopt, topt, g, zdrop_mode, w1_flags, flags, bpsw_sam_se_batch, out_text, text_cap, out_off, out_needed);
}

void bpsw_last_sam_se_times(double ms[6]) {
  if (ms) memcpy(ms, t_last, sizeof t_last);
}

}  // extern "C"
