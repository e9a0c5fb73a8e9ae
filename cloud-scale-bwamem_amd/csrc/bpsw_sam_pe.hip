// bpsw_sam_pe.hip -- the paired mode behind the C ABI with a flags argument: bpsw_sam_pe_batch_ex (the paired tail, its text
// optionally written on the device) and bpsw_align_pe_batch (paired reads to SAM text in one call).
//
// The pairing rules exist once, in bpsw_tail.cpp (bpsw_tail_internal.h): pe_check, pe_lines (mark-primary, memPair, the
// single-end fallback, the reg2aln jobs, every read's lines), pe_print (the text on the calling thread) and pe_finish.
// bpsw_sam_pe_batch is those four; with BPSW_SAM_TEXT_DEVICE the third is text_on_device (bpsw_sam_se.hip): sam_len_kernel and
// sam_write_kernel over bpsw_sam_core.h, every line naming the first line of its pair's other read as its mate.
//
// bpsw_align_pe_batch is mem_process_seqs under MEM_F_PE (native/bwamem.c:1064-1083 == FastMap.scala:262-307, :352-395) for a
// batch: bpsw_worker1_batch on the 2n reads, the insert-size statistics (given, or bpsw_pe_stat over this batch's lists), the
// rescue half of bpsw_worker2_batch (pe_rescue), then the tail above.
#include <string.h>

#include <vector>

#include "bpsw_tail_internal.h"

using namespace bpsw;

namespace {

// sam_len_kernel, sam_write_kernel, tables, round trip | worker1, statistics, rescue, tail
thread_local double t_last[8] = {0., 0., 0., 0., 0., 0., 0., 0.};

}  // namespace

extern "C" {

int bpsw_sam_pe_batch_ex(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, int flags, char* out_text,
                         size_t text_cap, int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs) {
  if (flags & ~BPSW_SAM_TEXT_DEVICE) return fail(BPSW_ERR_ARG, "sam_pe: unknown flag");
  memset(t_last, 0, 4 * sizeof(double));
  if (!(flags & BPSW_SAM_TEXT_DEVICE)) return bpsw_sam_pe_batch(c, opt, topt, g, out_text, text_cap, out_off, out_needed, out_regs);
  if (!c || !topt || !g || !out_off) return fail(BPSW_ERR_ARG, "sam_pe: null argument");
  SwScoring sw;
  int rc = make_scoring("tail", opt, 0, 1, &sw);
  if (rc != BPSW_OK) return rc;
  const int G = g->group_size;
  if (G < 0) return fail(BPSW_ERR_ARG, "sam_pe: negative group size");
  if (G == 0) { out_off[0] = 0; if (out_needed) *out_needed = 0; return BPSW_OK; }
  if (G > (1 << 29)) return fail(BPSW_ERR_LIMIT, "sam_pe: group too large for the device text");
  size_t n_regs = 0;
  rc = pe_check("sam_pe", g, &n_regs);
  if (rc != BPSW_OK) return rc;
  ContextEntry entry(c);
  if (entry.rc != BPSW_OK) return entry.rc;
  BnsView bns;
  rc = snapshot_bns(c, &bns);
  if (rc != BPSW_OK) return rc;
  static thread_local PeLines lines;
  rc = pe_lines(c, sw, opt, topt, g, bns, &lines);
  if (rc != BPSW_OK) return rc;
  TextReads tr;
  tr.n = 2 * G; tr.name_shift = 1;
  tr.read_len = g->read_len; tr.read_off = g->read_off; tr.read_pool = g->read_pool; tr.qual_pool = g->qual_pool;
  tr.read_pool_bytes = g->read_pool_bytes; tr.name_off = g->name_off; tr.name_pool = g->name_pool;
  size_t total = 0;
  rc = text_on_device(c, "sam_pe", bns, *topt, tr, lines.aa, lines.line_read, lines.read_first, lines.mate.data(), *lines.R, out_text, text_cap,
                      out_off, &total, t_last);
  if (rc != BPSW_OK) return rc;
  return pe_finish(c, lines, g, out_text, text_cap, total, out_needed, out_regs);
}

int bpsw_align_pe_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g,
                        const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out_text, size_t text_cap,
                        int64_t* out_off, size_t* out_needed, bpsw_pestat_t* out_pes) {
  if (!c || !opt || !sopt || !topt || !g || !out_off) return fail(BPSW_ERR_ARG, "align_pe: null argument");
  if (flags & ~BPSW_SAM_TEXT_DEVICE) return fail(BPSW_ERR_ARG, "align_pe: unknown flag");
  const int G = g->group_size;
  if (G < 0) return fail(BPSW_ERR_ARG, "align_pe: negative group size");
  memset(t_last, 0, sizeof t_last);
  if (G == 0) {
    out_off[0] = 0;
    if (out_needed) *out_needed = 0;
    if (out_pes) {
      if (pes0) memcpy(out_pes, pes0, 4 * sizeof(bpsw_pestat_t));
      else bpsw_pe_stat(opt, topt, 0, 0, nullptr, nullptr, out_pes);
    }
    return BPSW_OK;
  }
  if (G > (1 << 29)) return fail(BPSW_ERR_LIMIT, "align_pe: group too large");
  const int n = 2 * G;
  if (!g->read_len || !g->read_off || !g->read_pool || !g->name_off || !g->name_pool) return fail(BPSW_ERR_ARG, "align_pe: null group arrays");
  for (int r = 0; r < n; ++r)
    if (g->read_len[r] < 1 || g->read_off[r] < 0 || (unsigned long long)(g->read_off[r] + g->read_len[r]) > g->read_pool_bytes)
      return fail(BPSW_ERR_ARG, "align_pe: read outside its pool (or empty)");
  // ---- worker1: the 2n reads -> region lists ------------------------------------------------------------------------------------
  const double t0 = wall_ms();
  bpsw_reads_t rd;
  rd.n_reads = n; rd.read_len = g->read_len; rd.read_off = g->read_off; rd.read_pool = g->read_pool; rd.read_pool_bytes = g->read_pool_bytes;
  std::vector<int32_t> cnt((size_t)n, 0);
  std::vector<bpsw_alnreg_t> regs((size_t)(4 * (int64_t)n + 64));
  int64_t total = 0;
  int rc = bpsw_worker1_batch(c, opt, sopt, &rd, zdrop_mode, w1_flags | BPSW_C2A_SORT_DEDUP, cnt.data(), regs.data(), (int64_t)regs.size(), &total);
  if (rc == BPSW_ERR_CAPACITY && total > (int64_t)regs.size()) {
    regs.resize((size_t)total);
    rc = bpsw_worker1_batch(c, opt, sopt, &rd, zdrop_mode, w1_flags | BPSW_C2A_SORT_DEDUP, cnt.data(), regs.data(), (int64_t)regs.size(), &total);
  }
  if (rc != BPSW_OK) return rc;
  // ---- the insert-size statistics: the driver's, or this batch's (mem_pestat) --------------------------------------------------------
  const double t1 = wall_ms();
  bpsw_pairs_t p = *g;
  p.reg_cnt = cnt.data();
  p.regs = regs.data();
  if (pes0) {
    memcpy(p.pes, pes0, sizeof p.pes);
  } else {
    rc = bpsw_pe_stat(opt, topt, (int64_t)bpsw_ref_length(c), G, cnt.data(), regs.data(), p.pes);
    if (rc != BPSW_OK) return rc;
  }
  if (out_pes) memcpy(out_pes, p.pes, sizeof p.pes);
  // ---- worker2: the rescue, then the tail --------------------------------------------------------------------------------------------
  const double t2 = wall_ms();
  std::vector<int32_t> cnt2;
  std::vector<bpsw_alnreg_t> regs2;
  rc = pe_rescue(c, "align_pe", opt, &p, rescue_mode, &cnt2, &regs2, &total);
  if (rc != BPSW_OK) return rc;
  const double t3 = wall_ms();
  p.reg_cnt = cnt2.data();
  p.regs = regs2.data();
  rc = bpsw_sam_pe_batch_ex(c, opt, topt, &p, flags, out_text, text_cap, out_off, out_needed, nullptr);
  t_last[4] = t1 - t0; t_last[5] = t2 - t1; t_last[6] = t3 - t2; t_last[7] = wall_ms() - t3;
  return rc;
}

void bpsw_last_sam_pe_times(double ms[8]) {
  if (ms) memcpy(ms, t_last, sizeof t_last);
}

}  // extern "C"
