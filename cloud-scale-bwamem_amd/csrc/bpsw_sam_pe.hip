// bpsw_sam_pe.hip -- the paired mode behind the C ABI with a flags argument: bpsw_sam_pe_batch_ex (the paired tail, its text
// optionally written on the device) and bpsw_align_pe_batch (paired reads to SAM text in one call).
//
// The tail exists once, in bpsw_tail.cpp (bpsw_tail_internal.h): sam_batch is the body of bpsw_sam_pe_batch, of bpsw_sam_se_batch
// and of bpsw_sam_pe_batch_ex.  With BPSW_SAM_TEXT_DEVICE the entry here hands it text_on_device (bpsw_sam_se.hip): sam_len_kernel
// and sam_write_kernel over bpsw_sam_core.h, every line naming the first line of its pair's other read as its mate.
//
// bpsw_align_pe_batch is mem_process_seqs under MEM_F_PE (native/bwamem.c:1064-1083 == FastMap.scala:262-307, :352-395) for a
// batch: bpsw_worker1_batch on the 2n reads, the insert-size statistics (given, or bpsw_pe_stat over this batch's lists), the
// rescue half of bpsw_worker2_batch (pe_rescue), then the tail above.  worker1 with its lists and their capacity retry is
// worker1_lists (bpsw_sam_se.hip), as for single-end reads.  Its body is align_pe, with the tail it ends in as an argument:
// bpsw_align_bam_pe_batch (bpsw_bam.hip) is the same body with the BAM tail.
#include <string.h>

#include <vector>

#include "bpsw_tail_internal.h"

using namespace bpsw;

namespace {

// sam_len_kernel, sam_write_kernel, tables, round trip | worker1, statistics, rescue, tail
thread_local double t_last[8] = {0., 0., 0., 0., 0., 0., 0., 0.};

}  // namespace

int bpsw::align_pe(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g,
                   const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, PeTail tail, char* out_text, size_t text_cap,
                   int64_t* out_off, size_t* out_needed, bpsw_pestat_t* out_pes) {
  if (!c || !opt || !sopt || !topt || !g || !out_off) return fail(BPSW_ERR_ARG, "align_pe: null argument");
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
  if (!g->read_len || !g->read_off || !g->read_pool || !g->name_off || !g->name_pool) return fail(BPSW_ERR_ARG, "align_pe: null group arrays");
  size_t none = 0;
  int rc = check_reads("align_pe", text_reads(g), nullptr, false, &none);
  if (rc != BPSW_OK) return rc;
  // ---- worker1: the 2n reads -> region lists ------------------------------------------------------------------------------------
  const double t0 = wall_ms();
  std::vector<int32_t> cnt;
  std::vector<bpsw_alnreg_t> regs;
  rc = worker1_lists(c, opt, sopt, text_reads(g), zdrop_mode, w1_flags, &cnt, &regs);
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
  int64_t total = 0;
  rc = pe_rescue(c, "align_pe", opt, &p, rescue_mode, &cnt2, &regs2, &total);
  if (rc != BPSW_OK) return rc;
  const double t3 = wall_ms();
  p.reg_cnt = cnt2.data();
  p.regs = regs2.data();
  rc = tail(c, opt, topt, &p, flags, out_text, text_cap, out_off, out_needed, nullptr);
  t_last[4] = t1 - t0; t_last[5] = t2 - t1; t_last[6] = t3 - t2; t_last[7] = wall_ms() - t3;
  return rc;
}

extern "C" {

int bpsw_sam_pe_batch_ex(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g, int flags, char* out_text,
                         size_t text_cap, int64_t* out_off, size_t* out_needed, bpsw_alnreg_t* out_regs) {
  if (flags & ~BPSW_SAM_TEXT_DEVICE) return fail(BPSW_ERR_ARG, "sam_pe: unknown flag");
  memset(t_last, 0, 4 * sizeof(double));
  SamCall m;
  m.paired = true;
  if (flags & BPSW_SAM_TEXT_DEVICE) { m.on_device = text_on_device; m.times = t_last; m.n_times = 4; }
  return sam_batch(c, opt, topt, nullptr, g, m, out_text, text_cap, out_off, out_needed, out_regs);
}

int bpsw_align_pe_batch(bpsw_ctx_t* c, const bpsw_opt_t* opt, const bpsw_seed_opt_t* sopt, const bpsw_tail_opt_t* topt, const bpsw_pairs_t* g,
                        const bpsw_pestat_t* pes0, int zdrop_mode, int w1_flags, int rescue_mode, int flags, char* out_text, size_t text_cap,
                        int64_t* out_off, size_t* out_needed, bpsw_pestat_t* out_pes) {
  if (c && opt && sopt && topt && g && out_off && (flags & ~BPSW_SAM_TEXT_DEVICE)) return fail(BPSW_ERR_ARG, "align_pe: unknown flag");  // (after the null checks)
  return align_pe(c, opt, sopt, topt, g, pes0, zdrop_mode, w1_flags, rescue_mode, flags, bpsw_sam_pe_batch_ex, out_text, text_cap, out_off, out_needed,
                  out_pes);
}

void bpsw_last_sam_pe_times(double ms[8]) {
  if (ms) memcpy(ms, t_last, sizeof t_last);
}

}  // extern "C"
