// bpsw_rescue_core.h -- the rules of the mate rescue (mem_matesw, native/bwamem_pair.c:115-228 / MemSamPe.scala:1111-1238), each stated
// once: which regions of an end are anchors, which orientations of an anchor need no SW, how an orientation number decodes, what the
// length of a window is, and from those the plan of one pair against its initial lists.  Plain C++, no HIP, nothing from
// bpsw_internal.h: the boundary-1 host layer (bpsw_rescue.cpp: plan and replay), the JNI shim (bpsw_jni.cpp: which pairs of a mateSWJNI
// call it has to unmarshal at all) and worker2's prepare step (bpsw_tail.cpp: pe_rescue) all decide through this file, so that none of
// them can drift from what the library launches; tests/rescue_core_host runs it on the CPU under the sanitizers.  Regions are reached
// through a template parameter: any record with `rb` and `score` (bpsw_alnreg_t is 64 bytes, the shim's light record 16).
#pragma once
#include <stdint.h>

#include "bpsw.h"

namespace bpsw {

// native/bwamem_pair.c:27-34 (mem_infer_dir): orientation 0..3 of a pair of hits by their starts on the doubled reference, and their distance
inline int rescue_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t* dist) {
  const bool r1 = b1 >= l_pac, r2 = b2 >= l_pac;
  const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
  *dist = p2 > b1 ? p2 - b1 : b1 - p2;
  return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// orientation r: the mate is aligned reversed (native/bwamem_pair.c:177) / lies at the larger coordinate (:179)
inline bool rescue_is_rev(int r) { return (r >> 1) != (r & 1); }
inline bool rescue_is_larger(int r) { return !(r >> 1); }

// What decides which SW jobs a group needs, built once per call.  failed_mask bit r: pes[r].failed (an orientation without statistics
// is skipped for every anchor); scala_narrow: MemSamPe.scala:1137-1138 narrows the distance to Int.
struct RescueRules {
  int64_t l_pac;
  int32_t low[4], high[4];
  int failed_mask;
  bool scala_narrow;
  int32_t max_matesw, pen_unpaired;
};

inline RescueRules rescue_rules(const bpsw_opt_t& opt, const bpsw_pestat_t pes[4], int64_t l_pac, int mode) {
  RescueRules U = {l_pac, {}, {}, 0, mode == BPSW_RESCUE_SCALA, opt.max_matesw, opt.pen_unpaired};
  for (int r = 0; r < 4; ++r) { U.low[r] = pes[r].low; U.high[r] = pes[r].high; U.failed_mask |= (pes[r].failed ? 1 : 0) << r; }
  return U;
}

// One hit of the mate against one anchor: bit r set when the hit lies at a proper distance in the orientation r the two are in, else 0
// (native/bwamem_pair.c:119-124 / MemSamPe.scala:1131-1146)
inline int rescue_proper_bit(const RescueRules& U, int64_t a_rb, int64_t m_rb) {
  int64_t dist;
  const int r = rescue_infer_dir(U.l_pac, a_rb, m_rb, &dist);
  if (U.scala_narrow) dist = (int64_t)(int32_t)dist;
  return (dist >= U.low[r] && dist <= U.high[r]) ? 1 << r : 0;
}

// bit r set: orientation r of the anchor starting at a_rb needs no SW -- its statistics failed or one of the mate's hits already lies at
// a proper distance in that orientation.  15: the anchor needs nothing.  (No mate regions: `mates` is never looked at.)
template <class R>
inline int rescue_skip_flags(const RescueRules& U, int64_t a_rb, const R* mates, size_t n_mates) {
  int skip = U.failed_mask;
  for (size_t mi = 0; mi < n_mates; ++mi) skip |= rescue_proper_bit(U, a_rb, mates[mi].rb);
  return skip;
}

// The anchors of an end (native/bwamem_pair.c:126-131 / MemSamPe.scala:1944-1947): its regions within pen_unpaired of the best one, in
// list order, at most max_matesw of them and at most `cap` (the end's window rows; kRescueNoCap where those are being produced).
// f(j, ai) gets the anchor's rank and its index in the list and returns false to end the walk.
constexpr int kRescueNoCap = INT32_MAX;
template <class R, class F>
inline void rescue_walk_anchors(const RescueRules& U, const R* regs, int n, int cap, F&& f) {
  if (n <= 0) return;
  const int thr = regs[0].score - U.pen_unpaired;
  int j = 0;
  for (int ai = 0; ai < n; ++ai) {
    if (!(regs[ai].score >= thr)) continue;
    if (j >= U.max_matesw || j >= cap) break;
    if (!f(j, ai)) break;
    ++j;
  }
}

// What the plan reads of pair k besides its regions: region, window-row and mate-length counts of its two ends
struct RescuePairCounts { int rc[2], fc[2], sl[2]; };

// One pair against its INITIAL lists: open(i, j, skip) is called for anchor j of end i when not all of its orientations are skipped
// (skip: rescue_skip_flags) and returns true when nothing more is to be asked of end i now.  Fast: the common pair -- one hit per end,
// each its end's only anchor (it passes its own score threshold: pen_unpaired >= 0) with a window row and a mate to align -- is judged
// in straight-line code first: each end's only anchor against the other end's only hit; all four orientations skipped on both sides =
// nothing to do.  Anything else takes the general walk over both ends.  (Fast = false exists for tests/rescue_core_host: the two must agree.)
template <bool Fast = true, class R, class F>
inline void rescue_walk_pair(const RescueRules& U, const R* regs0, const R* regs1, const RescuePairCounts& p, F&& open) {
  if (Fast && p.rc[0] == 1 && p.rc[1] == 1 && p.fc[0] >= 1 && p.fc[1] >= 1 && p.sl[0] >= 1 && p.sl[1] >= 1 && U.max_matesw >= 1 && U.pen_unpaired >= 0) {
    const int m0 = U.failed_mask | rescue_proper_bit(U, regs0->rb, regs1->rb), m1 = U.failed_mask | rescue_proper_bit(U, regs1->rb, regs0->rb);
    if (m0 == 15 && m1 == 15) return;
  }
  const R* const regs[2] = {regs0, regs1};
  for (int i = 0; i < 2; ++i) {
    if (p.sl[i ^ 1] < 1) continue;  // a mate without bases never becomes a job
    rescue_walk_anchors(U, regs[i], p.rc[i], p.fc[i], [&](int j, int ai) {
      const int skip = rescue_skip_flags(U, regs[i][ai].rb, regs[i ^ 1], (size_t)p.rc[i ^ 1]);
      return !(skip != 15 && open(i, j, skip));
    });
  }
}

// length of window x as the SW sees it: shipped with the bytes, or -- coordinate mode (ref_pool == NULL), SURVEY.md 8f.2 -- what bnsGetSeq
// (util/BNTSeqUtil.scala:37-59) would return for (rb, re): swap, clamp to [0, 2 l_pac), nothing when it bridges the strands
inline int64_t rescue_win_len(const bpsw_rescue_group_t& g, int64_t x) {
  if (g.ref_pool) return g.ref_len[x];
  int64_t b = g.ref_rb[x], e = g.ref_re[x];
  if (b < 0 && e < 0) return 0;  // (-1,-1): failed orientation, MemSamPe.scala:1863-1868
  if (e < b) { const int64_t t = b; b = e; e = t; }
  if (e > (g.l_pac << 1)) e = g.l_pac << 1;
  if (b < 0) b = 0;
  if (!(b >= g.l_pac || e <= g.l_pac)) return 0;
  return e - b > 0 ? e - b : 0;
}
// "no funny things happening" (native/bwamem_pair.c:187): the window's bytes are all there
inline bool rescue_window_ok(const bpsw_rescue_group_t& g, int64_t x) { return rescue_win_len(g, x) == g.ref_re[x] - g.ref_rb[x]; }

// The plan of one pair: want(x, mate) for every window x (anchor row * 4 + orientation) to align before any result is known, `mate`
// being the end (2k + i) whose read is aligned; returns whether there was one.  reg_base / row_base: the first region / window row of
// each end.  Lean speculation: only the first anchor of an end that has a job is asked for now -- its hit may make the later anchors'
// jobs unnecessary; what they still need once its result is in, the replay asks for.
template <bool Fast = true, class W>
inline bool rescue_plan_pair(const RescueRules& U, const bpsw_rescue_group_t& g, int k, const RescuePairCounts& p, const int64_t reg_base[2],
                             const int64_t row_base[2], W&& want) {
  bool touched = false;
  rescue_walk_pair<Fast>(U, g.regs + reg_base[0], g.regs + reg_base[1], p, [&](int i, int j, int skip) {
    const int64_t x0 = (row_base[i] + j) * 4;
    bool emitted = false;
    for (int r = 0; r < 4; ++r)
      if (!((skip >> r) & 1) && rescue_window_ok(g, x0 + r)) { want(x0 + r, 2 * k + (i ^ 1)); emitted = true; }
    touched |= emitted;
    return emitted;
  });
  return touched;
}

// The shim's coarser verdict: the pair MAY need a job -- the same walk, blind to windows and mate lengths (a superset of the pairs
// rescue_plan_pair touches).  rc / fc: region and window-row counts of the two ends.
template <class R>
inline bool rescue_pair_may_need_job(const RescueRules& U, const R* regs0, const R* regs1, const int32_t rc[2], const int32_t fc[2]) {
  const RescuePairCounts p = {{rc[0], rc[1]}, {fc[0], fc[1]}, {1, 1}};
  bool may = false;
  rescue_walk_pair(U, regs0, regs1, p, [&](int, int, int) { return may = true; });
  return may;
}

}  // namespace bpsw
