// sift_n_host.cpp -- the sift kernel's arithmetic (csrc/bpsw_extend_sift_core.h) compiled for the HOST with flanks that hold N, so
// that tests/test_sift_n_host.py can hold it against the oracle's full DP without a GPU.  Test infrastructure, like tests/sift_host
// (which keeps every flank with an N away from the arithmetic, as the kernel did before an N column became a deficit column of its
// own weight): sift_n_host_batch mirrors what a lane of ext_sift_kernel<false> does with a task of a format-1 wire batch,
// sift_n_host_sides judges single flanks given as code arrays and returns the whole verdict of each.
// With -DSIFT_N_HOST_MAIN the file is a program of its own: it reads a flank set written by the test, judges it and prints a
// checksum of the verdicts -- the form a sanitizer build takes (-fsanitize=address,undefined), never loaded into an interpreter.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bpsw_extend_sift_core.h"

using namespace bpsw::sift;

static int lo16(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
static int hi16(uint32_t v) { return (int)(int16_t)(v >> 16); }

// one side as the kernel judges it: closed form, every shift of its certificate, start-gap form
static void judge_side(const SiftSeq& s, const int qLen, const int rLen, const SiftParams& P, SideRec* r) {
  *r = SideRec{SIFT_UNSEEN, 0, 0, 0, 0, 0, 0, 0};
  if (P.dn <= 0 && sift_flank_has_n(s, qLen, rLen, true)) return;
  int k = 0, p[3] = {0, 0, 0}, dI = 0, dD = 0;
  int st = sift_closed_form(s, qLen, rLen, P, r, &k, p, &dI, &dD);
  if (st == CF_IF_CERTIFIED) {
    bool ok = true;
    for (int d = 1; d <= dI && ok; ++d) ok = sift_certificate_shift(s, qLen, rLen, P, k, p[0], p[1], p[2], true, d);
    for (int d = 1; d <= dD && ok; ++d) ok = sift_certificate_shift(s, qLen, rLen, P, k, p[0], p[1], p[2], false, d);
    st = ok ? CF_HOLDS : CF_FAILS;
  }
  if (st == CF_FAILS) {
    r->kind = SIFT_FAIL;
    (void)sift_start_gap_form(s, qLen, rLen, P, r);
  } else if (st == CF_UNSEEN) {
    r->kind = SIFT_UNSEEN;
  }
}

// gaps[4] = oDel, eDel, oIns, eIns
static SiftParams params(const int* gaps, int wBand, int zdrop, int certify, int exact_a, int dm, int dn) {
  SiftParams P;
  P.oDel = gaps[0]; P.eDel = gaps[1]; P.oIns = gaps[2]; P.eIns = gaps[3];
  P.wBand = wBand; P.zdrop = zdrop; P.certify = certify; P.dm = dm; P.dn = dn;
  const int oe_min = sift_min(P.oIns + P.eIns, P.oDel + P.eDel);
  P.a = (oe_min > 0 && P.wBand >= 2) ? exact_a : 0;
  return P;
}

// flag[t]: 0 not examined, 1 record written (out + 10 t), 2 verdicts only; kinds[2 t + side]: SIFT_UNSEEN / _FAIL / _FORM
extern "C" int sift_n_host_batch(const uint32_t* wire, size_t wire_words, int n, int zdrop, int certify, int exact_a, int dm, int dn,
                                 int qmax, int16_t* out, uint8_t* flag, uint8_t* kinds) {
  const uint32_t hdr0 = wire[0], hdr1 = wire[1];
  const int gaps[4] = {(int8_t)(hdr0 & 0xff), (int8_t)((hdr0 >> 8) & 0xff), (int8_t)((hdr0 >> 16) & 0xff), (int8_t)((hdr0 >> 24) & 0xff)};
  const int penClip5 = (int8_t)(hdr1 & 0xff), penClip3 = (int8_t)((hdr1 >> 8) & 0xff);
  const SiftParams P = params(gaps, (int8_t)((hdr1 >> 16) & 0xff), zdrop, certify, exact_a, dm, dn);
  std::vector<uint32_t> raw;
  for (int t = 0; t < n; ++t) {
    const uint32_t* rec = wire + 8 + 8 * (size_t)t;
    const int lq = lo16(rec[0]), lr = hi16(rec[0]), rq = lo16(rec[1]), rr = hi16(rec[1]);
    const int pos = (int)rec[2];
    const int nwords = (lq + lr + rq + rr + 7) >> 3;
    flag[t] = 0; kinds[2 * t] = kinds[2 * t + 1] = SIFT_UNSEEN;
    if (P.a <= 0 || dm <= 0 || lq > qmax || rq > qmax) continue;
    if ((size_t)pos + (size_t)nwords > wire_words) return -1;
    raw.assign(wire + pos, wire + pos + nwords);
    raw.resize((size_t)nwords + 4, 0u);
    SideRec sr[2] = {{SIFT_UNSEEN, 0, 0, 0, 0, 0, 0, 0}, {SIFT_UNSEEN, 0, 0, 0, 0, 0, 0, 0}};
    for (int side = 0; side < 2; ++side) {
      const int qLen = side ? rq : lq, rLen = side ? rr : lr;
      if (qLen <= 0) continue;
      const SiftSeq s = {raw.data(), side ? lq : 0, raw.data(), side ? lq + rq + lr : lq + rq};
      judge_side(s, qLen, rLen, P, &sr[side]);
      kinds[2 * t + side] = (uint8_t)sr[side].kind;
    }
    const SiftTask T = {lq, rq, lo16(rec[3]), hi16(rec[3]), lo16(rec[4]), (int)rec[7], penClip5, penClip3, P.wBand};
    uint32_t o[5];
    if (sift_chain(T, sr[0], sr[1], o)) {
      memcpy(out + 10 * (size_t)t, o, 20);
      flag[t] = 1;
    } else {
      flag[t] = 2;
    }
  }
  return 0;
}

static void pack_nibbles(std::vector<uint32_t>& w, const uint8_t* codes, int len) {
  w.assign((size_t)((len + 7) >> 3) + 4, 0u);
  for (int i = 0; i < len; ++i) w[i >> 3] |= (uint32_t)(codes[i] & 0xFu) << (28 - 4 * (i & 7));
}

// n flanks: flank i has the query codes pool[off[2i] .. +len[2i]) and the target codes pool[off[2i+1] .. +len[2i+1]), 1 <= qLen <= 127;
// rec[8 i ..]: kind, hmin, max_rel, g_rel, qle, tle, gtle, max_off (the last six as they stand for a start score h: max = h + max_rel,
// gscore = h + g_rel)
extern "C" int sift_n_host_sides(int n, const uint8_t* pool, const int64_t* off, const int32_t* len, const int* gaps, int wBand, int zdrop,
                                 int certify, int exact_a, int dm, int dn, int32_t* rec) {
  const SiftParams P = params(gaps, wBand, zdrop, certify, exact_a, dm, dn);
  std::vector<uint32_t> qw, tw;
  for (int i = 0; i < n; ++i) {
    const int qLen = len[2 * i], rLen = len[2 * i + 1];
    SideRec r = {SIFT_UNSEEN, 0, 0, 0, 0, 0, 0, 0};
    if (qLen < 1 || qLen > 127 || rLen < 0) return -1;
    if (P.a > 0 && dm > 0) {
      pack_nibbles(qw, pool + off[2 * i], qLen);
      pack_nibbles(tw, pool + off[2 * i + 1], rLen);
      const SiftSeq s = {qw.data(), 0, tw.data(), 0};
      judge_side(s, qLen, rLen, P, &r);
    }
    const int v[8] = {r.kind, r.hmin, r.max_rel, r.g_rel, r.qle, r.tle, r.gtle, r.max_off};
    memcpy(rec + 8 * (size_t)i, v, sizeof v);
  }
  return 0;
}

// FNV-1a over the bytes of `count` verdict words, continued from h
extern "C" uint64_t sift_n_host_checksum(const int32_t* rec, size_t count, uint64_t h) {
  for (size_t i = 0; i < count; ++i) {
    const uint32_t v = (uint32_t)rec[i];
    for (int b = 0; b < 4; ++b) { h ^= (v >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
  }
  return h;
}

#ifdef SIFT_N_HOST_MAIN
// the flank set of the test as a file: int32 header {n, pool bytes, oDel, eDel, oIns, eIns, wBand, zdrop, certify, exact_a, dm, dn},
// int64 off[2n], int32 len[2n], the pool; any number of such blocks.  Prints one FNV-1a checksum over all the verdicts.
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h = 1469598103934665603ull;
  long long total = 0;
  int32_t hd[12];
  while (fread(hd, sizeof hd, 1, f) == 1) {
    const int n = hd[0];
    if (n < 0 || hd[1] < 0) return 3;
    std::vector<int64_t> off(2 * (size_t)n);
    std::vector<int32_t> len(2 * (size_t)n), rec(8 * (size_t)n);
    std::vector<uint8_t> pool((size_t)hd[1]);
    if (n && (fread(off.data(), 8, off.size(), f) != off.size() || fread(len.data(), 4, len.size(), f) != len.size())) return 3;
    if (!pool.empty() && fread(pool.data(), 1, pool.size(), f) != pool.size()) return 3;
    for (int i = 0; i < 2 * n; ++i)
      if (off[i] < 0 || len[i] < 0 || (uint64_t)off[i] + (uint64_t)len[i] > pool.size()) return 3;
    if (sift_n_host_sides(n, pool.data(), off.data(), len.data(), hd + 2, hd[6], hd[7], hd[8], hd[9], hd[10], hd[11], rec.data()) != 0) return 4;
    h = sift_n_host_checksum(rec.data(), rec.size(), h);
    total += n;
  }
  fclose(f);
  printf("%lld %016llx\n", total, (unsigned long long)h);
  return 0;
}
#endif
