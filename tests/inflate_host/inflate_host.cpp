// inflate_host.cpp -- csrc/bpsw_inflate_core.h (what bgzf_inflate_kernel compiles) on the host: bgzf_walk and inflate_serial, the twin
// that plays the 64 lanes in a loop.  A program of its own: tests/test_inflate_core_host.py builds it with -fsanitize=address,undefined
// and tests/test_bgzf_in_gpu.py without, as what the device's bytes and reasons must equal.
//
//   inflate_host run <in> <out>     <in>: cases of [u32 n | n bytes of a chunk].  The chunk is walked, then the whole blocks go through
//                                   inflate_serial from a heap block of exactly their bytes into one of exactly the inflated size, and
//                                   again block by block with each block's deflate data in a heap block of its own (a read outside
//                                   it is a sanitizer report); the two must agree.  <out> gets per case
//                                   [u32 blocks | i64 consumed | i64 total | i64 bad block | i32 reason | u32 header (1: the reason is
//                                   the walk's) | per block 6 x u32 | the bytes when there is no reason].
//   inflate_host trunc <in> <out>   <in>: cases of [u32 n | u32 cuts | n bytes of one block | cuts x u32]: the block's deflate data cut
//                                   to each of the lengths, in a heap block of exactly that many bytes; <out> gets a reason byte per cut.
//   inflate_host text               the reasons' texts, one per line: "<code> <text>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpsw_inflate_core.h"

namespace ic = bpsw::inflcore;

namespace {

bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }
template <class T> void put(FILE* f, T v) { fwrite(&v, sizeof v, 1, f); }

// a copy of p[0, n) in a heap block of exactly n bytes (one byte when n is 0, which is never read)
uint8_t* exact(const uint8_t* p, size_t n) {
  uint8_t* q = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(q, p, n);
  return q;
}

int run(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "rb");
  FILE* out = fopen(out_path, "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  ic::Work* w = new ic::Work;
  uint32_t n, cases = 0;
  while (read_u32(in, &n)) {
    std::vector<uint8_t> buf(n);
    if (n && fread(buf.data(), 1, n, in) != n) { fprintf(stderr, "a short case\n"); return 2; }
    uint8_t* chunk = exact(buf.data(), n);
    ic::Walk W;
    ic::bgzf_walk(chunk, (long long)n, &W);
    free(chunk);
    long long bad = W.bad_block;
    int reason = W.bad_reason;
    const uint32_t header = reason != 0;
    std::vector<uint8_t> bytes;
    if (!reason) {
      uint8_t* whole = exact(buf.data(), (size_t)W.consumed);
      uint8_t* dst = (uint8_t*)malloc(W.total ? (size_t)W.total : 1);
      memset(dst, 0xa5, W.total ? (size_t)W.total : 1);
      reason = ic::inflate_serial(*w, whole, W, dst, &bad);
      // ... and every block alone, its deflate data in a block of its own
      long long bad2 = -1;
      int reason2 = 0;
      std::vector<uint8_t> again((size_t)W.total);
      for (size_t b = 0; b < W.blocks.size() && !reason2; ++b) {
        const ic::Block& B = W.blocks[b];
        uint8_t* data = exact(buf.data() + B.data_off, B.data_len);
        reason2 = ic::inflate_member(*w, ic::SerialExec(), data, B.data_len, B.isize, B.crc);
        free(data);
        if (reason2) bad2 = (long long)b;
        else if (B.isize) memcpy(again.data() + B.out_off, w->win, B.isize);
      }
      if (reason != reason2 || bad != bad2 || (!reason && W.total && memcmp(again.data(), dst, (size_t)W.total))) {
        fprintf(stderr, "case %u: the chunk and its blocks one by one disagree (%d at %lld, %d at %lld)\n", cases, reason, bad, reason2, bad2);
        return 1;
      }
      if (!reason) bytes.assign(dst, dst + W.total);
      free(dst); free(whole);
    }
    put(out, (uint32_t)W.blocks.size()); put(out, (int64_t)W.consumed); put(out, (int64_t)W.total); put(out, (int64_t)bad);
    put(out, (int32_t)reason); put(out, header);
    for (const ic::Block& B : W.blocks) { put(out, B.coff); put(out, B.data_off); put(out, B.data_len); put(out, B.isize); put(out, B.crc); put(out, B.out_off); }
    if (!bytes.empty()) fwrite(bytes.data(), 1, bytes.size(), out);
    ++cases;
  }
  delete w;
  fclose(in); fclose(out);
  printf("inflate core: %u cases\n", cases);
  return 0;
}

int trunc_cases(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "rb");
  FILE* out = fopen(out_path, "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  ic::Work* w = new ic::Work;
  uint32_t n, cuts;
  while (read_u32(in, &n)) {
    if (!read_u32(in, &cuts)) return 2;
    std::vector<uint8_t> buf(n);
    std::vector<uint32_t> cut(cuts);
    if (n && fread(buf.data(), 1, n, in) != n) return 2;
    if (cuts && fread(cut.data(), 4, cuts, in) != cuts) return 2;
    ic::Walk W;
    ic::bgzf_walk(buf.data(), (long long)n, &W);
    if (W.bad_reason || W.blocks.size() != 1) { fprintf(stderr, "a truncation case is one whole block\n"); return 2; }
    const ic::Block& B = W.blocks[0];
    for (uint32_t k : cut) {
      if (k > B.data_len) return 2;
      uint8_t* data = exact(buf.data() + B.data_off, k);
      put(out, (uint8_t)ic::inflate_member(*w, ic::SerialExec(), data, k, B.isize, B.crc));
      free(data);
    }
  }
  delete w;
  fclose(in); fclose(out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "trunc")) return trunc_cases(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "text")) {
    for (int r = 1; r < ic::R_COUNT; ++r) printf("%d %s\n", r, ic::inflate_reason_text(r));
    return 0;
  }
  fprintf(stderr, "usage: inflate_host run <in> <out> | trunc <in> <out> | text\n");
  return 2;
}
