// deflate_host.cpp -- csrc/bpsw_deflate_core.h (what bgzf_deflate_kernel compiles) on the host: block_serial, the twin that plays the 64
// lanes in a loop.  A program of its own: tests/test_deflate_core_host.py builds it with -fsanitize=address,undefined and
// tests/test_bam_deflate_gpu.py without, as what the device's bytes must equal.
//
//   deflate_host run <in> <out>   <in>: cases of [u32 P | u32 n | n bytes]; the n bytes are cut every P bytes and every payload is framed
//                                 into heap blocks of exactly the room the contract names (an overrun is a sanitizer report), twice, and
//                                 the two results must agree; <out> gets per case [u32 bytes | the framed blocks one behind the other].
//   deflate_host self             prints what the Python side asserts on: the code-length alphabet's lengths for hand-made counts that are
//                                 Fibonacci numbers (an unlimited tree would be 10 deep), the ends of match_len at distance 32768, and the
//                                 symbols of every length and distance against the tables of RFC 1951 3.2.5.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bpsw_deflate_core.h"

namespace dc = bpsw::deflcore;
namespace bc = bpsw::bamcore;

namespace {

bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

// one payload -> its framed block, in blocks of exactly the size block_serial is promised
std::vector<uint8_t> frame(dc::Work& w, const uint8_t* src, int n) {
  const size_t room = ((size_t)n + bc::kBgzfAround + 3) & ~(size_t)3;
  uint8_t* dst = (uint8_t*)aligned_alloc(16, (room + 15) & ~(size_t)15);
  uint16_t* tok = (uint16_t*)malloc(2 * (size_t)n);
  uint8_t* pay = (uint8_t*)malloc((size_t)n);  // (the payload alone: a read past it is a report too)
  memcpy(pay, src, (size_t)n);
  memset(dst, 0xa5, room);
  const uint32_t got = dc::block_serial(w, pay, n, tok, dst);
  std::vector<uint8_t> out(dst, dst + got);
  if (got > (uint32_t)n + bc::kBgzfAround) { fprintf(stderr, "a block of %d bytes framed to %u\n", n, got); exit(1); }
  free(pay); free(tok); free(dst);
  return out;
}

int run(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "rb");
  FILE* out = fopen(out_path, "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  dc::Work* w = new dc::Work;
  uint32_t P, n, cases = 0;
  unsigned long long bytes = 0;
  while (read_u32(in, &P)) {
    if (!read_u32(in, &n) || P < 1 || P > (uint32_t)bc::kBgzfMaxPayload) { fprintf(stderr, "a bad case header\n"); return 2; }
    std::vector<uint8_t> buf(n);
    if (n && fread(buf.data(), 1, n, in) != n) { fprintf(stderr, "a short case\n"); return 2; }
    std::vector<uint8_t> all;
    for (size_t at = 0; at < n; at += P) {
      const int len = (int)(n - at < P ? n - at : P);
      const std::vector<uint8_t> a = frame(*w, buf.data() + at, len), b = frame(*w, buf.data() + at, len);
      if (a != b) { fprintf(stderr, "case %u: the same payload gave other bytes the second time\n", cases); return 1; }
      all.insert(all.end(), a.begin(), a.end());
    }
    const uint32_t total = (uint32_t)all.size();
    fwrite(&total, 4, 1, out);
    if (total) fwrite(all.data(), 1, total, out);
    ++cases;
    bytes += n;
  }
  delete w;
  fclose(in);
  fclose(out);
  printf("deflate core: %u cases, %llu bytes\n", cases, bytes);
  return 0;
}

int self() {
  dc::Work* w = new dc::Work;
  // ---- the 7-bit limit: eleven used lengths whose counts are 1 1 2 3 5 8 13 21 34 55 and 173 (89 and the 84 that fill 316 entries) ----
  const uint32_t fib[11] = {1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 173};
  for (int l = 0; l < dc::kLanes; ++l) dc::init_lane(*w, l);
  for (int k = 0; k < 11; ++k) w->cl_freq[k + 1] = fib[k];
  for (int l = 0; l < dc::kLanes; ++l) dc::rank_lane(*w, w->cl_freq, dc::kNumCL, l);
  dc::lengths_serial(*w, w->cl_freq, dc::kNumCL, dc::kBitsCL, w->cl_len);
  printf("cl");
  for (int s = 0; s < dc::kNumCL; ++s) printf(" %d", (int)w->cl_len[s]);
  printf("\n");
  // ... and the same counts under the limit of the two large alphabets, where nothing has to give
  for (int l = 0; l < dc::kLanes; ++l) dc::rank_lane(*w, w->cl_freq, dc::kNumCL, l);  // (the sort is spent: key holds depths now)
  dc::lengths_serial(*w, w->cl_freq, dc::kNumCL, dc::kBitsLL, w->cl_len);
  printf("free");
  for (int s = 0; s < dc::kNumCL; ++s) printf(" %d", (int)w->cl_len[s]);
  printf("\n");
  // ---- a candidate 32768 bytes back is a match, one byte further is none -------------------------------------------------------------
  std::vector<uint8_t> p(65280);
  uint32_t x = 12345;
  for (int i = 0; i < 32769; ++i) { x = x * 1664525u + 1013904223u; p[(size_t)i] = (uint8_t)(x >> 24); }
  for (int i = 32768; i < 65280; ++i) p[(size_t)i] = p[(size_t)i - 32768];
  printf("reach %d %d\n", dc::match_len(p.data(), 40000, 40000 - 32768, 258), dc::match_len(p.data(), 40000, 40000 - 32768, 100));
  for (int i = 32769; i < 65280; ++i) p[(size_t)i] = p[(size_t)i - 32769];
  printf("beyond %d %d\n", dc::match_len(p.data(), 40000, 40000 - 32769, 258), dc::match_len(p.data(), 40000, 40000, 258));
  // ---- every length and distance: symbol, number of extra bits, their value ----------------------------------------------------------
  for (int len = 3; len <= 258; ++len) printf("len %d %d %d %u\n", len, dc::len_code(len), dc::len_extra_bits(len), dc::len_extra(len));
  for (int d = 1; d <= 32768; ++d) printf("dist %d %d %d %u\n", d, dc::dist_code(d), dc::dist_extra_bits(d), dc::dist_extra(d));
  printf("order");
  for (int k = 0; k < dc::kNumCL; ++k) printf(" %d", dc::cl_order(k));
  printf("\n");
  delete w;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "self")) return self();
  fprintf(stderr, "usage: deflate_host run <in> <out> | deflate_host self\n");
  return 2;
}
