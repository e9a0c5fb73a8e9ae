// bam_sort_host.cpp -- csrc/bpsw_bam_sort_core.h applied serially on the host, as a program of its own (built by
// tests/test_bam_sort_core_host.py with -fsanitize=address,undefined; tools/bam_sort_rate.py times a plain build of it).
//
//   bam_sort_host run <in> <out>
// <in> holds cases, one behind the other:
//   u32 n_ref | i32 len[n_ref] | i64 file_off | u32 P | u32 n_bounds | i64 bound[n_bounds] | u64 bytes | the stream
// (segment g is stream[bound[g], bound[g + 1])).  Per case <out> gets
//   u32 verdict: 0 fine, 1 a chain broke (then u64 segment, u64 stream offset), 2 a record was refused (then u64 index, u64 reason)
// and for verdict 0:  u64 n | i64 rec_off[n] | u64 key[n] | i64 perm[n] | u64 bai bytes | the BAI
// where perm is std::stable_sort's order of the record indices by key and the BAI is that of the sorted stream in stored blocks of P.
// Every stream is copied into a heap block of exactly its size first, so that a read past it is the sanitizer's.  stdout: the
// milliseconds each case took (the walk, the keys, the sort, the gather into a sorted stream, the BAI).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "bpsw_bam_sort_core.h"

namespace bs = bpsw::bamsort;

namespace {

std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  std::vector<uint8_t> v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
template <class T> T take(const std::vector<uint8_t>& v, size_t* at) {
  T x;
  if (*at + sizeof(T) > v.size()) { fprintf(stderr, "the input ends inside a case\n"); exit(2); }
  memcpy(&x, v.data() + *at, sizeof(T));
  *at += sizeof(T);
  return x;
}
template <class T> void put(std::vector<uint8_t>& out, T x) {
  const uint8_t* p = (const uint8_t*)&x;
  out.insert(out.end(), p, p + sizeof(T));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: bam_sort_host run <in> <out>\n"); return 2; }
  const std::vector<uint8_t> in = slurp(argv[2]);
  std::vector<uint8_t> out;
  size_t at = 0;
  while (at < in.size()) {
    const uint32_t n_ref = take<uint32_t>(in, &at);
    std::vector<int32_t> len(n_ref);
    for (uint32_t k = 0; k < n_ref; ++k) len[k] = take<int32_t>(in, &at);
    const int64_t file_off = take<int64_t>(in, &at);
    const uint32_t P = take<uint32_t>(in, &at), n_bounds = take<uint32_t>(in, &at);
    std::vector<long long> bound(n_bounds);
    for (uint32_t k = 0; k < n_bounds; ++k) bound[k] = take<int64_t>(in, &at);
    const uint64_t bytes = take<uint64_t>(in, &at);
    if (at + bytes > in.size() || n_bounds < 2 || P < 1) { fprintf(stderr, "a malformed case\n"); return 2; }
    uint8_t* stream = (uint8_t*)malloc(bytes ? bytes : 1);   // exactly the stream: a byte past it is the sanitizer's business
    memcpy(stream, in.data() + at, bytes);
    at += bytes;
    const auto t0 = std::chrono::steady_clock::now();

    // ---- the walk ----
    std::vector<long long> rec_off;
    long long bad_seg = -1, bad_at = 0;
    for (uint32_t g = 0; g + 1 < n_bounds && bad_seg < 0; ++g) {
      long long o = bound[g];
      const long long end = bound[g + 1];
      while (o < end) {
        const long long next = bs::walk_step(o, end, stream + o);
        if (next < 0) { bad_seg = g; bad_at = o; break; }
        rec_off.push_back(o);
        o = next;
      }
    }
    if (bad_seg >= 0) {
      put<uint32_t>(out, 1); put<uint64_t>(out, (uint64_t)bad_seg); put<uint64_t>(out, (uint64_t)bad_at);
      free(stream);
      continue;
    }
    // ---- the checks and the keys ----
    long long longest = 0;
    for (int32_t l : len) longest = std::max(longest, (long long)l);
    const bs::KeyShape ks = bs::key_shape((int32_t)n_ref, longest);
    const size_t n = rec_off.size();
    std::vector<unsigned long long> key(n);
    std::vector<bs::Meta> meta(n);
    long long bad_rec = -1;
    int reason = 0;
    for (size_t i = 0; i < n && bad_rec < 0; ++i) {
      reason = bs::check_record(stream + rec_off[i], ks, len.data(), &key[i], &meta[i]);
      if (reason) bad_rec = (long long)i;
    }
    if (bad_rec >= 0) {
      put<uint32_t>(out, 2); put<uint64_t>(out, (uint64_t)bad_rec); put<uint64_t>(out, (uint64_t)reason);
      free(stream);
      continue;
    }
    // ---- the order, the sorted stream, the BAI ----
    std::vector<long long> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = (long long)i;
    const unsigned long long mask = bs::key_bits(ks) >= 64 ? ~0ull : (1ull << bs::key_bits(ks)) - 1;
    std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return (key[a] & mask) < (key[b] & mask); });
    std::vector<bs::Entry> table(n);
    std::vector<uint8_t> sorted(bytes);
    long long to = 0;
    for (size_t j = 0; j < n; ++j) {
      const bs::Meta& m = meta[(size_t)perm[j]];
      const uint32_t l = m.len_unmapped & 0x7fffffffu;
      memcpy(sorted.data() + to, stream + rec_off[(size_t)perm[j]], l);
      table[j] = bs::Entry{m.ref, m.pos, m.end, (uint32_t)to | (m.len_unmapped & 0x80000000u)};
      to += l;
    }
    if (to != (long long)bytes) { fprintf(stderr, "the records do not add up to the stream\n"); return 1; }
    const size_t blocks = (bytes + P - 1) / P;
    std::vector<long long> coff(blocks + 1);
    for (size_t b = 0; b <= blocks; ++b) coff[b] = (long long)std::min((uint64_t)b * P, bytes) + 31ll * (long long)b;
    std::vector<uint8_t> bai;
    bs::build_bai(table.data(), (long long)n, (long long)bytes, (int32_t)n_ref, bs::Blocks{coff.data(), (long long)P, file_off}, &bai);
    printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());

    put<uint32_t>(out, 0); put<uint64_t>(out, n);
    for (size_t i = 0; i < n; ++i) put<int64_t>(out, rec_off[i]);
    for (size_t i = 0; i < n; ++i) put<uint64_t>(out, key[i]);
    for (size_t i = 0; i < n; ++i) put<int64_t>(out, perm[i]);
    put<uint64_t>(out, bai.size());
    out.insert(out.end(), bai.begin(), bai.end());
    free(stream);
  }
  FILE* f = fopen(argv[3], "wb");
  if (!f || (out.size() && fwrite(out.data(), 1, out.size(), f) != out.size())) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
  fclose(f);
  return 0;
}
