// bam_host.cpp -- csrc/bpsw_bam_core.h (what bam_len_kernel / bam_write_kernel / bgzf_frame_kernel compile) on the host, over the
// line records in pairs that tests/sam_pe_host/sam_pe_host.cpp generates: that file is included as it is, its main renamed, so the
// generator exists once.
//
// A program of its own (tests/test_bam_core_host.py builds it with -fsanitize=address,undefined and runs it):
//   * per line: bam_rec_len == the bytes bam_rec_write wrote, into a heap block of exactly that size (an overrun is a sanitizer report);
//     block_size is the length without itself; a block one byte short is refused with ST_OVERRUN and the byte behind it is untouched;
//     another expected length is ST_MISMATCH;
//   * argv[1] gets, per batch, whether it has qualities, the contig names by put_contig's rule and per line the SAM text sam_line_write gives for the same
//     table and the record's bytes: the Python side applies tests/bam_plain.py to the text and compares;
//   * argv[2] gets CRCs of slices of a dumped buffer (every length 0..70 and 1016..1024 at the four alignments, every split of them
//     through crc32_combine, and the 64-slice fold of bgzf_frame_kernel for a row of payload sizes) for the Python side to hold
//     against zlib.crc32; the fold is also held against the plain CRC here.
// A BAM holds positions in 32 bits, which the library's contig table guarantees (its lengths are int32); the generator's positions
// past that are folded into 30 bits here, lines and mate records alike, before anything is written.
//
// Compiled by hipcc (--offload-arch=gfx950 -x hip -c) the same file instantiates the core in three kernels of the shape of the
// library's: the test reads the compiler's resource remarks for them.
#define main sam_pe_host_main
#include "../sam_pe_host/sam_pe_host.cpp"
#undef main

#include "bpsw_bam_core.h"

namespace bc = bpsw::bamcore;

#if defined(__HIPCC__)
__global__ __launch_bounds__(64) void bam_len_kernel(sc::SamBatch B, int n_lines, int32_t* len) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i < n_lines) len[i] = (int32_t)bc::bam_rec_len(B, i);
}
__global__ __launch_bounds__(64) void bam_write_kernel(sc::SamBatch B, int n_lines, const long long* rec_off, char* stream, int* status) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n_lines) return;
  int st = 0;
  bc::bam_rec_write(stream + rec_off[i], stream + rec_off[i + 1], B, i, rec_off[i + 1] - rec_off[i], &st);
  if (st) atomicOr(status, st);
}
__global__ __launch_bounds__(64) void bgzf_crc_kernel(const uint8_t* src, int n, uint8_t* out) {
  __shared__ uint32_t tab[256];
  const int lane = (int)threadIdx.x;
  for (int k = 0; k < 4; ++k) tab[4 * lane + k] = bc::crc32_table_entry((uint32_t)(4 * lane + k));
  __syncthreads();
  const int slice = ((n + 63) / 64 + 3) & ~3;
  const int lo = lane * slice < n ? lane * slice : n, hi = lo + slice < n ? lo + slice : n;
  uint32_t crc = bc::crc32_shift(bc::crc32_bytes(tab, 0u, src + lo, hi - lo), n - hi);
  for (int d = 1; d < 64; d <<= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
  if (lane < bc::kBgzfHead) out[lane] = bc::bgzf_head_byte(lane, (uint32_t)n);
  if (lane < bc::kBgzfTail) out[bc::kBgzfHead + lane] = bc::bgzf_tail_byte(lane, crc, (uint32_t)n);
}
#endif

namespace {

void put_u32(FILE* f, uint32_t v) { fwrite(&v, 4, 1, f); }
void put_blob(FILE* f, const void* p, size_t n) { put_u32(f, (uint32_t)n); if (n) fwrite(p, 1, n, f); }

void fold_positions(Batch& b) {
  for (sc::SamLine& L : b.lines) if (L.pos > 0) L.pos &= 0x3fffffff;
  for (Place& m : b.mates) if (m.pos > 0) m.pos &= 0x3fffffff;
}

int check_records(const Batch& b, FILE* dump, long long* bytes) {
  const sc::SamBatch B = b.view();
  const int n_names = (int)b.ctg_at.size() + 2;  // (rids run two past the table)
  put_u32(dump, b.have_qual ? 1u : 0u);
  put_u32(dump, (uint32_t)n_names);
  for (int rid = 0; rid < n_names; ++rid) { const std::string s = contig_of(b, rid); put_blob(dump, s.data(), s.size()); }
  put_u32(dump, (uint32_t)b.lines.size());
  for (int i = 0; i < (int)b.lines.size(); ++i) {
    int st = -1;
    const long long tl = sc::sam_line_len(B, i);
    std::string text((size_t)tl, '\0');
    sc::sam_line_write(&text[0], &text[0] + tl, B, i, tl, &st);
    if (st) { fprintf(stderr, "line %d: the text's status %d\n", i, st); return 1; }
    const long long len = bc::bam_rec_len(B, i);
    if (len < 37) { fprintf(stderr, "line %d: bam_rec_len %lld\n", i, len); return 1; }
    char* blk = (char*)malloc((size_t)len);  // exactly the record: a store past it is a sanitizer report
    st = -1;
    const long long wrote = bc::bam_rec_write(blk, blk + len, B, i, len, &st);
    if (wrote != len || st != 0) { fprintf(stderr, "line %d: wrote %lld of %lld, status %d\n", i, wrote, len, st); return 1; }
    uint32_t block_size;
    memcpy(&block_size, blk, 4);
    if ((long long)block_size != len - 4) { fprintf(stderr, "line %d: block_size %u of a record of %lld bytes\n", i, block_size, len); return 1; }
    put_blob(dump, text.data(), text.size());
    put_blob(dump, blk, (size_t)len);
    free(blk);
    *bytes += len;
    // a byte short: refused with the status, and the byte behind the block is as it was
    char* small = (char*)malloc((size_t)len);
    small[len - 1] = 0x5a;
    st = -1;
    const long long n2 = bc::bam_rec_write(small, small + len - 1, B, i, len, &st);
    if (n2 != len || !(st & bc::ST_OVERRUN) || small[len - 1] != 0x5a) { fprintf(stderr, "line %d: a short end gave %lld, status %d\n", i, n2, st); return 1; }
    free(small);
    if ((i & 63) == 0) {
      char* big = (char*)malloc((size_t)len + 8);
      bc::bam_rec_write(big, big + len + 8, B, i, len + 1, &st);
      if (st != bc::ST_MISMATCH) { fprintf(stderr, "line %d: an unexpected length gave status %d\n", i, st); return 1; }
      free(big);
    }
  }
  return 0;
}

// the CRC of p[0, n) the way bgzf_frame_kernel takes it: 64 slices, each shifted by the bytes behind it, XORed
uint32_t fold64(const uint32_t* tab, const uint8_t* p, int n) {
  const int slice = ((n + 63) / 64 + 3) & ~3;
  uint32_t crc = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int lo = lane * slice < n ? lane * slice : n, hi = lo + slice < n ? lo + slice : n;
    crc ^= bc::crc32_shift(bc::crc32_bytes(tab, 0u, p + lo, hi - lo), n - hi);
  }
  return crc;
}

int check_crc(FILE* out) {
  std::vector<uint32_t> tab(256);
  for (uint32_t i = 0; i < 256; ++i) tab[i] = bc::crc32_table_entry(i);
  Rng g(4242);
  std::vector<uint8_t> buf(70000);
  for (uint8_t& x : buf) x = (uint8_t)(g() & 0xff);
  for (int k = 0; k < 3000; ++k) buf[(size_t)(g() % buf.size())] = 0;  // (zero bytes, which a CRC without its conditioning would not see)
  fprintf(out, "buf ");
  for (uint8_t x : buf) fprintf(out, "%02x", x);
  fprintf(out, "\n");
  for (int o = 0; o < 4; ++o)
    for (int len = 0; len <= 1024; len = len == 70 ? 1016 : len + 1) {
      const uint8_t* p = buf.data() + 16 + o;
      fprintf(out, "crc %d %d %u\n", 16 + o, len, bc::crc32_bytes(tab.data(), 0u, p, len));
      for (int k = 0; k <= len; k = (len > 70 && k == 3) ? len - 3 : k + 1) {  // every split of the short ones, the ends of the long ones
        const uint32_t a = bc::crc32_bytes(tab.data(), 0u, p, k), c = bc::crc32_bytes(tab.data(), 0u, p + k, len - k);
        fprintf(out, "comb %d %d %d %u\n", 16 + o, len, k, bc::crc32_combine(a, c, len - k));
        if (bc::crc32_bytes(tab.data(), a, p + k, len - k) != bc::crc32_combine(a, c, len - k)) { fprintf(stderr, "combine %d %d %d\n", o, len, k); return 1; }
      }
    }
  const int sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 1021, 4097, 65279, 65280};
  for (int n : sizes)
    for (int o = 0; o < 4; ++o) {
      const uint32_t f = fold64(tab.data(), buf.data() + o, n);
      if (f != bc::crc32_bytes(tab.data(), 0u, buf.data() + o, n)) { fprintf(stderr, "the 64-slice fold of %d bytes at %d differs from the plain CRC\n", n, o); return 1; }
      fprintf(out, "fold %d %d %u\n", o, n, f);
    }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: bam_host <records out> <crc out>\n"); return 2; }
  FILE* dump = fopen(argv[1], "wb");
  FILE* crc = fopen(argv[2], "w");
  if (!dump || !crc) { fprintf(stderr, "cannot open the outputs\n"); return 2; }
  Rng g(20261019);
  long long lines = 0, bytes = 0;
  put_u32(dump, 32);
  for (int variant = 0; variant < 32; ++variant) {
    Batch b = make_batch(g, variant, 700);
    fold_positions(b);
    if (check_mates(b) || check_records(b, dump, &bytes)) { fprintf(stderr, "(variant %d)\n", variant); return 1; }
    lines += (long long)b.lines.size();
  }
  if (lines < 20000) { fprintf(stderr, "only %lld lines\n", lines); return 1; }
  if (check_crc(crc)) return 1;
  fclose(dump);
  fclose(crc);
  printf("bam core: %lld records, %lld bytes, both flavours: lengths, exact blocks and short ends hold; CRC slices dumped\n", lines, bytes);
  return 0;
}
