// bpsw_bgzf_in.hip -- BGZF blocks inflated on the device: bgzf_inflate_kernel, its launch for the FASTQ entries (bpsw_fastq.hip, whose
// text then never crosses PCIe) and bpsw_bgzf_inflate, the entry that hands the bytes back.
//
// The rules -- the header walk, the bit reader, the tables, the symbol loop, the reasons -- are bpsw_inflate_core.h's; this file is who
// applies them.  With BPSW_BGZF_HOST that is inflate_serial of the same header on the calling thread.  Otherwise the calling thread
// walks the headers (the offsets of every block's bytes and their total are known before anything is launched), the whole blocks and
// the block table go up in one staged block, and one kernel runs:
//   bgzf_inflate_kernel  one wavefront per block, no workgroup waits for another.  The block's output window (up to 64 KiB) and its
//                        tables live in LDS (inflcore::Work, 71 828 bytes: two workgroups a CU); decoding is wave-uniform, a literal
//                        is stored by one lane, a match by as many lanes as it has bytes.  The wave's LDS accesses execute in the order
//                        they were issued, so between a store and the reads that depend on it stands a wave-scope fence (which orders
//                        the compiler and costs no instruction), not a wait.  At the end the window goes to HBM 16 bytes a lane.  A
//                        refusal is one vector atomicMin on a 64-bit word (block << 8 | reason): the lowest block wins, as in the twin.
#include <string.h>

#include <string>
#include <vector>

#include "bpsw_internal.h"
#include "bpsw_inflate_core.h"

using namespace bpsw;
namespace ic = bpsw::inflcore;

namespace {

struct WaveExec {  // the wavefront itself as inflate_member's executor
  int lane;
  template <class F> __device__ __forceinline__ void each(F&& f) const { f(lane); barrier(); }
  __device__ __forceinline__ void barrier() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ bool lane0() const { return lane == 0; }
  template <class F> __device__ __forceinline__ uint32_t fold_xor(F&& f) const {
    uint32_t v = f(lane);
    for (int d = 1; d < 64; d <<= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
  }
};

// Block b of the table: in[data_off, data_off + data_len) inflated to out[out_off, out_off + isize).  status[0]: the lowest
// block << 8 | reason (all ones before the launch: none); status[1]: the last byte of block `last_block`'s output (-1: nobody's).
__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ in, const ic::Block* __restrict__ tab, uint8_t* __restrict__ out,
                                                          int last_block, unsigned long long* __restrict__ status) {
  __shared__ ic::Work w;
  const int lane = (int)threadIdx.x;
  const ic::Block B = tab[blockIdx.x];
  const int reason = ic::inflate_member(w, WaveExec{lane}, in + B.data_off, B.data_len, B.isize, B.crc);
  if (reason) {
    if (lane == 0) atomicMin(status, (unsigned long long)blockIdx.x << 8 | (unsigned)reason);
    return;
  }
  // the window to its place: single bytes up to the first 16-byte line of the output, whole lines, single bytes behind the last
  uint8_t* dst = out + B.out_off;
  const int n = (int)B.isize;
  const int to_line = (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u), head = to_line < n ? to_line : n;
  const int lines = (n - head) >> 4, rest = head + 16 * lines;
  if (lane < head) dst[lane] = w.win[lane];
  for (int v = lane; v < lines; v += 64) {
    uint4 x;
    __builtin_memcpy(&x, w.win + head + 16 * v, 16);
    *reinterpret_cast<uint4*>(dst + head + 16 * v) = x;
  }
  if (rest + lane < n) dst[rest + lane] = w.win[rest + lane];
  if ((int)blockIdx.x == last_block && lane == 0) status[1] = w.win[n - 1];
}

// bgzf_walk, bgzf_inflate_kernel, the round trip with the copies
thread_local double t_bgzf[3] = {0., 0., 0.};

}  // namespace

namespace bpsw {

hipError_t launch_bgzf_inflate(hipStream_t s, const uint8_t* d_in, const void* d_tab, int n_blocks, uint8_t* d_out, int last_block,
                               unsigned long long* d_status) {
  if (n_blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, d_in, (const ic::Block*)d_tab, d_out, last_block, d_status);
  return hipGetLastError();
}

}  // namespace bpsw

extern "C" {

int bpsw_bgzf_inflate(bpsw_ctx_t* c, const char* in, size_t in_bytes, int flags, char* out, size_t cap, size_t* out_needed, int64_t* n_blocks,
                      int64_t* consumed) {
  if ((!c && !(flags & BPSW_BGZF_HOST)) || (!in && in_bytes) || (!out && cap) || !out_needed || !n_blocks || !consumed)
    return fail(BPSW_ERR_ARG, "bgzf_inflate: null argument");
  if (flags & ~(BPSW_BGZF_FINAL | BPSW_BGZF_HOST)) return fail(BPSW_ERR_ARG, "bgzf_inflate: unknown flag");
  *out_needed = 0; *n_blocks = 0; *consumed = 0;
  if (in_bytes >= ((size_t)1 << 31)) return fail(BPSW_ERR_LIMIT, "bgzf_inflate: a chunk of 2^31 bytes or more");
  const double t0 = wall_ms();
  t_bgzf[0] = t_bgzf[1] = t_bgzf[2] = 0.;
  thread_local ic::Walk W;
  ic::bgzf_walk((const uint8_t*)in, (long long)in_bytes, &W);
  t_bgzf[0] = wall_ms() - t0;
  if (W.bad_reason)
    return fail(BPSW_ERR_ARG, "bgzf_inflate: block " + std::to_string(W.bad_block) + ": " + ic::inflate_reason_text(W.bad_reason));
  if ((flags & BPSW_BGZF_FINAL) && W.consumed != (long long)in_bytes)
    return fail(BPSW_ERR_ARG, "bgzf_inflate: " + std::to_string((long long)in_bytes - W.consumed) + " bytes behind the last whole block (BPSW_BGZF_FINAL)");
  if (W.total >= (1ll << 31)) return fail(BPSW_ERR_LIMIT, "bgzf_inflate: 2^31 inflated bytes or more");
  *out_needed = (size_t)W.total;
  *n_blocks = (int64_t)W.blocks.size();
  *consumed = W.consumed;
  if ((size_t)W.total > cap) return fail(BPSW_ERR_CAPACITY, "bgzf_inflate: out has room for fewer bytes than the blocks hold (*out_needed)");
  long long bad_block = -1;
  int reason = 0;
  if (flags & BPSW_BGZF_HOST) {
    thread_local std::vector<ic::Work> work(1);
    reason = ic::inflate_serial(work[0], (const uint8_t*)in, W, (uint8_t*)out, &bad_block);
  } else if (!W.blocks.empty()) {
    ContextEntry entry(c);
    if (entry.rc != BPSW_OK) return entry.rc;
    hipStream_t s = c->stream;
    StageIn up;
    const int i_chunk = up.add(in, (size_t)W.consumed), i_tab = up.add(W.blocks.data(), sizeof(ic::Block) * W.blocks.size());
    HIP_TRY(c->d_bgzf.reserve(16 + align16((size_t)W.total) + 16));
    HIP_TRY(c->h_stage_out.reserve(16 + (size_t)W.total));
    unsigned long long* d_status = (unsigned long long*)c->d_bgzf.ptr;
    uint8_t* d_out = (uint8_t*)c->d_bgzf.ptr + 16;
    HIP_TRY(up.stage(c->h_stage_in, c->d_sw_in, s));
    HIP_TRY(hipMemsetAsync(d_status, 0xff, 16, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    HIP_TRY(launch_bgzf_inflate(s, up.dev<uint8_t>(i_chunk), up.dev<ic::Block>(i_tab), (int)W.blocks.size(), d_out, -1, d_status));
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(c->h_stage_out.ptr, c->d_bgzf.ptr, 16 + (size_t)W.total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    t_bgzf[1] = ms;
    const unsigned long long st = *(const unsigned long long*)c->h_stage_out.ptr;
    if (st != ~0ull) { bad_block = (long long)(st >> 8); reason = (int)(st & 0xff); }
    else if (W.total) memcpy(out, (const uint8_t*)c->h_stage_out.ptr + 16, (size_t)W.total);
  }
  t_bgzf[2] = wall_ms() - t0;
  if (flags & BPSW_BGZF_HOST) t_bgzf[0] = t_bgzf[1] = t_bgzf[2] = 0.;
  if (reason) return fail(BPSW_ERR_ARG, "bgzf_inflate: block " + std::to_string(bad_block) + ": " + ic::inflate_reason_text(reason));
  return BPSW_OK;
}

void bpsw_last_bgzf_times(double ms[3]) {
  if (ms) memcpy(ms, t_bgzf, sizeof t_bgzf);
}

}  // extern "C"
