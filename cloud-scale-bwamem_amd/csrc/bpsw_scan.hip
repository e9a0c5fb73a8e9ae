// bpsw_scan.hip -- a device-wide exclusive prefix sum over 64-bit values, in place, that also leaves the total.
//
// Three launches on one stream, and no workgroup waits for another (no look-back, no flag, no "last block done"): what a
// workgroup needs from the others it gets from the launch before.
//   1. scan_reduce_kernel   one workgroup per tile: the tile's sum                                  -> tile_sums[tile]
//   2. scan_tiles_kernel    ONE wavefront: the exclusive scan of the tile sums, 64 at a time with a carry, so any number of
//                           tiles works; the column's total                                          -> data[n]
//   3. scan_apply_kernel    one workgroup per tile: the scan inside the tile plus the tile's base   -> data[i]
// Inside a wavefront the scan is the DPP ladder of bpsw_wave.h on both halves of the value (wave_scan_add64); the four
// wavefronts of a workgroup meet in LDS.  Several columns of the same length go through the same three launches (blockIdx.y): column
// k is data[k (n + 1) .. k (n + 1) + n], its total in entry n.
//
// The tile (items per workgroup) is a launch parameter: bpsw_scan_set_tile (diagnostics) lowers it so that a few thousand items
// reach many tiles and a second level that loops.  Its first user is the seeding plan (bpsw_seed.hip).
#include <atomic>

#include "bpsw_internal.h"
#include "bpsw_wave.h"

using namespace bpsw;

namespace {

constexpr int kScanThreads = 256, kScanWaves = kScanThreads / 64;
constexpr int kScanDefaultTile = 2048;  // eight items a thread

__global__ __launch_bounds__(kScanThreads) void scan_reduce_kernel(const long long* __restrict__ data, long long n, int tile,
                                                                    long long* __restrict__ tile_sums) {
  __shared__ long long part[kScanWaves];
  const long long* col = data + (size_t)blockIdx.y * (size_t)(n + 1);
  const long long lo = (long long)blockIdx.x * tile, hi = lo + tile < n ? lo + tile : n;
  long long v = 0;
  for (long long i = lo + threadIdx.x; i < hi; i += kScanThreads) v += col[i];
  v = wave_scan_add64(v);  // lane 63: the wavefront's sum
  if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
#pragma unroll
    for (int k = 0; k < kScanWaves; ++k) s += part[k];
    tile_sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void scan_tiles_kernel(long long* __restrict__ tile_sums, int tiles, int cols, long long* __restrict__ data,
                                                         long long n) {
  const int lane = threadIdx.x;
  for (int c = 0; c < cols; ++c) {
    long long* t = tile_sums + (size_t)c * (size_t)tiles;
    long long carry = 0;
    for (int b0 = 0; b0 < tiles; b0 += 64) {  // (the trip count is the wavefront's: every lane is in every step of the ladder)
      const int i = b0 + lane;
      const long long v = i < tiles ? t[i] : 0;
      const long long inc = wave_scan_add64(v);
      if (i < tiles) t[i] = carry + inc - v;
      carry += readlane64(inc, 63);
    }
    if (lane == 0) data[(size_t)c * (size_t)(n + 1) + (size_t)n] = carry;
  }
}

__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(long long* __restrict__ data, long long n, int tile,
                                                                   const long long* __restrict__ tile_sums) {
  __shared__ long long part[kScanWaves];
  long long* col = data + (size_t)blockIdx.y * (size_t)(n + 1);
  const long long lo = (long long)blockIdx.x * tile, hi = lo + tile < n ? lo + tile : n;
  const int wave = threadIdx.x >> 6;
  long long carry = tile_sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
  for (long long i0 = lo; i0 < hi; i0 += kScanThreads) {  // (the trip count is the workgroup's: both barriers are met by all)
    const long long i = i0 + threadIdx.x;
    const long long v = i < hi ? col[i] : 0;
    const long long inc = wave_scan_add64(v);
    if ((threadIdx.x & 63) == 63) part[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanWaves; ++k) {
      const long long p = part[k];
      all += p;
      before += k < wave ? p : 0;
    }
    if (i < hi) col[i] = carry + before + inc - v;
    carry += all;
    __syncthreads();  // part is written again in the next step
  }
}

std::atomic<int> g_scan_tile{0};

}  // namespace

namespace bpsw {

int scan_tile_items() {
  const int t = g_scan_tile.load(std::memory_order_relaxed);
  return t > 0 ? t : kScanDefaultTile;
}

long long scan_tiles(long long n, int tile) { return n > 0 ? (n + tile - 1) / tile : 0; }

hipError_t scan_exclusive_i64(hipStream_t s, long long* data, int cols, long long n, int tile, long long* tile_sums) {
  if (cols < 1 || n < 0 || tile < 64 || tile % 64) return hipErrorInvalidValue;
  const long long tiles = scan_tiles(n, tile);
  if (tiles > 0x7fffffffll) return hipErrorInvalidValue;
  if (tiles > 0) {
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)tiles, (unsigned)cols), dim3(kScanThreads), 0, s, (const long long*)data, n, tile,
                       tile_sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(64), 0, s, tile_sums, (int)tiles, cols, data, n);  // (no tiles: the totals are 0)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || tiles == 0) return e;
  hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)tiles, (unsigned)cols), dim3(kScanThreads), 0, s, data, n, tile,
                     (const long long*)tile_sums);
  return hipGetLastError();
}

}  // namespace bpsw

extern "C" void bpsw_scan_set_tile(int items) {
  g_scan_tile.store(items <= 0 ? 0 : items < 64 ? 64 : (items + 63) / 64 * 64, std::memory_order_relaxed);
}
