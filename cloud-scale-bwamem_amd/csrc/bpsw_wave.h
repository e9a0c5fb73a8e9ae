// bpsw_wave.h -- wave64 cross-lane helpers (DPP) shared by the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace bpsw {

constexpr int NEG = -(1 << 29);

// DPP controls (gfx9 encodings)
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_WAVE_SHR1 = 0x138, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

// lanes whose source is out of range or masked off keep `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_mov(int old, int src) {
  return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false);
}
// lane l <- lane l-1 ; lane 0 <- old
__device__ __forceinline__ int wave_shr1(int old, int src) { return dpp_mov<DPP_WAVE_SHR1, 0xf>(old, src); }

// inclusive max-scan over the 64 lanes; lane 63 ends up with the wave maximum
__device__ __forceinline__ int wave_scan_max(int v) {
  v = max(v, dpp_mov<DPP_ROW_SHR1, 0xf>(NEG, v));
  v = max(v, dpp_mov<DPP_ROW_SHR2, 0xf>(NEG, v));
  v = max(v, dpp_mov<DPP_ROW_SHR4, 0xf>(NEG, v));
  v = max(v, dpp_mov<DPP_ROW_SHR8, 0xf>(NEG, v));
  v = max(v, dpp_mov<DPP_ROW_BCAST15, 0xa>(NEG, v));
  v = max(v, dpp_mov<DPP_ROW_BCAST31, 0xc>(NEG, v));
  return v;
}
// inclusive prefix sum / prefix minimum over the 64 lanes (same DPP ladder)
__device__ __forceinline__ int wave_scan_add(int v) {
  v += dpp_mov<DPP_ROW_SHR1, 0xf>(0, v);
  v += dpp_mov<DPP_ROW_SHR2, 0xf>(0, v);
  v += dpp_mov<DPP_ROW_SHR4, 0xf>(0, v);
  v += dpp_mov<DPP_ROW_SHR8, 0xf>(0, v);
  v += dpp_mov<DPP_ROW_BCAST15, 0xa>(0, v);
  v += dpp_mov<DPP_ROW_BCAST31, 0xc>(0, v);
  return v;
}
// the same over 64-bit values: both halves moved by the same control, one 64-bit add per step
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_mov64(long long src) {
  const int lo = dpp_mov<CTRL, ROW_MASK>(0, (int)(unsigned long long)src);
  const int hi = dpp_mov<CTRL, ROW_MASK>(0, (int)((unsigned long long)src >> 32));
  return (long long)((unsigned long long)(unsigned)hi << 32 | (unsigned)lo);
}
__device__ __forceinline__ long long wave_scan_add64(long long v) {
  v += dpp_mov64<DPP_ROW_SHR1, 0xf>(v);
  v += dpp_mov64<DPP_ROW_SHR2, 0xf>(v);
  v += dpp_mov64<DPP_ROW_SHR4, 0xf>(v);
  v += dpp_mov64<DPP_ROW_SHR8, 0xf>(v);
  v += dpp_mov64<DPP_ROW_BCAST15, 0xa>(v);
  v += dpp_mov64<DPP_ROW_BCAST31, 0xc>(v);
  return v;
}
__device__ __forceinline__ long long readlane64(long long v, int lane) {
  const int lo = __builtin_amdgcn_readlane((int)(unsigned long long)v, lane);
  const int hi = __builtin_amdgcn_readlane((int)((unsigned long long)v >> 32), lane);
  return (long long)((unsigned long long)(unsigned)hi << 32 | (unsigned)lo);
}
constexpr int POS = 1 << 29;
__device__ __forceinline__ int wave_scan_min(int v) {
  v = min(v, dpp_mov<DPP_ROW_SHR1, 0xf>(POS, v));
  v = min(v, dpp_mov<DPP_ROW_SHR2, 0xf>(POS, v));
  v = min(v, dpp_mov<DPP_ROW_SHR4, 0xf>(POS, v));
  v = min(v, dpp_mov<DPP_ROW_SHR8, 0xf>(POS, v));
  v = min(v, dpp_mov<DPP_ROW_BCAST15, 0xa>(POS, v));
  v = min(v, dpp_mov<DPP_ROW_BCAST31, 0xc>(POS, v));
  return v;
}
__device__ __forceinline__ int wave_max(int v) { return __builtin_amdgcn_readlane(wave_scan_max(v), 63); }

__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// `n` bytes from src to dst by the 64 lanes of a wavefront: single bytes up to the first 16-byte line of the destination, whole lines
// 16 bytes a lane (the source is wherever it is), single bytes behind the last line
__device__ inline void copy_lines(const uint8_t* src, uint8_t* dst, int n, int lane) {
  int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
  if (head > n) head = n;
  const int lines = (n - head) / 16, rest = head + 16 * lines;
  if (lane < head) dst[lane] = src[lane];
  for (int v = lane; v < lines; v += 64) {
    uint4 x;
    __builtin_memcpy(&x, src + head + 16 * v, 16);
    *reinterpret_cast<uint4*>(dst + head + 16 * v) = x;
  }
  if (rest + lane < n) dst[rest + lane] = src[rest + lane];
}

}  // namespace bpsw
