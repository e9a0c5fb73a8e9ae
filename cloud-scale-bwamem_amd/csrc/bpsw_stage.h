// bpsw_stage.h -- the staged block: how a host entry ships a job table to a kernel and takes the results back.
//
// A block is a row of parts, each at the previous part's end rounded up to its own alignment (16 bytes unless said otherwise):
//   o_0 = 0,  o_k = align_k(o_{k-1} + size_{k-1}),  total = align16(o_last + size_last)
// -- the definition the kernels index by.  StageLayout is that arithmetic on sizes alone; StageIn / StageOut put one block each
// through a pinned host buffer and a device buffer: a part is named once, with its source and its size, and read back through a
// typed accessor, so that an offset, a byte count and an element type cannot drift apart.
//
// Host only.  Included by bpsw_internal.h behind bpsw::PinnedBuffer / bpsw::DeviceBuffer ({ void* ptr; size_t cap;
// hipError_t reserve(size_t); }); tests/stage_host/stage_host.cpp includes it behind stand-ins for the two.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace bpsw {

struct StageLayout {
  size_t end = 0;  // the last part's end, not rounded
  size_t add(size_t bytes, size_t align = 16) {
    const size_t at = (end + align - 1) & ~(align - 1);
    end = at + bytes;
    return at;
  }
  size_t total() const { return (end + 15) & ~(size_t)15; }
};

constexpr int kStageMaxParts = 12;  // the widest block, chain2aln's input, has 11

// Host -> device.  add() every part, then stage(): both buffers reserved, every part copied into the pinned block once, one H2D
// copy enqueued.  A part without a source (or of zero bytes) is laid out and not copied: the caller fills it through host<T>()
// between pack() and send(), the two halves of stage(), or leaves it as padding.
struct StageIn {
  struct Part { const void* src; size_t bytes, at; };
  StageLayout lay;
  Part part[kStageMaxParts];
  int n = 0;
  uint8_t* h = nullptr;
  uint8_t* d = nullptr;

  int add(const void* src, size_t bytes, size_t align = 16) {
    if (n == kStageMaxParts) abort();
    part[n].src = src; part[n].bytes = bytes; part[n].at = lay.add(bytes, align);
    return n++;
  }
  size_t total() const { return lay.total(); }
  hipError_t pack(PinnedBuffer& pinned, DeviceBuffer& dev) {
    hipError_t e = pinned.reserve(total());
    if (e == hipSuccess) e = dev.reserve(total());
    if (e != hipSuccess) return e;
    h = (uint8_t*)pinned.ptr; d = (uint8_t*)dev.ptr;
    for (int k = 0; k < n; ++k)
      if (part[k].src && part[k].bytes) memcpy(h + part[k].at, part[k].src, part[k].bytes);  // (memcpy from null is undefined even at length 0)
    return hipSuccess;
  }
  hipError_t send(hipStream_t s) { return hipMemcpyAsync(d, h, total(), hipMemcpyHostToDevice, s); }
  hipError_t stage(PinnedBuffer& pinned, DeviceBuffer& dev, hipStream_t s) {
    const hipError_t e = pack(pinned, dev);
    return e == hipSuccess ? send(s) : e;
  }
  template <class T> T* host(int p) const { return (T*)(h + part[p].at); }
  template <class T> const T* dev(int p) const { return (const T*)(d + part[p].at); }
};

// Device -> host.  add() every part by size, reserve(), launch over dev<T>(), fetch(), and after the stream has been waited for
// read host<T>().  The pinned block is the context's: its pointers hold until the next block is reserved over it.
struct StageOut {
  StageLayout lay;
  size_t at[kStageMaxParts];
  int n = 0;
  uint8_t* h = nullptr;
  uint8_t* d = nullptr;

  int add(size_t bytes, size_t align = 16) {
    if (n == kStageMaxParts) abort();
    at[n] = lay.add(bytes, align);
    return n++;
  }
  size_t total() const { return lay.total(); }
  hipError_t reserve(PinnedBuffer& pinned, DeviceBuffer& dev) {
    hipError_t e = pinned.reserve(total());
    if (e == hipSuccess) e = dev.reserve(total());
    if (e != hipSuccess) return e;
    h = (uint8_t*)pinned.ptr; d = (uint8_t*)dev.ptr;
    return hipSuccess;
  }
  hipError_t fetch(hipStream_t s) { return hipMemcpyAsync(h, d, total(), hipMemcpyDeviceToHost, s); }
  template <class T> T* dev(int p) const { return (T*)(d + at[p]); }
  template <class T> const T* host(int p) const { return (const T*)(h + at[p]); }
};

}  // namespace bpsw
