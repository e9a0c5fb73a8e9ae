// bpsw_klib_sort.h -- the tie order of klib's ks_introsort, restated once for every host list that the reference sorts with it
// (regions in bpsw_rescue.cpp, chain weights in bpsw_chain.cpp).
#pragma once

#include <stddef.h>

#include <utility>
#include <vector>

namespace bpsw {

template <class T, class Lt>
void insertion_sort(T* first, T* last, Lt lt) {  // stable
  for (T* i = first + 1; i < last; ++i)
    for (T* j = i; j > first && lt(*j, *(j - 1)); --j) std::swap(*j, *(j - 1));
}

template <class T, class Lt>
void comb_sort(size_t n, T* a, Lt lt) {  // fallback of klib's introsort, native/ksort.h:154-175
  const double shrink = 1.2473309501039786540366528676643;
  size_t gap = n;
  bool swapped;
  do {
    if (gap > 2) {
      gap = (size_t)(gap / shrink);
      if (gap == 9 || gap == 10) gap = 11;
    }
    swapped = false;
    for (T* i = a; i < a + n - gap; ++i)
      if (lt(*(i + gap), *i)) { std::swap(*i, *(i + gap)); swapped = true; }
  } while (swapped || gap > 2);
  if (gap != 1) insertion_sort(a, a + n, lt);
}

// The C library's tie order is a property of klib's ks_introsort (native/ksort.h:176-227): median of
// (first, middle+1, last) as pivot moved to the end, Hoare partition, sub-ranges of <= 16 elements left
// for one final insertion sort, comb sort when the depth budget runs out.  To hand the caller the same
// order as jniNative.so does, the same sequence of comparisons and swaps is performed here.
template <class T, class Lt>
void klib_order_sort(size_t n, T* a, Lt lt) {
  struct Frame { T *lo, *hi; int depth; };
  if (n < 1) return;
  if (n == 2) {
    if (lt(a[1], a[0])) std::swap(a[0], a[1]);
    return;
  }
  int d = 2;
  while ((1ul << d) < n) ++d;
  std::vector<Frame> stack;
  stack.reserve(sizeof(size_t) * (size_t)d + 2);
  T *s = a, *t = a + (n - 1);
  d <<= 1;
  for (;;) {
    if (s < t) {
      if (--d == 0) { comb_sort((size_t)(t - s) + 1, s, lt); t = s; continue; }
      T *i = s, *j = t, *k = i + ((j - i) >> 1) + 1;
      if (lt(*k, *i)) { if (lt(*k, *j)) k = j; }
      else k = lt(*j, *i) ? i : j;
      const T pivot = *k;
      if (k != t) std::swap(*k, *t);
      for (;;) {
        do ++i; while (lt(*i, pivot));
        do --j; while (i <= j && lt(pivot, *j));
        if (j <= i) break;
        std::swap(*i, *j);
      }
      std::swap(*i, *t);
      if (i - s > t - i) {
        if (i - s > 16) stack.push_back({s, i - 1, d});
        s = t - i > 16 ? i + 1 : t;
      } else {
        if (t - i > 16) stack.push_back({i + 1, t, d});
        t = i - s > 16 ? i - 1 : s;
      }
    } else {
      if (stack.empty()) { insertion_sort(a, a + n, lt); return; }
      s = stack.back().lo; t = stack.back().hi; d = stack.back().depth;
      stack.pop_back();
    }
  }
}

}  // namespace bpsw
