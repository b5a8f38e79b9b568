// What the kernels that work on the (pair run, feature of its target) items of a list of final hits share
// (feature_kernels.hip, fnull_kernels.hip): a hit's span in the page's text, a pair's run, and the run of an item.
#pragma once
#include "search_kernels.hpp"

namespace prb {

// the span of hit i in the page's text, or ok = false (and `bad` raised): it leaves sequence d
struct FeatSpan {
  int32_t lo, hi;
  bool ok;
};
__device__ __forceinline__ FeatSpan feat_span(const FeatHits &h, const FeatPage &pg, int32_t d, int64_t i, uint32_t *bad) {
  FeatSpan s;
  const int32_t a = h.ends[4 * i + 1], b = h.ends[4 * i + 3];
  s.lo = min(a, b);
  s.hi = max(a, b);
  const int32_t s0 = pg.slo[d];
  s.ok = s.lo >= s0 && (int64_t)s.hi < (int64_t)s0 + pg.slen[d];
  if (!s.ok) atomicOr(bad, 1u);
  return s;
}
// the run [a, b) of pair k, its target d (or -1: the run names a query or a sequence outside the page)
struct FeatRun {
  int64_t a, b;
  int32_t d;
};
__device__ __forceinline__ FeatRun feat_run(const FeatHits &h, const uint32_t *__restrict__ start, int64_t npairs, int64_t k) {
  FeatRun r;
  r.a = start[k];
  r.b = k + 1 < npairs ? (int64_t)start[k + 1] : h.n;
  r.d = -1;
  if (r.a < 0 || r.a >= r.b || r.b > h.n) r.b = r.a; // (an empty run: nothing is read)
  else r.d = h.db_id[r.a];
  return r;
}
// the run that holds item x: the last k with ioff[k] <= x (runs without a feature share their offset with the next one)
__device__ __forceinline__ int64_t item_run(const int64_t *__restrict__ ioff, int64_t npairs, int64_t x) {
  int64_t lo = 0, hi = npairs; // ioff[lo] <= x < ioff[hi]
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (ioff[m] <= x) lo = m;
    else hi = m;
  }
  return lo;
}

} // namespace prb
