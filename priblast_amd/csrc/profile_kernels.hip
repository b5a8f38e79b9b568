// The per-position interaction profile of each query on gfx950 (prb_search_page_profile, prb_profset_merge, `ris -q`).
// The reference has no counterpart: the rows are defined in include/priblast_hip.h.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// ---- per-position profile (prb_search_page_profile) ----
// Every column is an integer count, a minimum or a lexicographic minimum, built with integer atomics only, so the table
// does not depend on the order in which hits, sub-batches or pages arrive.  A hit's span is [min(q0, qN), max(q0, qN)]
// of its `-s 0` end pairs (q0 <= qN except for the unsorted first hit of a list).  The kernels run a lane
// per hit over the whole grid (a query's hits spread over many workgroups); a lane walks its span, which is short (tens
// of positions), and the atomics of the minima are skipped wherever the value already there is not larger.
__device__ __forceinline__ void prof_span(const int32_t *ends, int64_t h, int32_t &lo, int32_t &hi) {
  const int32_t a = ends[4 * h], b = ends[4 * h + 2];
  lo = min(a, b);
  hi = max(a, b);
}
// the slots of hit h's span: first slot, or -1 (and `bad` raised) when the span lies outside its query
__device__ __forceinline__ int64_t prof_base(const ProfTab &t, int32_t q, int32_t lo, int32_t hi) {
  if (q < 0 || q >= t.nq || lo < 0 || (int64_t)hi >= t.off[q + 1] - t.off[q] - 1) {
    atomicOr(t.bad, 1u);
    return -1;
  }
  return t.off[q];
}
__device__ __forceinline__ unsigned long long prof_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t prof_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_prof_keys(int64_t n, const uint32_t *__restrict__ start, int64_t npairs,
                                                      const int32_t *__restrict__ ends, uint64_t *key, uint32_t *val) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int64_t lo = 0, hi = npairs; // the last pair that starts at or before i
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if ((int64_t)start[m] <= i) lo = m;
    else hi = m;
  }
  int32_t a, b;
  prof_span(ends, i, a, b);
  key[i] = ((uint64_t)lo << 32) | (uint32_t)a;
  val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_prof_span(int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                      const int32_t *__restrict__ ends, uint64_t *v) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int32_t a, b;
  prof_span(ends, val[i], a, b);
  v[i] = (key[i] & 0xFFFFFFFF00000000ull) | (uint32_t)max(b + 1, 0);
}

// Hits sorted by (pair, first position): m[i - 1] of the same pair holds 1 + the furthest position that the pair's
// earlier hits reach, so [max(lo, that), hi] is what hit i adds to the union of the pair's spans (nothing if empty).
__global__ __launch_bounds__(kBlock) void k_prof_add(HitSoA h, int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                     const uint64_t *__restrict__ m, const int32_t *__restrict__ ends, ProfTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = val[i];
  int32_t lo, hi;
  prof_span(ends, x, lo, hi);
  const int64_t base = prof_base(t, h.query[x], lo, hi);
  if (base < 0) return;
  atomicAdd(&t.hdiff[base + lo], 1ull);
  atomicAdd(&t.hdiff[base + hi + 1], ~0ull);
  int32_t from = lo;
  if (i > 0 && (m[i - 1] >> 32) == (key[i] >> 32)) from = max(lo, (int32_t)(uint32_t)m[i - 1]);
  if (from <= hi) {
    atomicAdd(&t.tdiff[base + from], 1);
    atomicAdd(&t.tdiff[base + hi + 1], -1);
  }
}

// pass 0: skey = min energy key; pass 1 (after pass 0 has finished): stie = min place among the hits at that key
template <int kPass>
__global__ __launch_bounds__(kBlock) void k_prof_min(HitSoA h, int64_t n, const uint32_t *__restrict__ val, const int32_t *__restrict__ ends,
                                                     ProfTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = val[i]; // (in span order: neighbouring lanes walk neighbouring positions)
  int32_t lo, hi;
  prof_span(ends, x, lo, hi);
  const int64_t base = prof_base(t, h.query[x], lo, hi);
  if (base < 0) return;
  const unsigned long long ek = energy_key(h.e_tot[x]);
  for (int64_t p = base + lo; p <= base + hi; p++) {
    if (kPass == 0) {
      if (ek < prof_load(&t.skey[p])) atomicMin(&t.skey[p], ek); // (the value only falls: a skipped atomic would not have won)
    } else if (t.skey[p] == ek && x < prof_load(&t.stie[p])) {
      atomicMin(&t.stie[p], x);
    }
  }
}

// A slot the sub-batch covers takes the sub-batch's best hit if (key, page << 32 | place) is below the table's.  The
// sub-batch's list is gone once the page is done, so the hit's fields are copied now.
__global__ __launch_bounds__(kBlock) void k_prof_merge(HitSoA h, const int32_t *__restrict__ ends, ProfTab t, int64_t p0, int64_t p1,
                                                       int32_t page) {
  const int64_t p = p0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= p1) return;
  const unsigned long long sk = t.skey[p];
  if (sk == ~0ull) return; // (not covered in this sub-batch: the scratch is untouched)
  const uint32_t x = t.stie[p];
  const unsigned long long tie = ((unsigned long long)(uint32_t)page << 32) | x;
  const unsigned long long k = t.key[p];
  if (sk < k || (sk == k && tie < t.tie[p])) {
    t.key[p] = sk;
    t.tie[p] = tie;
    t.e_min[p] = h.e_tot[x];
    t.db_id[p] = h.db_id[x];
#pragma unroll
    for (int c = 0; c < 4; c++) t.bp[4 * p + c] = ends[4 * x + c];
  }
  t.skey[p] = ~0ull;
  t.stie[p] = ~0u;
}

// prb_profset_merge: the table s, over other pages of the same batch, into t, a lane per slot.  The difference arrays
// add (no page is in both, so no (page, db_id) is counted twice among the targets); the best hit is the lower of the two
// (key, tie) pairs.
__global__ __launch_bounds__(kBlock) void k_prof_join(ProfTab t, ProfTab s, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p == 0 && *s.bad) *t.bad = 1u;
  if (p >= P) return;
  t.hdiff[p] += s.hdiff[p];
  t.tdiff[p] += s.tdiff[p];
  const unsigned long long sk = s.key[p], st = s.tie[p], k = t.key[p];
  if (sk < k || (sk == k && st < t.tie[p])) {
    t.key[p] = sk;
    t.tie[p] = st;
    t.e_min[p] = s.e_min[p];
    t.db_id[p] = s.db_id[p];
#pragma unroll
    for (int c = 0; c < 4; c++) t.bp[4 * p + c] = s.bp[4 * p + c];
  }
}

__global__ __launch_bounds__(kBlock) void k_prof_rows(ProfTab t, const uint32_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ hits,
                                                      const int32_t *__restrict__ targets, prb_profile_pos *rows) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int64_t p = idx[j];
  int32_t lo = 0, hi = t.nq; // the query whose slots hold p
  while (hi - lo > 1) {
    const int32_t m = (lo + hi) >> 1;
    if (t.off[m] <= p) lo = m;
    else hi = m;
  }
  prb_profile_pos r;
  r.query = lo;
  r.pos = (int32_t)(p - t.off[lo]);
  r.hits = hits[p];
  r.targets = targets[p];
  r.page = (int32_t)(t.tie[p] >> 32);
  r.db_id = t.db_id[p];
  r.reserved = 0;
  r.e_min = t.e_min[p];
  r.bp_first[0] = t.bp[4 * p];
  r.bp_first[1] = t.bp[4 * p + 1];
  r.bp_last[0] = t.bp[4 * p + 2];
  r.bp_last[1] = t.bp[4 * p + 3];
  rows[j] = r;
}

} // namespace

hipError_t launch_prof_keys(int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, uint64_t *key, uint32_t *val,
                            hipStream_t s) {
  return launch_1d(k_prof_keys, n, kBlock, 0, s, n, start, npairs, ends, key, val);
}
hipError_t launch_prof_span(int64_t n, const uint64_t *key, const uint32_t *val, const int32_t *ends, uint64_t *v, hipStream_t s) {
  return launch_1d(k_prof_span, n, kBlock, 0, s, n, key, val, ends, v);
}
hipError_t launch_prof_add(const HitSoA &h, int64_t n, const uint64_t *key, const uint32_t *val, const uint64_t *m, const int32_t *ends,
                           const ProfTab &t, hipStream_t s) {
  return launch_1d(k_prof_add, n, kBlock, 0, s, h, n, key, val, m, ends, t);
}
hipError_t launch_prof_min(const HitSoA &h, int64_t n, const uint32_t *val, const int32_t *ends, const ProfTab &t, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_min<0>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, h, n, val, ends, t);
  hipLaunchKernelGGL(k_prof_min<1>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, h, n, val, ends, t);
  return hipGetLastError(); // (one report for the two launches)
}
hipError_t launch_prof_merge(const HitSoA &h, const int32_t *ends, const ProfTab &t, int64_t p0, int64_t p1, int32_t page,
                             hipStream_t s) {
  return launch_1d(k_prof_merge, p1 - p0, kBlock, 0, s, h, ends, t, p0, p1, page);
}
hipError_t launch_prof_join(const ProfTab &t, const ProfTab &src, int64_t P, hipStream_t s) {
  return launch_1d(k_prof_join, P, kBlock, 0, s, t, src, P);
}
hipError_t launch_prof_rows(const ProfTab &t, const uint32_t *idx, int64_t n, const int64_t *hits, const int32_t *targets, void *rows,
                            hipStream_t s) {
  return launch_1d(k_prof_rows, n, kBlock, 0, s, t, idx, n, hits, targets, static_cast<prb_profile_pos *>(rows));
}

} // namespace prb
