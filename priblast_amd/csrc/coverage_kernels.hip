// The per-position coverage of every target and its regions on gfx950 (prb_search_page_coverage, prb_covset_add_hits,
// prb_covset_merge, prb_covset_finish, `ris -c D`).  The reference has no counterpart: the columns and the records are
// defined in include/priblast_hip.h.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// ---- the merge of a list of final hits of one page (prb_search_page_coverage, prb_covset_add_hits) ----
// The `-q` construction (profile_kernels.hip) turned round: the slots are the characters of the page's text, a hit's span
// is [min(db0, dbN), max(db0, dbN)] of its `-s 0` end pairs, and what is counted once per position is the query's
// identifier.  Every column is an integer count, a minimum or a lexicographic minimum, built with integer atomics only.
// A lane per hit; a lane walks its span, which is short (tens of positions).
struct CovSpan {
  int64_t base; // the page's first slot; -1 (and `bad` raised): the span leaves its sequence
  int32_t lo, hi;
};
__device__ __forceinline__ CovSpan cov_span(const CovTab &t, const CovPage &pg, const int32_t *db_id, const int32_t *ends, int64_t h) {
  CovSpan s;
  const int32_t a = ends[4 * h + 1], b = ends[4 * h + 3], d = db_id[h];
  s.lo = min(a, b);
  s.hi = max(a, b);
  s.base = pg.slot0;
  bool ok = d >= 0 && d < pg.nseq;
  if (ok) {
    const int64_t first = t.seq_lo[pg.target0 + d] - pg.slot0, behind = t.seq_lo[pg.target0 + d + 1] - pg.slot0 - 1; // (the separator)
    ok = (int64_t)s.lo >= first && (int64_t)s.hi < behind;
  }
  if (!ok) {
    atomicOr(t.bad, 1u);
    s.base = -1;
  }
  return s;
}
__device__ __forceinline__ unsigned long long cov_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// key = query (index in the call's batch) << 32 | first position of the span in the page's text, val = the hit,
// place = its index among its query's hits (the list is ascending by query)
__global__ __launch_bounds__(kBlock) void k_cov_keys(int64_t n, const int32_t *__restrict__ query, const int32_t *__restrict__ db_id,
                                                     const int32_t *__restrict__ ends, CovTab t, CovPage pg, uint64_t *key, uint32_t *val,
                                                     uint32_t *place) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t q = query[i];
  int64_t lo = -1, hi = i; // the first hit of query q: query[lo] < q <= query[hi]
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (query[m] < q) lo = m;
    else hi = m;
  }
  const CovSpan s = cov_span(t, pg, db_id, ends, i);
  key[i] = ((uint64_t)(uint32_t)q << 32) | (s.base < 0 ? 0u : (uint32_t)s.lo);
  val[i] = (uint32_t)i;
  place[i] = (uint32_t)(i - hi);
}

// v = query << 32 | 1 + last position of the span: what the max-scan takes.  Sequences end in a separator that no span
// reaches, so within a query the running maximum of one sequence never passes the first position of the next one.
__global__ __launch_bounds__(kBlock) void k_cov_span(int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                     const int32_t *__restrict__ db_id, const int32_t *__restrict__ ends, CovTab t, CovPage pg,
                                                     uint64_t *v) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const CovSpan s = cov_span(t, pg, db_id, ends, val[i]);
  v[i] = (key[i] & 0xFFFFFFFF00000000ull) | (s.base < 0 ? 0u : (uint32_t)(s.hi + 1));
}

// Hits sorted by (query, first position): m[i - 1] of the same query holds 1 + the furthest position that the query's
// earlier hits reach, so [max(lo, that), hi] is what hit i adds to the union of the query's spans (nothing if empty).
__global__ __launch_bounds__(kBlock) void k_cov_add(int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                    const uint64_t *__restrict__ m, const int32_t *__restrict__ db_id,
                                                    const int32_t *__restrict__ ends, CovTab t, CovPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const CovSpan s = cov_span(t, pg, db_id, ends, val[i]);
  if (s.base < 0) return;
  atomicAdd(&t.hdiff[s.base + s.lo], 1ull);
  atomicAdd(&t.hdiff[s.base + s.hi + 1], ~0ull);
  atomicAdd(&t.starts[s.base + s.lo], 1u);
  int32_t from = s.lo;
  if (i > 0 && (m[i - 1] >> 32) == (key[i] >> 32)) from = max(s.lo, (int32_t)(uint32_t)m[i - 1]);
  if (from <= s.hi) {
    atomicAdd(&t.qdiff[s.base + from], 1);
    atomicAdd(&t.qdiff[s.base + s.hi + 1], -1);
  }
}

// pass 0: skey = min energy key; pass 1 (after pass 0 has finished): stie = min (identifier, place) among the hits at
// that key; pass 2 (after pass 1): the one hit that holds both takes the slot over if it is below the table's best hit -
// it is the slot's only writer; pass 3 (after pass 2): the scratch of the covered slots back to "none"
template <int kPass>
__global__ __launch_bounds__(kBlock) void k_cov_min(int64_t n, const uint32_t *__restrict__ val, const int32_t *__restrict__ query,
                                                    const int32_t *__restrict__ db_id, const double *__restrict__ e_tot,
                                                    const int32_t *__restrict__ ends, const uint32_t *__restrict__ place,
                                                    const int32_t *__restrict__ ids, CovTab t, CovPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = val[i]; // (in span order: neighbouring lanes walk neighbouring positions)
  const CovSpan s = cov_span(t, pg, db_id, ends, x);
  if (s.base < 0) return;
  const unsigned long long ek = energy_key(e_tot[x]);
  const unsigned long long tie = ((unsigned long long)(uint32_t)ids[query[x]] << 32) | place[x];
  for (int64_t p = s.base + s.lo; p <= s.base + s.hi; p++) {
    if (kPass == 0) {
      if (ek < cov_load(&t.skey[p])) atomicMin(&t.skey[p], ek); // (the value only falls: a skipped atomic would not have won)
    } else if (kPass == 1) {
      if (t.skey[p] == ek && tie < cov_load(&t.stie[p])) atomicMin(&t.stie[p], tie);
    } else if (kPass == 2) {
      if (t.skey[p] != ek || t.stie[p] != tie) continue;
      const unsigned long long k = t.key[p];
      if (ek < k || (ek == k && tie < t.tie[p])) {
        t.key[p] = ek;
        t.tie[p] = tie;
        t.e_min[p] = e_tot[x];
#pragma unroll
        for (int c = 0; c < 4; c++) t.bp[4 * p + c] = ends[4 * x + c];
      }
    } else {
      t.skey[p] = ~0ull; // (every hit that covers the slot writes the same)
      t.stie[p] = ~0ull;
    }
  }
}

// prb_covset_merge: the table s, over other (identifier, page) sets of the same database, into t, a lane per slot.  The
// difference and start arrays add (no identifier is in both for a page, so none is counted twice among the queries); the
// best hit is the lower of the two (key, tie) pairs.
__global__ __launch_bounds__(kBlock) void k_cov_join(CovTab t, CovTab s, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p == 0 && *s.bad) *t.bad = 1u;
  if (p >= P) return;
  t.hdiff[p] += s.hdiff[p];
  t.qdiff[p] += s.qdiff[p];
  t.starts[p] += s.starts[p];
  const unsigned long long sk = s.key[p], st = s.tie[p], k = t.key[p];
  if (sk < k || (sk == k && st < t.tie[p])) {
    t.key[p] = sk;
    t.tie[p] = st;
    t.e_min[p] = s.e_min[p];
#pragma unroll
    for (int c = 0; c < 4; c++) t.bp[4 * p + c] = s.bp[4 * p + c];
  }
}

// ---- the regions (prb_covset_finish) ----
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor(v, o);
  return v;
}

// A wavefront per region: region r begins at slot first[r] (a head: queries >= D there and below D in front of it) and
// runs to the first slot below D, at the latest the separator behind its sequence, whose counts are 0.  The lanes take
// the region's slots 64 at a time and keep their own sums, maxima and lexicographic minima; one butterfly per column at
// the end, no atomics, and lane 0 writes the record.  Counts are added and compared as integers, so the record does not
// depend on which lane saw what.
__global__ __launch_bounds__(kBlock) void k_cov_regions(CovTab t, const int64_t *__restrict__ tbase, int32_t npages, int64_t ntargets,
                                                        const uint32_t *__restrict__ first, int64_t nregions, const int64_t *__restrict__ hits,
                                                        const int32_t *__restrict__ queries, int32_t D, prb_target_region *out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (r >= nregions) return; // (a whole wavefront)
  const int64_t p0 = first[r];
  int64_t lo = 0, hi = ntargets; // the target whose slots hold p0
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (t.seq_lo[m] <= p0) lo = m;
    else hi = m;
  }
  const int64_t tg = lo, s0 = t.seq_lo[tg], sep = t.seq_lo[tg + 1] - 1;
  unsigned long long sum = 0, mh = 0, mq = 0, bk = ~0ull, bt = ~0ull, bp = ~0ull, last = 0;
  for (int64_t base = p0; base < sep; base += 64) {
    const int64_t p = base + lane;
    const bool in = p < sep && queries[p] >= D;
    const unsigned long long out_mask = __ballot(!in);
    const int run = out_mask ? __builtin_ctzll(out_mask) : 64; // the lanes in front of the first slot outside
    if (lane < run) {
      sum += t.starts[p];
      mh = max(mh, (unsigned long long)hits[p]);
      // (the highest text position among the deepest ones: the lowest forward position)
      mq = max(mq, ((unsigned long long)(uint32_t)queries[p] << 32) | (uint32_t)(p - s0));
      const unsigned long long k = t.key[p], e = t.tie[p];
      if (k < bk || (k == bk && e < bt)) {
        bk = k;
        bt = e;
        bp = (unsigned long long)p;
      }
      last = (unsigned long long)p;
    }
    if (run < 64) break;
  }
  sum = wave_sum(sum);
  mh = wave_max(mh);
  mq = wave_max(mq);
  last = wave_max(last);
  // the best hit: the lowest key, among its slots the lowest tie, among those the lowest slot (all hold the same hit)
  const unsigned long long k_min = wave_min(bk);
  const unsigned long long t_min = wave_min(bk == k_min ? bt : ~0ull);
  const unsigned long long p_min = wave_min(bk == k_min && bt == t_min ? bp : ~0ull);
  if (lane != 0) return;
  int32_t pl = 0, ph = npages; // the page of the target
  while (ph - pl > 1) {
    const int32_t m = (pl + ph) >> 1;
    if (tbase[m] <= tg) pl = m;
    else ph = m;
  }
  const int64_t len = sep - s0;
  prb_target_region x;
  x.page = pl;
  x.db_id = (int32_t)(tg - tbase[pl]);
  x.start = (int32_t)(len - 1 - ((int64_t)last - s0)); // (the text is the reversed sequence)
  x.end = (int32_t)(len - 1 - (p0 - s0));
  x.hits = (int64_t)sum;
  x.max_hits = (int64_t)mh;
  x.max_queries = (int32_t)(mq >> 32);
  x.peak = (int32_t)(len - 1 - (int64_t)(uint32_t)mq);
  x.e_min = t.e_min[p_min];
  x.query = (int32_t)(t_min >> 32);
  x.reserved = 0;
  x.bp_first[0] = t.bp[4 * p_min];
  x.bp_first[1] = t.bp[4 * p_min + 1];
  x.bp_last[0] = t.bp[4 * p_min + 2];
  x.bp_last[1] = t.bp[4 * p_min + 3];
  out[r] = x;
}

} // namespace

hipError_t launch_cov_keys(const CovHits &h, const CovTab &t, const CovPage &pg, uint64_t *key, uint32_t *val, uint32_t *place, hipStream_t s) {
  return launch_1d(k_cov_keys, h.n, kBlock, 0, s, h.n, h.query, h.db_id, h.ends, t, pg, key, val, place);
}
hipError_t launch_cov_span(const CovHits &h, const uint64_t *key, const uint32_t *val, const CovTab &t, const CovPage &pg, uint64_t *v,
                           hipStream_t s) {
  return launch_1d(k_cov_span, h.n, kBlock, 0, s, h.n, key, val, h.db_id, h.ends, t, pg, v);
}
hipError_t launch_cov_add(const CovHits &h, const uint64_t *key, const uint32_t *val, const uint64_t *m, const CovTab &t, const CovPage &pg,
                          hipStream_t s) {
  return launch_1d(k_cov_add, h.n, kBlock, 0, s, h.n, key, val, m, h.db_id, h.ends, t, pg);
}
hipError_t launch_cov_min(const CovHits &h, const uint32_t *val, const uint32_t *place, const int32_t *ids, const CovTab &t, const CovPage &pg,
                          hipStream_t s) {
  if (h.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((h.n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(k_cov_min<0>, grid, block, 0, s, h.n, val, h.query, h.db_id, h.e_tot, h.ends, place, ids, t, pg);
  hipLaunchKernelGGL(k_cov_min<1>, grid, block, 0, s, h.n, val, h.query, h.db_id, h.e_tot, h.ends, place, ids, t, pg);
  hipLaunchKernelGGL(k_cov_min<2>, grid, block, 0, s, h.n, val, h.query, h.db_id, h.e_tot, h.ends, place, ids, t, pg);
  hipLaunchKernelGGL(k_cov_min<3>, grid, block, 0, s, h.n, val, h.query, h.db_id, h.e_tot, h.ends, place, ids, t, pg);
  return hipGetLastError(); // (one report for the four launches)
}
hipError_t launch_cov_join(const CovTab &t, const CovTab &src, int64_t P, hipStream_t s) {
  return launch_1d(k_cov_join, P, kBlock, 0, s, t, src, P);
}
hipError_t launch_cov_regions(const CovTab &t, const int64_t *tbase, int32_t npages, int64_t ntargets, const uint32_t *first, int64_t nregions,
                              const int64_t *hits, const int32_t *queries, int32_t D, void *out, hipStream_t s) {
  return launch_1d(k_cov_regions, nregions * 64, kBlock, 0, s, t, tbase, npages, ntargets, first, nregions, hits, queries, D,
                   static_cast<prb_target_region *>(out));
}

} // namespace prb
