// The (query, database sequence) runs of a final, sorted hit list on gfx950: their heads, the per-pair summaries
// (prb_search_page_summary; also what the top-N pair table and the profile start from) and the distinct interaction
// sites of each pair (prb_ris_opts::distinct_sites, `ris -u`).  The reference has no counterpart: the records and the
// selection rule are defined in include/priblast_hip.h.
#include <algorithm>

#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// ---- per-pair summaries ----
// The final list is sorted by query, then db_sp, and a database sequence is one contiguous range of the page text
// (db_id = seq_of(db_sp)), so the hits of a (query, db_id) pair are one run of the list.
__global__ __launch_bounds__(kBlock) void k_pair_heads(const int32_t *__restrict__ query, const int32_t *__restrict__ db_id,
                                                       int64_t n, uint8_t *head) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  head[i] = i == 0 || query[i] != query[i - 1] || db_id[i] != db_id[i - 1];
}

// A lane walks its pair's run in list order: strict `<` keeps the first minimum, the sum is the left-to-right one.
// (A lane per pair: the skew of the run lengths is in DESIGN.md §4.)
__global__ __launch_bounds__(kBlock) void k_pair_fold(HitSoA h, int64_t n, const uint32_t *__restrict__ start, int64_t npairs,
                                                      const int32_t *__restrict__ ends, prb_pair_summary *out) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= npairs) return;
  const int64_t a = start[k], b = k + 1 < npairs ? (int64_t)start[k + 1] : n;
  double sum = 0.0, mn = h.e_tot[a];
  int64_t best = a;
  for (int64_t i = a; i < b; i++) {
    const double e = h.e_tot[i];
    sum += e;
    if (e < mn) {
      mn = e;
      best = i;
    }
  }
  prb_pair_summary r;
  r.query = h.query[a];
  r.db_id = h.db_id[a];
  r.hits = b - a;
  r.e_min = mn;
  r.e_sum = sum;
  r.e_acc = h.e_acc[best];
  r.e_hyb = h.e_hyb[best];
  r.bp_first[0] = ends[4 * best];
  r.bp_first[1] = ends[4 * best + 1];
  r.bp_last[0] = ends[4 * best + 2];
  r.bp_last[1] = ends[4 * best + 3];
  out[k] = r;
}

// ---- distinct interaction sites (prb_ris_opts::distinct_sites, `ris -u`) ----
// Greedy non-maximum suppression inside every (query, db_id) run of the final list (the rule: include/priblast_hip.h),
// in its fix-point form: a hit is kept once every intersecting hit before it in the order (e_tot, place) is dropped, and
// dropped once one of them is kept.  The first undecided hit of the order has only decided hits before it, so every
// round decides it at least: a run of L hits is done after at most L rounds, and every loop below has that bound.
// Decisions are final and never wrong whenever they are taken, so a round may read states that the same round writes.
__device__ __forceinline__ int4 site_rect(const HitSoA &h, int64_t i) { // inclusive ends: (q0, q1, db0, db1)
  const int q = h.q_sp[i], d = h.db_sp[i];
  return make_int4(q, q + h.q_len[i] - 1, d, d + h.db_len[i] - 1);
}
__device__ __forceinline__ bool site_intersect(const int4 &a, const int4 &b) {
  return a.x <= b.y && b.x <= a.y && a.z <= b.w && b.z <= a.w;
}
// hit j comes before hit i: e_tot ascending, compared as doubles (-0.0 == +0.0), then the place in the list
__device__ __forceinline__ bool site_before(double ej, int j, double ei, int i) { return ej < ei || (ej == ei && j < i); }

// Runs of up to 64 hits (fourteen on average, most of them one to thirty), several per wavefront: a wavefront (= a
// workgroup) owns the runs that start in its slice of 64 hits and lays 64 consecutive hits from the first of them over
// its lanes; a run that does not end inside that window opens a second one (two windows always reach the end of the
// slice's runs: whatever the second one leaves open starts behind the slice).  Per window: the run of each lane from
// the ballot of the head flags; if all runs are singletons nothing else happens; else rectangles and energies go
// through 1.5 KB of LDS once, every lane collects the mask of the lanes before it in the order that intersect it, and
// the rounds are three ballots and a few mask operations each.  Runs longer than short_max (<= 64) are appended to
// long_list for k_site_select_long.
__global__ __launch_bounds__(64) void k_site_select_packed(HitSoA h, int64_t n, const uint8_t *__restrict__ head, int short_max,
                                                           uint8_t *__restrict__ keep, uint32_t *__restrict__ long_list, uint32_t *nlong) {
  __shared__ int4 rect_s[64];
  __shared__ double key_s[64];
  const int lane = threadIdx.x;
  const int64_t slice0 = (int64_t)blockIdx.x * 64, slice1 = min(n, slice0 + 64);
  const uint64_t starts = __ballot(slice0 + lane < n && head[min(slice0 + lane, n - 1)] != 0);
  if (starts == 0) return; // (the slice lies inside a run that began before it)
  int64_t base = slice0 + __builtin_ctzll(starts);
  for (int pass = 0; pass < 2 && base < slice1; pass++) {
    const int wlen = (int)min((int64_t)64, n - base);
    const bool valid = lane < wlen;
    const int64_t i = valid ? base + lane : base;
    const uint64_t heads = __ballot(valid && head[i] != 0); // (bit 0 is set)
    const bool closed = base + 64 >= n || head[base + 64] != 0; // the window's last run ends with the window
    // the run of this lane, as lanes [ls, le)
    const int ls = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
    const uint64_t above = lane < 63 ? heads >> (lane + 1) : 0;
    const int le = above ? lane + 1 + __builtin_ctzll(above) : wlen;
    const int len = le - ls;
    const bool whole = le < wlen || closed;
    const bool mine = valid && base + ls < slice1;
    // the run that does not end inside the window (only the last one can): from lane 0 on it is longer than a wavefront,
    // else the next window starts with it
    const uint64_t open = __ballot(mine && !whole && lane == ls);
    const bool packed = mine && whole && len <= short_max;
    if (mine && lane == ls && (whole ? len > short_max : ls == 0)) long_list[atomicAdd(nlong, 1u)] = (uint32_t)(base + ls);
    uint8_t st = 1; // a singleton is kept
    if (__ballot(packed && len > 1) != 0) {
      if (valid) {
        rect_s[lane] = site_rect(h, i);
        key_s[lane] = h.e_tot[i];
      }
      __syncthreads();
      int maxlen = packed ? len : 0;
      for (int o = 32; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
      const int4 r = rect_s[valid ? lane : 0];
      const double e = key_s[valid ? lane : 0];
      uint64_t before = 0; // the lanes of the run that intersect this one and come before it in the order
      for (int k = 0; k < maxlen; k++) {
        const int j = ls + k;
        if (packed && k < len && j != lane && site_intersect(r, rect_s[j]) && site_before(key_s[j], j, e, lane)) before |= 1ull << j;
      }
      uint64_t kept = 0, dropped = 0;
      st = 0;
      for (int round = 0; round < maxlen; round++) {
        if (packed && st == 0) {
          if (before & kept) st = 2;
          else if ((before & ~dropped) == 0) st = 1;
        }
        kept = __ballot(packed && st == 1);
        dropped = __ballot(packed && st == 2);
        if (__ballot(packed && st == 0) == 0) break;
      }
      __syncthreads(); // (the next window writes the same LDS)
    }
    if (packed) keep[i] = st == 1;
    if (open == 0 || (open & 1)) break; // nothing open, or the long run: whatever follows starts behind the slice
    base += __builtin_ctzll(open);
  }
}

// A run's rectangles, energies and state, indexed from the run's first hit: in the workgroup's LDS ...
struct SiteLds {
  int4 *rect;
  double *key;
  int32_t *lo;
  uint16_t *hi;
  volatile uint8_t *st;
  __device__ __forceinline__ int4 r(int k) const { return rect[k]; }
  __device__ __forceinline__ double e(int k) const { return key[k]; }
  __device__ __forceinline__ int d0(int k) const { return rect[k].z; }
  __device__ __forceinline__ int get_hi(int k) const { return hi[k]; }
  __device__ __forceinline__ void set_hi(int k, int v) const { hi[k] = (uint16_t)v; }
};
// ... or, for a run beyond the LDS capacity, read from the list itself with the state in HBM scratch (through the L2:
// a workgroup's run is a few hundred KB)
struct SiteHbm {
  HitSoA h; // from the run's first hit on
  int32_t *lo, *hi;
  volatile uint8_t *st;
  __device__ __forceinline__ int4 r(int k) const { return site_rect(h, k); }
  __device__ __forceinline__ double e(int k) const { return h.e_tot[k]; }
  __device__ __forceinline__ int d0(int k) const { return h.db_sp[k]; }
  __device__ __forceinline__ int get_hi(int k) const { return hi[k]; }
  __device__ __forceinline__ void set_hi(int k, int v) const { hi[k] = v; }
};

constexpr int kSiteBlock = 256;

// One run of L hits by one workgroup, the hits dealt round-robin to its threads.  The search's list is sorted by db_sp,
// so hit k can intersect only a window [lo, hi) of its run: hi = the first hit behind k that starts behind k's target
// interval, lo = the first hit whose own window reaches k (an atomicMin from every such hit while it looks for its
// hi).  A caller's list (prb_distinct_sites) need not be sorted: then the window is the run.  state: 0 undecided,
// 1 kept, 2 dropped.
template <class S> __device__ void site_select_run(const S &s, int L, uint8_t *__restrict__ keep) {
  const int tid = threadIdx.x;
  int unsorted = 0;
  for (int k = tid; k < L; k += kSiteBlock) {
    if (k + 1 < L) unsorted |= s.d0(k + 1) < s.d0(k);
    s.lo[k] = k;
    s.st[k] = 0;
  }
  unsorted = __syncthreads_or(unsorted);
  for (int k = tid; k < L; k += kSiteBlock) {
    int j = L;
    if (unsorted) {
      s.lo[k] = 0;
    } else {
      const int d1 = s.r(k).w;
      for (j = k + 1; j < L; j++) {
        if (s.d0(j) > d1) break;
        atomicMin(&s.lo[j], k);
      }
    }
    s.set_hi(k, j);
  }
  __syncthreads();
  for (int round = 0; round < L; round++) {
    int undecided = 0;
    for (int k = tid; k < L; k += kSiteBlock) {
      if (s.st[k] != 0) continue;
      const int4 r = s.r(k);
      const double e = s.e(k);
      const int hi = s.get_hi(k);
      bool waits = false, drop = false;
      for (int j = s.lo[k]; j < hi; j++) {
        if (j == k) continue;
        const uint8_t sj = s.st[j];
        if (sj == 2 || !site_intersect(r, s.r(j)) || !site_before(s.e(j), j, e, k)) continue;
        if (sj == 1) {
          drop = true;
          break;
        }
        waits = true;
      }
      if (drop) s.st[k] = 2;
      else if (!waits) s.st[k] = 1;
      else undecided = 1;
    }
    if (__syncthreads_or(undecided) == 0) break;
  }
  for (int k = tid; k < L; k += kSiteBlock) keep[k] = s.st[k] == 1;
}

// The runs of long_list, one workgroup each (the workgroups take them in turns): up to lds_hits hits with everything in
// LDS (62 KB for kSiteLdsHits: two workgroups per CU), longer ones through SiteHbm with lo / hi / state = scratch of
// one entry per hit of the list.
__global__ __launch_bounds__(kSiteBlock) void k_site_select_long(HitSoA h, int64_t n, const uint8_t *__restrict__ head,
                                                                 const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ nlong,
                                                                 int lds_hits, int32_t *lo, int32_t *hi, uint8_t *state, uint8_t *keep) {
  __shared__ int4 rect_s[kSiteLdsHits];
  __shared__ double key_s[kSiteLdsHits];
  __shared__ int32_t lo_s[kSiteLdsHits];
  __shared__ uint16_t hi_s[kSiteLdsHits];
  __shared__ uint8_t st_s[kSiteLdsHits];
  __shared__ unsigned end_s;
  const int tid = threadIdx.x;
  const uint32_t nl = *nlong;
  for (uint32_t run = blockIdx.x; run < nl; run += gridDim.x) {
    const int64_t s0 = long_list[run];
    // the run ends at the next head flag (or with the list)
    if (tid == 0) end_s = 0xFFFFFFFFu;
    __syncthreads();
    for (int64_t c0 = s0 + 1; c0 < n + kSiteBlock; c0 += kSiteBlock) {
      const int64_t pos = c0 + tid;
      const int ends = pos >= n || head[pos] != 0;
      if (ends) atomicMin(&end_s, (unsigned)min(pos, n));
      if (__syncthreads_or(ends)) break;
    }
    const int L = (int)((int64_t)end_s - s0);
    if (L <= lds_hits) {
      for (int k = tid; k < L; k += kSiteBlock) {
        rect_s[k] = site_rect(h, s0 + k);
        key_s[k] = h.e_tot[s0 + k];
      }
      __syncthreads();
      site_select_run(SiteLds{rect_s, key_s, lo_s, hi_s, st_s}, L, keep + s0);
    } else {
      const HitSoA hr{h.q_sp + s0, h.db_sp + s0, h.q_len + s0, h.db_len + s0, h.db_id + s0, h.db_id_start + s0, h.query + s0,
                      h.e_acc + s0, h.e_hyb + s0, h.e_tot + s0};
      site_select_run(SiteHbm{hr, lo + s0, hi + s0, state + s0}, L, keep + s0);
    }
    __syncthreads(); // (the next run takes the same LDS)
  }
}

} // namespace

hipError_t launch_pair_heads(const int32_t *query, const int32_t *db_id, int64_t n, uint8_t *head, hipStream_t s) {
  return launch_1d(k_pair_heads, n, kBlock, 0, s, query, db_id, n, head);
}
hipError_t launch_pair_fold(const HitSoA &h, int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, void *out,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  return launch_1d(k_pair_fold, npairs, kBlock, 0, s, h, n, start, npairs, ends, static_cast<prb_pair_summary *>(out));
}
hipError_t launch_site_select(const HitSoA &h, int64_t n, const uint8_t *head, int lds_hits, const SiteScratch &w, uint8_t *keep,
                              hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX) return hipErrorInvalidValue;
  lds_hits = std::min(std::max(lds_hits, 1), kSiteLdsHits);
  if (hipError_t e = hipMemsetAsync(w.nlong, 0, sizeof(uint32_t), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_site_select_packed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, h, n, head, std::min(lds_hits, 64), keep,
                     w.long_list, w.nlong);
  // (how many runs the first kernel left is known on the device only: the workgroups read the count)
  hipLaunchKernelGGL(k_site_select_long, dim3((unsigned)std::min<int64_t>(kSiteLongGrid, site_long_runs_max(n))), dim3(kSiteBlock), 0, s, h,
                     n, head, w.long_list, w.nlong, lds_hits, w.lo, w.hi, w.state, keep);
  return hipGetLastError();
}

} // namespace prb
