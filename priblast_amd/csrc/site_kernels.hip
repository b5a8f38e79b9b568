// The (query, database sequence) runs of a final, sorted hit list on gfx950: their heads, the per-pair summaries
// (prb_search_page_summary; also what the top-N pair table and the profile start from), the distinct interaction
// sites of each pair (prb_ris_opts::distinct_sites, `ris -u`) and each pair's best co-linear chain of sites
// (prb_ris_opts::chain_sites, `ris -j`).  The reference has no counterpart: the records and the two selection rules
// are defined in include/priblast_hip.h.
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

// ---- what the two selections share ----
__device__ __forceinline__ int4 site_rect(const HitSoA &h, int64_t i) { // inclusive ends: (q0, q1, db0, db1)
  const int q = h.q_sp[i], d = h.db_sp[i];
  return make_int4(q, q + h.q_len[i] - 1, d, d + h.db_len[i] - 1);
}

// The windows of the packed kernels.  A wavefront owns the runs that start in its slice [.., slice1) of 64 hits and
// lays 64 consecutive hits from `base` (the first hit of one of them) over its lanes: what a lane then knows of its hit
// and of its run.  The runs that a packed kernel does not take - longer than short_max, or longer than a wavefront - are
// appended to long_list here.
struct RunWindow {
  int wlen;      // hits in the window
  bool valid;    // the lane has a hit ...
  int64_t i;     // ... this one (the window's first for a lane without)
  int ls, len;   // the run of this lane: the lanes [ls, ls + len)
  bool packed;   // the run is this slice's, ends inside the window and has at most short_max hits
  uint64_t open; // the first lane of the slice's run that does not end inside the window (only the last one can)
};
__device__ __forceinline__ RunWindow run_window(const uint8_t *__restrict__ head, int64_t n, int64_t base, int64_t slice1, int lane,
                                                int short_max, uint32_t *__restrict__ long_list, uint32_t *nlong) {
  RunWindow w;
  w.wlen = (int)min((int64_t)64, n - base);
  w.valid = lane < w.wlen;
  w.i = w.valid ? base + lane : base;
  const uint64_t heads = __ballot(w.valid && head[w.i] != 0); // (bit 0 is set)
  const bool closed = base + 64 >= n || head[base + 64] != 0; // the window's last run ends with the window
  // the run of this lane, as lanes [ls, le)
  w.ls = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
  const uint64_t above = lane < 63 ? heads >> (lane + 1) : 0;
  const int le = above ? lane + 1 + __builtin_ctzll(above) : w.wlen;
  w.len = le - w.ls;
  const bool whole = le < w.wlen || closed;
  const bool mine = w.valid && base + w.ls < slice1;
  // the run that does not end inside the window: from lane 0 on it is longer than a wavefront, else the next window
  // starts with it
  w.open = __ballot(mine && !whole && lane == w.ls);
  w.packed = mine && whole && w.len <= short_max;
  if (mine && lane == w.ls && (whole ? w.len > short_max : w.ls == 0)) long_list[atomicAdd(nlong, 1u)] = (uint32_t)(base + w.ls);
  return w;
}

// For a workgroup: where the run that starts at hit s0 ends - at the next head flag, or with the list.  end_s is a word
// of its LDS.  (A step looks at blockDim.x more hits: n / blockDim.x + 1 steps at most.)
__device__ __forceinline__ int64_t run_end(const uint8_t *__restrict__ head, int64_t n, int64_t s0, unsigned *end_s) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) *end_s = 0xFFFFFFFFu;
  __syncthreads();
  for (int64_t c0 = s0 + 1; c0 < n + nt; c0 += nt) {
    const int64_t pos = c0 + tid;
    const int ends = pos >= n || head[pos] != 0;
    if (ends) atomicMin(end_s, (unsigned)min(pos, n));
    if (__syncthreads_or(ends)) break;
  }
  return (int64_t)*end_s;
}

// ---- distinct interaction sites (prb_ris_opts::distinct_sites, `ris -u`) ----
// Greedy non-maximum suppression inside every (query, db_id) run of the final list (the rule: include/priblast_hip.h),
// in its fix-point form: a hit is kept once every intersecting hit before it in the order (e_tot, place) is dropped, and
// dropped once one of them is kept.  The first undecided hit of the order has only decided hits before it, so every
// round decides it at least: a run of L hits is done after at most L rounds, and every loop below has that bound.
// Decisions are final and never wrong whenever they are taken, so a round may read states that the same round writes.
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
    const RunWindow w = run_window(head, n, base, slice1, lane, short_max, long_list, nlong);
    const bool valid = w.valid, packed = w.packed;
    const int64_t i = w.i;
    const int ls = w.ls, len = w.len;
    const uint64_t open = w.open;
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
    const int L = (int)(run_end(head, n, s0, &end_s) - s0);
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

// ---- best co-linear chain of sites (prb_ris_opts::chain_sites, `ris -j`) ----
// A dynamic programme over every (query, db_id) run of the final list (the rule: include/priblast_hip.h): hit i PRECEDES
// hit j when its rectangle ends before j's begins in both coordinates; S(j) = e_tot[j] + the lowest negative S of the
// hits that precede j (the lowest place among equals), or + 0.0; the chain ends at the lowest S and is read back through
// the chosen predecessors.  The list is sorted by db_sp inside a run, so a hit's predecessors all lie before it: one
// pass in list order finishes every S.

// The pass over the (at most 64) hits that a wavefront holds one per lane, in list order, k = 0 .. count - 1: lane k's S
// is final by then - every hit that precedes it has a lower lane or was counted into P before -, it is broadcast with
// its rectangle's ends and its run, and every later lane of the same run that k precedes takes k on a strict `<`: the
// lowest place among equals, and nothing that is not below 0.0 (P starts there or below).  Alongside, every lane of
// k's run keeps the run's lowest S so far and its place, again on a strict `<`.
//   in:  r, e of the lane's hit; run = the same number on the lanes of one run, different ones otherwise; place0 = the
//        place of lane 0's hit (what prev and best count from); P, prev = the best predecessor before the pass (0.0, -1:
//        none)
//   out: P, prev; best_s, best = the lowest S of the lane's run among the lanes and its place; returns S of the lane
__device__ __forceinline__ double chain_pass(const int4 &r, double e, int run, int count, int lane, int place0, double &P, int &prev,
                                             double &best_s, int &best) {
  double S = P + e;
  best = -1;
  best_s = 0.0;
  for (int k = 0; k < count; k++) { // (count <= 64)
    const double Sk = __shfl(S, k);
    const int q1k = __shfl(r.y, k), d1k = __shfl(r.w, k), runk = __shfl(run, k);
    const bool same = run == runk;
    if (same && lane > k && q1k < r.x && d1k < r.z && Sk < P) {
      P = Sk;
      prev = place0 + k;
      S = P + e;
    }
    if (same && (best < 0 || Sk < best_s)) {
      best_s = Sk;
      best = place0 + k;
    }
  }
  return S;
}

// Runs of up to 64 hits, several per wavefront, in the windows of k_site_select_packed (run_window).  A window of
// singletons only sets keep.  Otherwise one chain_pass over the window's lanes - S, P and the predecessor's lane stay
// in registers, there is no LDS -, and every lane walks its run's chain back from the run's end through the lanes'
// `prev`, one bpermute a step.  Runs longer than short_max (<= 64) are appended to long_list for k_chain_select_long.
__global__ __launch_bounds__(64) void k_chain_select_packed(HitSoA h, int64_t n, const uint8_t *__restrict__ head, int short_max,
                                                            uint8_t *__restrict__ keep, uint32_t *__restrict__ long_list, uint32_t *nlong) {
  const int lane = threadIdx.x;
  const int64_t slice0 = (int64_t)blockIdx.x * 64, slice1 = min(n, slice0 + 64);
  const uint64_t starts = __ballot(slice0 + lane < n && head[min(slice0 + lane, n - 1)] != 0);
  if (starts == 0) return; // (the slice lies inside a run that began before it)
  int64_t base = slice0 + __builtin_ctzll(starts);
  for (int pass = 0; pass < 2 && base < slice1; pass++) {
    const RunWindow w = run_window(head, n, base, slice1, lane, short_max, long_list, nlong);
    bool kept = true; // a singleton is kept
    if (__ballot(w.packed && w.len > 1) != 0) {
      const int4 r = site_rect(h, w.i);
      const double e = h.e_tot[w.i];
      int maxlen = w.packed ? w.len : 0;
      for (int o = 32; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
      double P = 0.0, best_s;
      int prev = -1, best;
      chain_pass(r, e, w.packed ? w.ls : -1 - lane, w.wlen, lane, 0, P, prev, best_s, best);
      // back from the run's end: a chain has at most as many members as its run has hits
      int cur = best;
      kept = false;
      for (int step = 0; step < maxlen; step++) {
        kept = kept || cur == lane;
        const int next = __shfl(prev, cur < 0 ? lane : cur);
        cur = cur < 0 ? -1 : next;
        if (__ballot(w.packed && cur >= 0) == 0) break;
      }
    }
    if (w.packed) keep[w.i] = kept;
    if (w.open == 0 || (w.open & 1)) break; // nothing open, or the long run: whatever follows starts behind the slice
    base += __builtin_ctzll(w.open);
  }
}

// A run's rectangles, energies, scores and predecessors, indexed from the run's first hit: in the workgroup's LDS ...
struct ChainLds {
  int4 *rect;
  double *key, *score;
  int32_t *pv;
  __device__ __forceinline__ int4 r(int k) const { return rect[k]; }
  __device__ __forceinline__ double e(int k) const { return key[k]; }
  __device__ __forceinline__ double S(int k) const { return score[k]; }
  __device__ __forceinline__ int prev(int k) const { return pv[k]; }
  __device__ __forceinline__ void set(int k, double s, int p) const { score[k] = s, pv[k] = p; }
};
// ... or, for a run beyond the LDS capacity, read from the list itself with scores and predecessors in HBM scratch
struct ChainHbm {
  HitSoA h; // from the run's first hit on
  double *score;
  int32_t *pv;
  __device__ __forceinline__ int4 r(int k) const { return site_rect(h, k); }
  __device__ __forceinline__ double e(int k) const { return h.e_tot[k]; }
  __device__ __forceinline__ double S(int k) const { return score[k]; }
  __device__ __forceinline__ int prev(int k) const { return pv[k]; }
  __device__ __forceinline__ void set(int k, double s, int p) const { score[k] = s, pv[k] = p; }
};

constexpr int kChainBlock = 256, kChainWaves = kChainBlock / 64;

// One run of L hits by one workgroup, in tiles of 64 hits, a hit per lane.  The earlier tiles are final, so the tile's
// hits first take their best predecessor among them: wavefront v scans the hits v, v + 4, .. (every lane reads the
// same one: a broadcast) on a strict `<`, and the four results are combined by (S, place) through red_*.  Then the
// first wavefront finishes the tile with chain_pass - a predecessor inside the tile has a higher place than any
// before it and wins only if strictly lower -, stores S and prev and keeps the run's best end.  At the end thread 0
// walks the chain back.
template <class St> __device__ void chain_select_run(const St &s, int L, uint8_t *__restrict__ keep, double (*red_s)[64], int (*red_i)[64]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double tail_s = 0.0;
  int tail = -1; // the run's best end so far (the first wavefront's)
  for (int t0 = 0; t0 < L; t0 += 64) { // (L / 64 + 1 tiles at most)
    const int j = t0 + lane;
    const bool valid = j < L;
    const int4 r = s.r(valid ? j : t0);
    double P = 0.0;
    int prev = -1;
    for (int i = wave; i < t0; i += kChainWaves) { // (t0 / 4 + 1 hits at most)
      const int4 ri = s.r(i);
      const double Si = s.S(i);
      if (ri.y < r.x && ri.w < r.z && Si < P) {
        P = Si;
        prev = i;
      }
    }
    red_s[wave][lane] = P;
    red_i[wave][lane] = prev;
    __syncthreads();
    if (wave == 0) {
      for (int v = 1; v < kChainWaves; v++) {
        const double Pv = red_s[v][lane];
        const int iv = red_i[v][lane];
        if (Pv < P || (Pv == P && iv < prev)) { // (equal and one of them none: both are none)
          P = Pv;
          prev = iv;
        }
      }
      double best_s;
      int best;
      const double S = chain_pass(r, s.e(valid ? j : t0), valid ? 0 : -1 - lane, min(64, L - t0), lane, t0, P, prev, best_s, best);
      if (valid) s.set(j, S, prev);
      if (tail < 0 || best_s < tail_s) { // (lane 0 has a hit in every tile: its values are the tile's)
        tail_s = best_s;
        tail = best;
      }
    }
    __syncthreads(); // the tile is final; red_* are free again
  }
  for (int k = tid; k < L; k += kChainBlock) keep[k] = 0;
  __syncthreads();
  if (tid == 0) {
    int cur = tail;
    for (int step = 0; step < L && cur >= 0; step++) { // a chain has at most L members
      keep[cur] = 1;
      cur = s.prev(cur);
    }
  }
}

// The runs of long_list, one workgroup each (the workgroups take them in turns): up to lds_hits hits with everything in
// LDS (57 KB for kChainLdsHits: two workgroups per CU), longer ones through ChainHbm with `score` and `prev` = scratch of
// one entry per hit of the list.
__global__ __launch_bounds__(kChainBlock) void k_chain_select_long(HitSoA h, int64_t n, const uint8_t *__restrict__ head,
                                                                   const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ nlong,
                                                                   int lds_hits, double *score, int32_t *prev, uint8_t *keep) {
  __shared__ int4 rect_s[kChainLdsHits];
  __shared__ double key_s[kChainLdsHits];
  __shared__ double score_s[kChainLdsHits];
  __shared__ int32_t prev_s[kChainLdsHits];
  __shared__ double red_s[kChainWaves][64];
  __shared__ int red_i[kChainWaves][64];
  __shared__ unsigned end_s;
  const int tid = threadIdx.x;
  const uint32_t nl = *nlong;
  for (uint32_t run = blockIdx.x; run < nl; run += gridDim.x) { // (nl / gridDim.x + 1 runs at most)
    const int64_t s0 = long_list[run];
    const int L = (int)(run_end(head, n, s0, &end_s) - s0);
    if (L <= lds_hits) {
      for (int k = tid; k < L; k += kChainBlock) {
        rect_s[k] = site_rect(h, s0 + k);
        key_s[k] = h.e_tot[s0 + k];
      }
      __syncthreads();
      chain_select_run(ChainLds{rect_s, key_s, score_s, prev_s}, L, keep + s0, red_s, red_i);
    } else {
      const HitSoA hr{h.q_sp + s0, h.db_sp + s0, h.q_len + s0, h.db_len + s0, h.db_id + s0, h.db_id_start + s0, h.query + s0,
                      h.e_acc + s0, h.e_hyb + s0, h.e_tot + s0};
      chain_select_run(ChainHbm{hr, score + s0, prev + s0}, L, keep + s0, red_s, red_i);
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
hipError_t launch_chain_select(const HitSoA &h, int64_t n, const uint8_t *head, int lds_hits, const ChainScratch &w, uint8_t *keep,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX) return hipErrorInvalidValue;
  lds_hits = std::min(std::max(lds_hits, 1), kChainLdsHits);
  if (hipError_t e = hipMemsetAsync(w.nlong, 0, sizeof(uint32_t), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_chain_select_packed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, h, n, head, std::min(lds_hits, 64), keep,
                     w.long_list, w.nlong);
  // (how many runs the first kernel left is known on the device only: the workgroups read the count)
  hipLaunchKernelGGL(k_chain_select_long, dim3((unsigned)std::min<int64_t>(kSiteLongGrid, site_long_runs_max(n))), dim3(kChainBlock), 0, s, h,
                     n, head, w.long_list, w.nlong, lds_hits, w.score, w.prev, keep);
  return hipGetLastError();
}

} // namespace prb
