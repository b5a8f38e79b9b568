// The feature table on gfx950: per (query, annotated feature of a target) of one batch, the `-t` summary over the final
// hits whose span meets the feature (prb_featset_*, `ris -t -A FILE`).  The reference has no counterpart: the membership
// rule, the columns and the record are defined in include/priblast_hip.h.
//
// No sort: a (query, target) run of the final list is contiguous, in output order, and owns all of its target's features.
// The work items of a list are (run, feature of its target); every item walks its run in list order, so every column is
// a count or a left-to-right fold that does not depend on how the list was cut.  Every kernel checks queries, sequences
// and spans against the page before it reads through them: a violation raises `bad` and the hit is counted nowhere.
#include <algorithm>

#include "../../include/priblast_hip.h"

#include "feature_device.hpp"
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_feature_pair) == 80, "a record moves as 10 x 8 bytes");

constexpr int kLongWaves = kBlock / 64; // wavefronts per workgroup of the long-run form
constexpr int kLongGroups = 256;        // ... and its workgroups: they stride over the listed items

__global__ __launch_bounds__(kBlock) void k_feat_count(FeatHits h, const uint32_t *__restrict__ start, int64_t npairs, FeatPage pg, int32_t nq,
                                                       FeatWork w) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k > npairs) return;
  int32_t c = 0;
  if (k < npairs) {
    const FeatRun r = feat_run(h, start, npairs, k);
    const int32_t q = r.a < r.b ? h.query[r.a] : -1;
    if (r.d < 0 || r.d >= pg.nseq || q < 0 || q >= nq) atomicOr(w.bad, 1u);
    else c = pg.off[r.d + 1] - pg.off[r.d];
  }
  w.cnt[k] = c;
}

// what an item has folded so far, and its record
struct FeatFold {
  int64_t hits = 0, inside = 0, best = -1;
  double sum = 0.0, mn = 0.0;
  __device__ __forceinline__ void add(double e, int64_t i) { // (strict `<`: the first minimum stays)
    sum += e;
    if (hits == 0 || e < mn) {
      mn = e;
      best = i;
    }
    hits++;
  }
};
__device__ __forceinline__ void feat_write(const FeatHits &h, const FeatPage &pg, const FeatWork &w, int64_t x, int64_t a, int32_t d, int32_t f,
                                           const FeatFold &t) {
  w.flag[x] = t.hits > 0;
  if (t.hits == 0) return;
  prb_feature_pair r;
  r.s.query = h.query[a];
  r.s.db_id = d;
  r.s.hits = t.hits;
  r.s.e_min = t.mn;
  r.s.e_sum = t.sum;
  r.s.e_acc = h.e_acc[t.best];
  r.s.e_hyb = h.e_hyb[t.best];
  r.s.bp_first[0] = h.ends[4 * t.best];
  r.s.bp_first[1] = h.ends[4 * t.best + 1];
  r.s.bp_last[0] = h.ends[4 * t.best + 2];
  r.s.bp_last[1] = h.ends[4 * t.best + 3];
  r.page = pg.page;
  r.feature = pg.idx[f];
  r.inside = t.inside;
  static_cast<prb_feature_pair *>(w.tmp)[x] = r;
}

// A lane per item walks its run in list order (k_pair_fold's walk, over the hits that meet the feature).  The item of a
// run of more than kFeatLongRun hits is listed for the wavefront form instead (the order of that list does not matter:
// an item has its own place in tmp and flag).
__global__ __launch_bounds__(kBlock) void k_feat_items(FeatHits h, const uint32_t *__restrict__ start, int64_t npairs, int64_t nitems, FeatPage pg,
                                                       FeatWork w) {
  const int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (x >= nitems) return;
  const int64_t k = item_run(w.ioff, npairs, x);
  const FeatRun r = feat_run(h, start, npairs, k);
  const int64_t nf = r.d >= 0 && r.d < pg.nseq ? (int64_t)pg.off[r.d + 1] - pg.off[r.d] : 0;
  if (x - w.ioff[k] >= nf) { // (not an item of this run: k_feat_count saw another list)
    atomicOr(w.bad, 1u);
    w.flag[x] = 0;
    return;
  }
  if (r.b - r.a > kFeatLongRun) {
    w.long_list[atomicAdd(w.nlong, 1u)] = (uint32_t)x;
    return;
  }
  const int32_t f = pg.off[r.d] + (int32_t)(x - w.ioff[k]);
  const int32_t tlo = pg.tlo[f], thi = pg.thi[f];
  FeatFold t;
  for (int64_t i = r.a; i < r.b; i++) {
    const FeatSpan s = feat_span(h, pg, r.d, i, w.bad);
    if (!s.ok || s.lo > thi || s.hi < tlo) continue;
    t.add(h.e_tot[i], i);
    t.inside += s.lo >= tlo && s.hi <= thi;
  }
  feat_write(h, pg, w, x, r.a, r.d, f, t);
}

// A wavefront per listed item: 64 hits of the run are loaded and tested at a time, then the members - the set bits of a
// ballot, lowest lane first, which is list order - are folded one by one with the energy of their lane: the additions
// and comparisons of the lane form, in its order.  Every lane carries the same fold; lane 0 writes.
__global__ __launch_bounds__(kBlock) void k_feat_items_long(FeatHits h, const uint32_t *__restrict__ start, int64_t npairs, int64_t nitems, FeatPage pg,
                                                            FeatWork w) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kLongWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kLongWaves;
  const int64_t nlong = min((int64_t)*w.nlong, nitems);
  for (int64_t j = wave; j < nlong; j += nwaves) {
    const int64_t x = w.long_list[j];
    if (x >= nitems) { // (uniform over the wavefront)
      if (lane == 0) atomicOr(w.bad, 1u);
      continue;
    }
    const int64_t k = item_run(w.ioff, npairs, x);
    const FeatRun r = feat_run(h, start, npairs, k);
    const int64_t nf = r.d >= 0 && r.d < pg.nseq ? (int64_t)pg.off[r.d + 1] - pg.off[r.d] : 0;
    if (x - w.ioff[k] >= nf) {
      if (lane == 0) {
        atomicOr(w.bad, 1u);
        w.flag[x] = 0;
      }
      continue;
    }
    const int32_t f = pg.off[r.d] + (int32_t)(x - w.ioff[k]);
    const int32_t tlo = pg.tlo[f], thi = pg.thi[f];
    FeatFold t;
    for (int64_t base = r.a; base < r.b; base += 64) {
      const int64_t i = base + lane;
      bool member = false, in = false;
      double e = 0.0;
      if (i < r.b) {
        const FeatSpan s = feat_span(h, pg, r.d, i, w.bad);
        member = s.ok && s.lo <= thi && s.hi >= tlo;
        in = member && s.lo >= tlo && s.hi <= thi;
        e = h.e_tot[i];
      }
      t.inside += __popcll(__ballot(in));
      for (uint64_t m = __ballot(member); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        t.add(__shfl(e, l), base + l);
      }
    }
    if (lane == 0) feat_write(h, pg, w, x, r.a, r.d, f, t);
  }
}

// A lane per hit looks through its target's features; the wavefront's unassigned hits go into the counter with one
// 64-bit integer atomic.
__global__ __launch_bounds__(kBlock) void k_feat_unassigned(FeatHits h, FeatPage pg, int32_t nq, FeatWork w) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool un = false;
  if (i < h.n) {
    const int32_t d = h.db_id[i], q = h.query[i];
    if (d < 0 || d >= pg.nseq || q < 0 || q >= nq) {
      atomicOr(w.bad, 1u);
    } else {
      const FeatSpan s = feat_span(h, pg, d, i, w.bad);
      if (s.ok) {
        un = true;
        for (int32_t f = pg.off[d]; f < pg.off[d + 1] && un; f++) un = s.lo > pg.thi[f] || s.hi < pg.tlo[f];
      }
    }
  }
  const uint64_t m = __ballot(un);
  if (m && (threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(reinterpret_cast<unsigned long long *>(w.bad + 2), (unsigned long long)__popcll(m));
}

// the surviving items are in the list's order: a query's records are one run of them
__global__ __launch_bounds__(kBlock) void k_feat_append(const prb_feature_pair *__restrict__ tmp, const uint32_t *__restrict__ sel, int64_t nsel,
                                                        prb_feature_pair *rec, int64_t base, int64_t *first, int64_t *end, int32_t page,
                                                        int32_t nq) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nsel) return;
  const prb_feature_pair r = tmp[sel[j]];
  rec[base + j] = r;
  const int32_t q = r.s.query; // (checked by k_feat_count: in [0, nq))
  if (q < 0 || q >= nq) return;
  const int64_t cell = (int64_t)page * nq + q;
  if (j == 0 || tmp[sel[j - 1]].s.query != q) first[cell] = base + j;
  if (j + 1 == nsel || tmp[sel[j + 1]].s.query != q) end[cell] = base + j + 1;
}

__global__ __launch_bounds__(kBlock) void k_feat_join(prb_feature_pair *rec, int64_t base, int64_t *first, int64_t *end,
                                                      const prb_feature_pair *__restrict__ src_rec, int64_t nsrc,
                                                      const int64_t *__restrict__ src_first, const int64_t *__restrict__ src_end, int64_t ncells) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < nsrc) rec[base + i] = src_rec[i];
  if (i < ncells && src_end[i] > src_first[i]) { // (the page sets are disjoint: dst's cell is empty)
    first[i] = src_first[i] + base;
    end[i] = src_end[i] + base;
  }
}

__global__ __launch_bounds__(kBlock) void k_feat_cell_counts(const int64_t *__restrict__ first, const int64_t *__restrict__ end, int32_t npages,
                                                             int32_t nq, int64_t *cnt) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; // = q * npages + p
  const int64_t ncells = (int64_t)npages * nq;
  if (c > ncells) return;
  int64_t v = 0;
  if (c < ncells) {
    const int64_t cell = (c % npages) * nq + c / npages;
    v = max(end[cell] - first[cell], (int64_t)0);
  }
  cnt[c] = v;
}

__global__ __launch_bounds__(kBlock) void k_feat_gather(const prb_feature_pair *__restrict__ rec, int64_t nrec, const int64_t *__restrict__ first,
                                                        const int64_t *__restrict__ off, int32_t npages, int32_t nq, int64_t total,
                                                        prb_feature_pair *out, uint32_t *bad) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o >= total) return;
  const int64_t c = item_run(off, (int64_t)npages * nq, o);
  const int64_t cell = (c % npages) * nq + c / npages;
  const int64_t src = first[cell] + (o - off[c]);
  if (src < 0 || src >= nrec) {
    atomicOr(bad, 1u);
    return;
  }
  out[o] = rec[src];
}

} // namespace

hipError_t launch_feat_count(const FeatHits &h, const uint32_t *start, int64_t npairs, const FeatPage &pg, int32_t nq, const FeatWork &w,
                             hipStream_t s) {
  return launch_1d(k_feat_count, npairs + 1, kBlock, 0, s, h, start, npairs, pg, nq, w);
}
hipError_t launch_feat_items(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg, const FeatWork &w,
                             hipStream_t s) {
  return launch_1d(k_feat_items, nitems, kBlock, 0, s, h, start, npairs, nitems, pg, w);
}
hipError_t launch_feat_items_long(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg,
                                  const FeatWork &w, hipStream_t s) {
  if (nitems <= 0) return hipSuccess;
  const int64_t groups = std::min<int64_t>(kLongGroups, (nitems + kLongWaves - 1) / kLongWaves);
  hipLaunchKernelGGL(k_feat_items_long, dim3((unsigned)groups), dim3(kBlock), 0, s, h, start, npairs, nitems, pg, w);
  return hipGetLastError();
}
hipError_t launch_feat_unassigned(const FeatHits &h, const FeatPage &pg, int32_t nq, const FeatWork &w, hipStream_t s) {
  return launch_1d(k_feat_unassigned, h.n, kBlock, 0, s, h, pg, nq, w);
}
hipError_t launch_feat_append(const void *tmp, const uint32_t *sel, int64_t nsel, void *rec, int64_t base, int64_t *first, int64_t *end,
                              int32_t page, int32_t nq, hipStream_t s) {
  return launch_1d(k_feat_append, nsel, kBlock, 0, s, static_cast<const prb_feature_pair *>(tmp), sel, nsel, static_cast<prb_feature_pair *>(rec),
                   base, first, end, page, nq);
}
hipError_t launch_feat_join(void *rec, int64_t base, int64_t *first, int64_t *end, const void *src_rec, int64_t nsrc, const int64_t *src_first,
                            const int64_t *src_end, int64_t ncells, hipStream_t s) {
  return launch_1d(k_feat_join, std::max(nsrc, ncells), kBlock, 0, s, static_cast<prb_feature_pair *>(rec), base, first, end,
                   static_cast<const prb_feature_pair *>(src_rec), nsrc, src_first, src_end, ncells);
}
hipError_t launch_feat_cell_counts(const int64_t *first, const int64_t *end, int32_t npages, int32_t nq, int64_t *cnt, hipStream_t s) {
  return launch_1d(k_feat_cell_counts, (int64_t)npages * nq + 1, kBlock, 0, s, first, end, npages, nq, cnt);
}
hipError_t launch_feat_gather(const void *rec, int64_t nrec, const int64_t *first, const int64_t *off, int32_t npages, int32_t nq, int64_t total,
                              void *out, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_feat_gather, total, kBlock, 0, s, static_cast<const prb_feature_pair *>(rec), nrec, first, off, npages, nq, total,
                   static_cast<prb_feature_pair *>(out), bad);
}

} // namespace prb
