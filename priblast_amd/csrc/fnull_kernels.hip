// The feature null table on gfx950: per kept (query, annotated feature of a target) record of one batch, how the query's
// decoys - shuffles of it - fare against the same feature (prb_fnullset_*, `ris -t -A FILE -F N`).  The reference has no
// counterpart: the columns and the record are defined in include/priblast_hip.h.
//
// A kept record k has the four 8-byte words of the group null table: the energy key of its e_min and the three counters.
// Queries x features is too many for a dense lookup, so the records' keys (query << 32 | feature) stand sorted, with the
// records they belong to beside them and the first key of every query: a (query, feature) is found by binary search in
// its query's keys.  A decoy's minimum over the hits that meet a feature is built in a scratch cell per (decoy of the
// open batch, kept record of its owner): the work items of a list of decoy hits are the feature table's - (pair run,
// feature of its target) -, an item that is not kept for its decoy's owner ends before it reads a hit, and the others
// put the minimum energy key of their run's members into their cell with one atomic minimum.  A minimum over a total
// order does not depend on the order of its terms, so a long run is simply cut over the lanes of a wavefront.  Once the
// batch's last page is in, every cell that holds a key is counted into its record - once - and set back to empty.  Every
// column is an integer sum or an integer minimum, built with integer atomics only; all index arithmetic is in int64_t.
// Every kernel checks its hits, records and cells against the table's ranges before it writes: a violation raises `bad`,
// is counted nowhere and writes nothing (the next host call fails).
#include <algorithm>

#include "../../include/priblast_hip.h"

#include "feature_device.hpp"
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_feature_pair) == 80 && sizeof(prb_fnull_pair) == 112 && sizeof(GNullCount) == 32, "a record moves as 8-byte words");

constexpr unsigned long long kNoKey = ~0ull;                  // an empty cell; above every hit's key
constexpr unsigned long long kInfKey = 0xFFF0000000000000ull; // energy_key(+inf): no decoy minimum yet

constexpr int kLongWaves = kBlock / 64; // wavefronts per workgroup of the long-run form
constexpr int kLongGroups = 256;        // ... and its workgroups: they stride over the listed items

// the place among the sorted keys of (query q, feature), or -1 when the feature is not kept for the query; -2 when the
// query's range of keys lies outside the table (q is in [0, nq): the caller has checked)
__device__ __forceinline__ int64_t kept_place(const FNullTab &t, int32_t q, int32_t feature) {
  int64_t lo = t.qoff[q], hi = t.qoff[q + 1];
  if (lo < 0 || lo > hi || hi > t.nkept) return -2;
  const unsigned long long want = ((unsigned long long)(uint32_t)q << 32) | (uint32_t)feature;
  while (lo < hi) { // the first key >= want
    const int64_t m = (lo + hi) >> 1;
    if (t.key[m] < want) lo = m + 1;
    else hi = m;
  }
  return lo < t.qoff[q + 1] && t.key[lo] == want ? lo : -1;
}

// prb_fnullset_create: rec[0, nkept) = the kept records as prb_featset_finish gathered them, a lane per record
__global__ __launch_bounds__(kBlock) void k_fnull_keep(const prb_feature_pair *__restrict__ rec, FNullTab t, prb_feature_pair *__restrict__ kept,
                                                       unsigned long long *__restrict__ key, uint32_t *__restrict__ idx) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= t.nkept) return;
  uint2 v[10];
#pragma unroll
  for (int w = 0; w < 10; w++) v[w] = reinterpret_cast<const uint2 *>(rec + k)[w];
#pragma unroll
  for (int w = 0; w < 10; w++) reinterpret_cast<uint2 *>(kept + k)[w] = v[w];
  const int32_t q = rec[k].s.query, f = rec[k].feature, page = rec[k].page;
  idx[k] = (uint32_t)k;
  t.cnt[k] = GNullCount{energy_key(rec[k].s.e_min), 0ull, 0ull, kInfKey};
  if (q < 0 || q >= t.nq || f < 0 || f >= t.nfeat || page < 0 || page >= t.npages) {
    atomicOr(t.bad, 1u);
    key[k] = kNoKey;
    return;
  }
  key[k] = ((unsigned long long)(uint32_t)q << 32) | (uint32_t)f;
}

// ... the sorted keys against what the folds rely on
__global__ __launch_bounds__(kBlock) void k_fnull_order(FNullTab t) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= t.nkept) return;
  const unsigned long long kj = t.key[j];
  const int64_t q = (int64_t)(kj >> 32);
  if (q >= t.nq || j < t.qoff[q] || j >= t.qoff[q + 1] || (int64_t)t.rec[j] >= t.nkept || (j > 0 && t.key[j - 1] >= kj)) atomicOr(t.bad, 1u);
}

// What both forms of the fold start an item x with: its run, the feature's ends in the page's text and its cell.  False:
// the item is not kept for its decoy's owner, or something lies outside the table (`bad` raised) - nothing more is read.
struct FNullItem {
  FeatRun r;
  int32_t tlo, thi;
  int64_t cell;
};
__device__ __forceinline__ bool fnull_item(const FeatHits &h, const uint32_t *__restrict__ start, int64_t npairs, const FeatPage &pg,
                                           const FeatWork &w, const FNullTab &t, int64_t x, FNullItem &it) {
  const int64_t k = item_run(w.ioff, npairs, x);
  it.r = feat_run(h, start, npairs, k);
  const int32_t d = it.r.d;
  const int64_t nf = d >= 0 && d < pg.nseq ? (int64_t)pg.off[d + 1] - pg.off[d] : 0;
  if (x - w.ioff[k] >= nf) { // (not an item of this run: k_feat_count saw another list)
    atomicOr(t.bad, 1u);
    return false;
  }
  const int32_t dq = h.query[it.r.a];
  if (dq < 0 || dq >= t.ndq || pg.page < 0 || pg.page >= t.npages) {
    atomicOr(t.bad, 1u);
    return false;
  }
  const int32_t owner = t.owner[dq], dec = t.decoy[dq];
  if (owner < 0 || owner >= t.nq || dec < 0 || dec >= t.ndecoys) {
    atomicOr(t.bad, 1u);
    return false;
  }
  const int32_t f = pg.off[d] + (int32_t)(x - w.ioff[k]);
  const int64_t j = kept_place(t, owner, pg.idx[f]);
  if (j == -1) return false;
  it.cell = j < 0 ? -1 : t.doff[dq] + (j - t.qoff[owner]);
  if (it.cell < 0 || it.cell < t.doff[dq] || it.cell >= t.doff[dq + 1] || it.cell >= t.ncells) {
    atomicOr(t.bad, 1u);
    return false;
  }
  it.tlo = pg.tlo[f];
  it.thi = pg.thi[f];
  return true;
}

// A lane per item.  The item of a run of more than kFeatLongRun hits is listed for the wavefront form instead.
__global__ __launch_bounds__(kBlock) void k_fnull_items(FeatHits h, const uint32_t *__restrict__ start, int64_t npairs, int64_t nitems, FeatPage pg,
                                                        FeatWork w, FNullTab t) {
  const int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (x >= nitems) return;
  FNullItem it;
  if (!fnull_item(h, start, npairs, pg, w, t, x, it)) return;
  if (it.r.b - it.r.a > kFeatLongRun) {
    const uint32_t slot = atomicAdd(w.nlong, 1u);
    if ((int64_t)slot < nitems) w.long_list[slot] = (uint32_t)x;
    return;
  }
  unsigned long long key = kNoKey;
  for (int64_t i = it.r.a; i < it.r.b; i++) {
    const FeatSpan s = feat_span(h, pg, it.r.d, i, t.bad);
    if (!s.ok || s.lo > it.thi || s.hi < it.tlo) continue;
    key = min(key, (unsigned long long)energy_key(h.e_tot[i]));
  }
  if (key != kNoKey) atomicMin(&t.cell[it.cell], key);
}

// A wavefront per listed item: every lane takes each 64th hit of the run, then a cross-lane minimum; lane 0 writes.
__global__ __launch_bounds__(kBlock) void k_fnull_items_long(FeatHits h, const uint32_t *__restrict__ start, int64_t npairs, int64_t nitems,
                                                             FeatPage pg, FeatWork w, FNullTab t) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kLongWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kLongWaves;
  const int64_t nlong = min((int64_t)*w.nlong, nitems);
  for (int64_t j = wave; j < nlong; j += nwaves) {
    const int64_t x = w.long_list[j];
    if (x >= nitems) { // (uniform over the wavefront)
      if (lane == 0) atomicOr(t.bad, 1u);
      continue;
    }
    FNullItem it;
    if (!fnull_item(h, start, npairs, pg, w, t, x, it)) continue; // (uniform: every lane looks the same item up)
    unsigned long long key = kNoKey;
    for (int64_t i = it.r.a + lane; i < it.r.b; i += 64) {
      const FeatSpan s = feat_span(h, pg, it.r.d, i, t.bad);
      if (!s.ok || s.lo > it.thi || s.hi < it.tlo) continue;
      key = min(key, (unsigned long long)energy_key(h.e_tot[i]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, off));
    if (lane == 0 && key != kNoKey) atomicMin(&t.cell[it.cell], key);
  }
}

// prb_fnullset_end: a lane per cell of the open batch.  A cell that holds a key is the minimum of one decoy over one kept
// feature: it counts once, and the lane that counted it empties it, so the scratch is all empty again when the kernel is
// over - whatever the size of the next batch.
__global__ __launch_bounds__(kBlock) void k_fnull_close(FNullTab t) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= t.ncells) return;
  const unsigned long long key = t.cell[c];
  if (key == kNoKey) return;
  const int64_t dq = item_run(t.doff, t.ndq, c); // (the last decoy whose cells begin at or before c)
  const int32_t owner = t.owner[dq];
  int64_t k = -1;
  if (owner >= 0 && owner < t.nq && c >= t.doff[dq] && c < t.doff[dq + 1]) {
    const int64_t j = t.qoff[owner] + (c - t.doff[dq]);
    if (j >= 0 && j < t.qoff[owner + 1] && j < t.nkept) k = t.rec[j];
  }
  if (k < 0 || k >= t.nkept) { // (the fold writes the cells of kept records only)
    atomicOr(t.bad, 1u);
    return;
  }
  t.cell[c] = kNoKey;
  GNullCount &n = t.cnt[k];
  atomicAdd(&n.null_hits, 1ull);
  if (key <= n.ekey) atomicAdd(&n.null_le, 1ull);
  atomicMin(&n.null_min, key);
}

// prb_fnullset_finish: out[k] = the kept record k with its counters
__global__ __launch_bounds__(kBlock) void k_fnull_gather(FNullTab t, const prb_feature_pair *__restrict__ kept, prb_fnull_pair *out) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= t.nkept) return;
  const GNullCount n = t.cnt[k];
  prb_fnull_pair r;
  r.f = kept[k];
  r.decoys = t.ndecoys;
  r.pad = 0;
  r.null_hits = (int64_t)n.null_hits;
  r.null_le = (int64_t)n.null_le;
  // the energy key back to its double (energy_key: negative values are stored inverted, the others with the top bit set)
  r.null_min = __longlong_as_double((long long)((n.null_min >> 63) ? n.null_min & 0x7FFFFFFFFFFFFFFFull : ~n.null_min));
  out[k] = r;
}

} // namespace

hipError_t launch_fnull_keep(const void *rec, const FNullTab &t, void *kept, unsigned long long *key, uint32_t *idx, hipStream_t s) {
  return launch_1d(k_fnull_keep, t.nkept, kBlock, 0, s, static_cast<const prb_feature_pair *>(rec), t, static_cast<prb_feature_pair *>(kept), key, idx);
}
hipError_t launch_fnull_order(const FNullTab &t, hipStream_t s) { return launch_1d(k_fnull_order, t.nkept, kBlock, 0, s, t); }
hipError_t launch_fnull_items(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg, const FeatWork &w,
                              const FNullTab &t, hipStream_t s) {
  return launch_1d(k_fnull_items, nitems, kBlock, 0, s, h, start, npairs, nitems, pg, w, t);
}
hipError_t launch_fnull_items_long(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg,
                                   const FeatWork &w, const FNullTab &t, hipStream_t s) {
  if (nitems <= 0) return hipSuccess;
  const int64_t groups = std::min<int64_t>(kLongGroups, (nitems + kLongWaves - 1) / kLongWaves);
  hipLaunchKernelGGL(k_fnull_items_long, dim3((unsigned)groups), dim3(kBlock), 0, s, h, start, npairs, nitems, pg, w, t);
  return hipGetLastError();
}
hipError_t launch_fnull_close(const FNullTab &t, hipStream_t s) { return launch_1d(k_fnull_close, t.ncells, kBlock, 0, s, t); }
hipError_t launch_fnull_gather(const FNullTab &t, const void *kept, void *out, hipStream_t s) {
  return launch_1d(k_fnull_gather, t.nkept, kBlock, 0, s, t, static_cast<const prb_feature_pair *>(kept), static_cast<prb_fnull_pair *>(out));
}

} // namespace prb
