// The top-N tables on gfx950: each query's N best pairs (prb_search_page_top, `ris -t -n`) or N best hits
// (prb_search_page_tophits, `ris -k`) over the pages of a database, ranked on the device; the merge of two such tables
// (prb_topset_merge, prb_tophits_merge) and the base-pair pool of the hit table.  The reference has no counterpart:
// the records and the order are defined in include/priblast_hip.h.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// ---- top-N tables (prb_search_page_top, prb_search_page_tophits) ----
// What k_top_merge ranks: the per-pair summaries by e_min into prb_top_pair slots, or the final hits by e_tot into
// prb_top_hit slots.  Either record is 64 bytes with `query` in it, and either slot is the record, `page`, `rank`.
struct TopPairs {
  using Rec = prb_pair_summary;
  using Slot = prb_top_pair;
  static __device__ __forceinline__ double energy(const Rec &r) { return r.e_min; }
  static __device__ __forceinline__ Rec &body(Slot &s) { return s.s; }
  static __device__ __forceinline__ const Rec &body(const Slot &s) { return s.s; }
};
struct TopHits {
  using Rec = prb_hit;
  using Slot = prb_top_hit;
  static __device__ __forceinline__ double energy(const Rec &r) { return r.e_tot; }
  static __device__ __forceinline__ Rec &body(Slot &s) { return s.h; }
  static __device__ __forceinline__ const Rec &body(const Slot &s) { return s.h; }
};
static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_hit) == 64 && sizeof(prb_top_pair) == 72 && sizeof(prb_top_hit) == 72,
              "k_top_merge moves a record as 8 x 8 bytes");
// A record's rank key is (energy key, tie key), compared as two u64 with the smaller one first.  The energy key maps
// the energy to an unsigned integer of the same order (-0.0 becomes +0.0 first, so the two compare equal); the tie key is
// (page << 32) | ordinal, the pair's position among its query's records of that page: the `-t` output order.  Within
// one table no two pairs share a tie key (a page is merged once), so every merge below is one of distinct keys.
constexpr int kTopBlock = 256;
constexpr int kTopLoads = 4;                        // records per lane per step of the stream (loads in flight)
constexpr int kTopTile = kTopBlock * kTopLoads;     // records per step
constexpr int kTopCap = 2 * kTopMaxN;               // candidate buffer: room for at least one step beyond kTopMaxN
constexpr int kTopPer = kTopMaxN / kTopBlock;       // set entries per lane in a merge
constexpr int kTopCandPer = kTopCap / kTopBlock;    // candidate entries per lane in a merge
static_assert(kTopPer * kTopBlock == kTopMaxN && kTopTile <= kTopCap - kTopMaxN, "top-N entries per lane");

__device__ __forceinline__ bool key_less(uint64_t a1, uint64_t a2, uint64_t b1, uint64_t b2) {
  return a1 < b1 || (a1 == b1 && a2 < b2);
}
// entries of the sorted keys (k1, k2)[0, n) below (x1, x2)
__device__ __forceinline__ int count_below(const uint64_t *k1, const uint64_t *k2, int n, uint64_t x1, uint64_t x2) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key_less(k1[m], k2[m], x1, x2)) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// One workgroup per query q = q0 + blockIdx.x of a sub-batch.  rec[0, nrec) are the sub-batch's pair records against
// `page`, ascending by query, so q's records are one run [a, b).  The table keeps q's best pairs in slots
// tab[q * n, q * n + fill[q]), in rank order; on the device a slot's `rank` holds its ordinal.
// LDS (dynamic): the current set's keys and sources (n entries) and a candidate buffer of cap = kTopCap entries.  The
// run streams through in steps of kTopTile records, kTopLoads per lane (one wavefront ballot per load): a record whose
// key beats the set's n-th key (any key while the set is not full) is appended to the buffer, placed by the ballots
// and the waves' counts.  When the next step might not fit, the buffer is bitonic-sorted and merged into the set (each entry's new place = its index + the entries of the
// other list below it), the set is cut to n and the threshold drops.  At the end the set's records are gathered -
// new ones from rec, kept ones from their old slots - and written in rank order.
template <class R>
__global__ __launch_bounds__(kTopBlock) void k_top_merge(const typename R::Rec *__restrict__ rec, int64_t nrec, int32_t q0,
                                                         int32_t page, int32_t n, int32_t cap, typename R::Slot *__restrict__ tab,
                                                         int32_t *__restrict__ fill) {
  using Rec = typename R::Rec;
  using Slot = typename R::Slot;
  extern __shared__ uint64_t top_lds[];
  uint64_t *sk1 = top_lds, *sk2 = sk1 + n, *ck1 = sk2 + n, *ck2 = ck1 + cap;
  uint32_t *ssrc = reinterpret_cast<uint32_t *>(ck2 + cap); // < 2^31: the old slot; else 2^31 | ordinal of a new record
  __shared__ int64_t s_run[2];
  __shared__ int s_wave[kTopBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t q = q0 + (int32_t)blockIdx.x;
  if (tid < 2) { // lower bound of q (tid 0) and of q + 1 (tid 1) in rec
    const int32_t want = q + tid;
    int64_t lo = 0, hi = nrec;
    while (lo < hi) {
      const int64_t m = (lo + hi) >> 1;
      if (rec[m].query < want) lo = m + 1;
      else hi = m;
    }
    s_run[tid] = lo;
  }
  __syncthreads();
  const int64_t a = s_run[0], b = s_run[1];
  if (a >= b) return; // (uniform: no record of q against this page)
  Slot *const slots = tab + (int64_t)q * n;
  int cnt = fill[q];
  for (int i = tid; i < cnt; i += kTopBlock) {
    const Slot &t = slots[i];
    sk1[i] = energy_key(R::energy(R::body(t)));
    sk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
    ssrc[i] = (uint32_t)i;
  }
  __syncthreads();
  uint64_t thr1 = ~0ull, thr2 = ~0ull;
  if (cnt == n) {
    thr1 = sk1[n - 1];
    thr2 = sk2[n - 1];
  }
  int bcnt = 0;
  bool changed = false;
  auto flush = [&]() { // (uniform) sort the buffer, merge it into the set, cut to n
    int P = 1;
    while (P < bcnt) P <<= 1;
    for (int i = bcnt + tid; i < P; i += kTopBlock) ck1[i] = ck2[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P; i += kTopBlock) {
          const int o = i ^ j;
          if (o > i) {
            const uint64_t x1 = ck1[i], x2 = ck2[i], y1 = ck1[o], y2 = ck2[o];
            if (key_less(y1, y2, x1, x2) == ((i & k) == 0)) {
              ck1[i] = y1;
              ck2[i] = y2;
              ck1[o] = x1;
              ck2[o] = x2;
            }
          }
        }
        __syncthreads();
      }
    }
    constexpr int kE = kTopPer + kTopCandPer;
    uint64_t e1[kE], e2[kE];
    uint32_t src[kE];
    int pos[kE];
#pragma unroll
    for (int r = 0; r < kTopPer; r++) {
      const int i = tid + r * kTopBlock;
      pos[r] = n; // (not written)
      if (i < cnt) {
        e1[r] = sk1[i];
        e2[r] = sk2[i];
        src[r] = ssrc[i];
        pos[r] = i + count_below(ck1, ck2, bcnt, e1[r], e2[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kTopCandPer; r++) {
      const int i = tid + r * kTopBlock;
      pos[kTopPer + r] = n;
      if (i < bcnt) {
        e1[kTopPer + r] = ck1[i];
        e2[kTopPer + r] = ck2[i];
        src[kTopPer + r] = 0x80000000u | (uint32_t)ck2[i];
        pos[kTopPer + r] = i + count_below(sk1, sk2, cnt, ck1[i], ck2[i]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kE; r++) {
      if (pos[r] < n) {
        sk1[pos[r]] = e1[r];
        sk2[pos[r]] = e2[r];
        ssrc[pos[r]] = src[r];
      }
    }
    __syncthreads();
    cnt = min(n, cnt + bcnt);
    bcnt = 0;
    changed = true;
    if (cnt == n) {
      thr1 = sk1[n - 1];
      thr2 = sk2[n - 1];
    }
  };
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t base = a; base < b; base += kTopTile) {
    if (bcnt + kTopTile > cap) flush();
    double e[kTopLoads];
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) { // (all loads issued before the first is used)
      const int64_t i = base + u * kTopBlock + tid;
      e[u] = i < b ? R::energy(rec[i]) : 0.0;
    }
    uint64_t k1[kTopLoads], mask[kTopLoads];
    bool take[kTopLoads];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) {
      const int64_t i = base + u * kTopBlock + tid;
      k1[u] = energy_key(e[u]);
      take[u] = i < b && key_less(k1[u], ((uint64_t)(uint32_t)page << 32) | (uint32_t)(i - a), thr1, thr2);
      mask[u] = __ballot(take[u]);
      mine += __popcll(mask[u]);
    }
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    int off = bcnt, total = 0;
#pragma unroll
    for (int w = 0; w < kTopBlock / 64; w++) {
      const int c = s_wave[w];
      off += w < wave ? c : 0;
      total += c;
    }
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) {
      if (take[u]) {
        const int64_t i = base + u * kTopBlock + tid;
        const int at = off + __popcll(mask[u] & below);
        ck1[at] = k1[u];
        ck2[at] = ((uint64_t)(uint32_t)page << 32) | (uint32_t)(i - a);
      }
      off += __popcll(mask[u]);
    }
    bcnt += total;
    __syncthreads(); // (the buffer is complete, s_wave free for the next step)
  }
  if (bcnt > 0) flush();
  if (!changed) return;
  // Write-back in rank order.  A kept pair moves from slot s to a place j >= s, so rounds of 256 places from the top
  // down never read a slot an earlier round wrote; within a round every lane reads before any lane writes.
  for (int r0 = ((cnt - 1) / kTopBlock) * kTopBlock; r0 >= 0; r0 -= kTopBlock) {
    const int j = r0 + tid;
    const Rec *from = nullptr; // (the record, moved as 8 x 8 bytes: 8-byte aligned in both places)
    int32_t pg = 0, rk = 0;
    if (j < cnt) {
      const uint32_t s = ssrc[j];
      if (s & 0x80000000u) {
        rk = (int32_t)(s & 0x7FFFFFFFu);
        from = rec + a + rk;
        pg = page;
      } else if ((int)s != j) {
        from = &R::body(slots[s]);
        pg = slots[s].page;
        rk = slots[s].rank;
      }
    }
    uint2 v[8];
    if (from) {
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(from)[k];
    }
    __syncthreads();
    if (from) {
      uint2 *to = reinterpret_cast<uint2 *>(&R::body(slots[j]));
#pragma unroll
      for (int k = 0; k < 8; k++) to[k] = v[k];
      slots[j].page = pg;
      slots[j].rank = rk;
    }
  }
  if (tid == 0) fill[q] = cnt;
}

// ---- two tables of one kind into one (prb_topset_merge, prb_tophits_merge) ----
// One workgroup per query.  The query's slots in use are two ranked lists - tab's and src's - over disjoint page sets, so
// no two of their (energy key, tie key) pairs are equal, and an entry's place in the union is its index plus the entries
// of the other list below it (binary-search rank: no re-sort).  LDS (dynamic): the two lists' keys (n entries each) and
// the sources of the n places kept - < 2^31: tab's slot, else 2^31 | src's slot.  A record from src keeps its page and
// ordinal; shift = what is added to its bp_offset (the top-N hit table: its list lies behind tab's pool, see
// k_tophits_gather).  The write-back is k_top_merge's: in rank order, from the top down.
template <class R> struct TopRebase;
template <> struct TopRebase<TopPairs> {
  static __device__ __forceinline__ void apply(prb_top_pair &, int64_t) {}
};
template <> struct TopRebase<TopHits> {
  static __device__ __forceinline__ void apply(prb_top_hit &s, int64_t shift) { s.h.bp_offset += shift; }
};
template <class R>
__global__ __launch_bounds__(kTopBlock) void k_table_merge(typename R::Slot *__restrict__ tab, int32_t *__restrict__ fill,
                                                           const typename R::Slot *__restrict__ src, const int32_t *__restrict__ src_fill,
                                                           int32_t n, int64_t shift) {
  using Slot = typename R::Slot;
  extern __shared__ uint64_t top_lds[];
  uint64_t *dk1 = top_lds, *dk2 = dk1 + n, *sk1 = dk2 + n, *sk2 = sk1 + n;
  uint32_t *from = reinterpret_cast<uint32_t *>(sk2 + n);
  const int tid = threadIdx.x;
  const int32_t q = (int32_t)blockIdx.x;
  const int cs = min(max(src_fill[q], 0), n);
  if (cs == 0) return; // (uniform: src has nothing of q)
  const int cd = min(max(fill[q], 0), n);
  Slot *const slots = tab + (int64_t)q * n;
  const Slot *const other = src + (int64_t)q * n;
  for (int i = tid; i < cd; i += kTopBlock) {
    const Slot &t = slots[i];
    dk1[i] = energy_key(R::energy(R::body(t)));
    dk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
  }
  for (int i = tid; i < cs; i += kTopBlock) {
    const Slot &t = other[i];
    sk1[i] = energy_key(R::energy(R::body(t)));
    sk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
  }
  for (int i = tid; i < n; i += kTopBlock) from[i] = (uint32_t)i; // (every place has a source inside the table, whatever the keys)
  __syncthreads();
  for (int i = tid; i < cd; i += kTopBlock) {
    const int pos = i + count_below(sk1, sk2, cs, dk1[i], dk2[i]);
    if (pos < n) from[pos] = (uint32_t)i;
  }
  for (int i = tid; i < cs; i += kTopBlock) {
    const int pos = i + count_below(dk1, dk2, cd, sk1[i], sk2[i]);
    if (pos < n) from[pos] = 0x80000000u | (uint32_t)i;
  }
  __syncthreads();
  const int cnt = min(n, cd + cs);
  // A kept record of tab moves from slot s to a place j >= s, so rounds of 256 places from the top down never read a
  // slot an earlier round wrote; within a round every lane reads before any lane writes.
  for (int r0 = ((cnt - 1) / kTopBlock) * kTopBlock; r0 >= 0; r0 -= kTopBlock) {
    const int j = r0 + tid;
    bool move = false;
    Slot v;
    if (j < cnt) {
      const uint32_t s = from[j];
      if (s & 0x80000000u) {
        v = other[s & 0x7FFFFFFFu];
        TopRebase<R>::apply(v, shift);
        move = true;
      } else if ((int)s != j) {
        v = slots[s];
        move = true;
      }
    }
    __syncthreads();
    if (move) slots[j] = v;
  }
  if (tid == 0) fill[q] = cnt;
}

// ---- base pairs of the top-N hit table ----
// The kept hits' lists lie in a pool in table order without gaps.  After a merge: the counts of the slots in use, their
// exclusive scan (rocPRIM, on the host side), then every list gathered into a second pool at its scanned place.
__global__ __launch_bounds__(kBlock) void k_tophits_counts(const prb_top_hit *__restrict__ tab, const int32_t *__restrict__ fill,
                                                           int32_t n, int64_t nslots, int32_t *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > nslots) return;
  int32_t c = 0;
  if (i < nslots && (int32_t)(i % n) < fill[i / n]) c = max(tab[i].h.bp_count, 0);
  cnt[i] = c;
}
// kTopHitLanes lanes per slot, a pair (8 bytes) per lane and step.  A hit that came with this merge has an offset at
// or beyond `split`, the old pool's size in pairs - its list lies in `fresh` at that offset less `split` -, every other
// one lies in the old pool.  (The lanes of a slot have its old offset in a register before they copy, the first of them
// replaces it behind the copy.)
constexpr int kTopHitLanes = 16;
static_assert(kBlock % kTopHitLanes == 0, "whole slots per workgroup");
__global__ __launch_bounds__(kBlock) void k_tophits_gather(prb_top_hit *__restrict__ tab, const int32_t *__restrict__ fill, int32_t n,
                                                           int64_t nslots, const int64_t *__restrict__ off, int64_t split,
                                                           const int2 *__restrict__ old_pool, const int2 *__restrict__ fresh,
                                                           int2 *__restrict__ pool) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = t / kTopHitLanes;
  const int sub = (int)(t % kTopHitLanes);
  if (i >= nslots) return;
  const int32_t q = (int32_t)(i / n);
  if ((int32_t)(i % n) >= fill[q]) return;
  prb_top_hit &slot = tab[i];
  const int32_t c = max(slot.h.bp_count, 0);
  const int64_t from = slot.h.bp_offset, to = off[i];
  const int2 *src = from >= split ? fresh + (from - split) : old_pool + from;
  for (int32_t j = sub; j < c; j += kTopHitLanes) pool[to + j] = src[j];
  if (sub == 0) slot.h.bp_offset = to;
}

template <class R>
hipError_t launch_top_merge_of(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                               hipStream_t s) {
  if (nrec <= 0 || q1 <= q0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const int cap = kTopCap;
  const size_t lds = (size_t)n * (8 + 8 + 4) + (size_t)cap * 16; // at most 52 KB (n = 1024)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_top_merge<R>), dim3((unsigned)(q1 - q0)), dim3(kTopBlock), lds, s,
                     static_cast<const typename R::Rec *>(rec), nrec, q0, page, n, cap, static_cast<typename R::Slot *>(tab), fill);
  return hipGetLastError();
}
template <class R>
hipError_t launch_table_merge_of(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, int64_t shift,
                                 hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t lds = (size_t)n * (4 * 8 + 4); // at most 36 KB (n = 1024)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_table_merge<R>), dim3((unsigned)nq), dim3(kTopBlock), lds, s, static_cast<typename R::Slot *>(tab),
                     fill, static_cast<const typename R::Slot *>(src), src_fill, n, shift);
  return hipGetLastError();
}

} // namespace

hipError_t launch_top_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                            hipStream_t s) {
  return launch_top_merge_of<TopPairs>(rec, nrec, q0, q1, page, n, tab, fill, s);
}
hipError_t launch_tophits_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                                hipStream_t s) {
  return launch_top_merge_of<TopHits>(rec, nrec, q0, q1, page, n, tab, fill, s);
}
hipError_t launch_top_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, hipStream_t s) {
  return launch_table_merge_of<TopPairs>(tab, fill, src, src_fill, nq, n, 0, s);
}
hipError_t launch_tophits_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, int64_t shift,
                               hipStream_t s) {
  return launch_table_merge_of<TopHits>(tab, fill, src, src_fill, nq, n, shift, s);
}
hipError_t launch_tophits_counts(const void *tab, const int32_t *fill, int32_t n, int64_t nslots, int32_t *cnt, hipStream_t s) {
  if (nslots < 0 || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tophits_counts, dim3((unsigned)((nslots + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     static_cast<const prb_top_hit *>(tab), fill, n, nslots, cnt);
  return hipGetLastError();
}
hipError_t launch_tophits_gather(void *tab, const int32_t *fill, int32_t n, int64_t nslots, const int64_t *off, int64_t split,
                                 const int32_t *old_pool, const int32_t *fresh, int32_t *pool, hipStream_t s) {
  if (nslots <= 0) return hipSuccess;
  if (n < 1 || split < 0) return hipErrorInvalidValue;
  return launch_1d(k_tophits_gather, nslots * kTopHitLanes, kBlock, 0, s, static_cast<prb_top_hit *>(tab), fill, n, nslots, off, split,
                   reinterpret_cast<const int2 *>(old_pool), reinterpret_cast<const int2 *>(fresh), reinterpret_cast<int2 *>(pool));
}

} // namespace prb
