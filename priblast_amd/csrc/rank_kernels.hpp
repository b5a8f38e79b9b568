// The ranked top-N lists of the run tables on gfx950 - the per-target table (each database sequence's N best queries),
// the group ranking table (each group's) and the feature ranking table (each annotated feature's): the order, the merge
// of a run of candidates into a list, the merge of two tables and the gather of the finish.  ranked_kernels.hip wraps
// the bodies below in one kernel template each and says what the payloads are and where a newcomer's comes from.
//
// A list t (a target, a group, a feature) owns n ranked keys keys[t * n ..), n payload slots slots[t * n ..) and
// fill[t].  A key is (energy key, query id, payload slot); the keys in use are keys[t * n, t * n + fill[t]) in rank
// order, and the slots they name are - as a set - 0 .. fill[t] - 1.  Payloads never move: a newcomer takes a slot that
// was never used, or the slot of an entry that the same merge pushed out, and the finish gathers in rank order.
//
// A Source of newcomers names its candidates by a 32-bit `at` (all ones: none).  It has
//   uint32_t limit()                                 a candidate key's `at` lies below it, else the candidate is skipped
//   int64_t first()                                  the list of the table that the source's list 0 is
//   void put(Payload *to, const TargetKey &c)        the payload of candidate c into a slot
// and, for the kernels that group a merge's candidates by list (the per-target table has two of its own instead),
//   bool locate(int64_t c, uint32_t *list, uint32_t *at)   the list and the name of the c-th candidate; false: it names
//                                                          a list outside the table
//   bool key(uint32_t at, TargetKey *k)              the rank key of the candidate named `at`; false: it names a query
//                                                    or an identifier outside the table
#pragma once
#include <algorithm>

#include "search_kernels.hpp"

namespace prb {
namespace ranked {

constexpr int kWaves = 4;             // lists per workgroup, at most
constexpr size_t kLdsMax = 64 * 1024; // dynamic LDS of a workgroup

__device__ __forceinline__ void wave_sync() { // LDS written by one lane of the wavefront, read by another
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the tables' order: energy key, then the query's identifier (`at` takes no part)
__device__ __forceinline__ bool key_less(const TargetKey &a, const TargetKey &b) { return a.e < b.e || (a.e == b.e && a.id < b.id); }
// entries of the sorted keys k[0, n) below x
__device__ __forceinline__ int count_below(const TargetKey *k, int n, const TargetKey &x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key_less(k[m], x)) lo = m + 1;
    else hi = m;
  }
  return lo;
}
__device__ __forceinline__ TargetKey shfl_xor_key(const TargetKey &k, int j) {
  TargetKey o;
  o.e = __shfl_xor((unsigned long long)k.e, j);
  o.id = __shfl_xor(k.id, j);
  o.at = __shfl_xor(k.at, j);
  return o;
}
// the wavefront's 64 keys (one per lane) in ascending order over the lanes: a bitonic network over shuffles
__device__ __forceinline__ TargetKey wave_sort(TargetKey c, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const TargetKey o = shfl_xor_key(c, j);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      if (keep_min ? key_less(o, c) : key_less(c, o)) c = o;
    }
  }
  return c;
}
// a payload from slot to slot (8-byte aligned in both places)
template <class Payload> __device__ __forceinline__ void copy_payload(Payload *to, const Payload *from) {
  static_assert(sizeof(Payload) % 8 == 0, "a payload moves as 8-byte words");
  constexpr int kWords = (int)(sizeof(Payload) / 8);
  uint2 v[kWords];
#pragma unroll
  for (int k = 0; k < kWords; k++) v[k] = reinterpret_cast<const uint2 *>(from)[k];
#pragma unroll
  for (int k = 0; k < kWords; k++) reinterpret_cast<uint2 *>(to)[k] = v[k];
}

// ---- the merge of a run of candidates into its list ----
// One wavefront per run [start[run], start[run + 1]) of rkey, blockDim.x / 64 runs per workgroup; no workgroup barrier
// anywhere.  Run `run` belongs to list src.first() + list_of[start[run]] (below nlists).  Fast path: the list is full and
// no key of the run beats its last kept key - the wavefront has read the run's 16-byte keys and one key of the table.  Else
// the list's keys go to LDS (S, n entries) and the run is streamed 64 keys a step: those that beat the threshold are
// appended to C by ballot and ordered (a bitonic network over the lanes); either list's entries find their new places by
// rank - own index plus the other list's keys below it -, S moving in rounds of 64 from the top down (an entry only
// moves up, so a round never overwrites one that a later round reads), the result cut to n; the threshold drops to the
// new last key.  A newcomer kept takes payload slot cnt + j while there are unused ones, then the slots of the entries
// pushed out (both are prefixes / suffixes of their lists).  Its payload is written at once; a later step may hand the
// slot on, so the steps' writes are kept in order by a fence.
template <class Payload, class Source>
__device__ __forceinline__ void merge_runs(TargetKey *lds, const Source &src, const TargetKey *__restrict__ rkey, const uint32_t *__restrict__ list_of,
                                           const uint32_t *__restrict__ start, int64_t nruns, int64_t nrec, int32_t nlists, int32_t n,
                                           TargetKey *__restrict__ keys, Payload *__restrict__ slots, int32_t *__restrict__ fill) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t run = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (run >= nruns) return; // (uniform over the wavefront)
  TargetKey *const S = lds + (size_t)wave * (size_t)(n + 64), *const C = S + n;
  const int64_t a = start[run], b = run + 1 < nruns ? (int64_t)start[run + 1] : nrec;
  if (a >= b || b > nrec) return;
  const uint32_t list = list_of[a];
  if (list >= (uint32_t)nlists) return;
  const int64_t t = src.first() + list;
  TargetKey *const tk = keys + t * n;
  Payload *const ts = slots + t * n;
  int cnt = min(max(fill[t], 0), n);
  TargetKey thr{~0ull, ~0u, 0};
  if (cnt == n) thr = tk[n - 1];
  const uint64_t below = (1ull << lane) - 1;
  const uint32_t limit = src.limit();
  bool loaded = false;
  for (int64_t base = a; base < b; base += 64) {
    const int64_t i = base + lane;
    TargetKey k{~0ull, ~0u, 0};
    bool take = false;
    if (i < b) {
      k = rkey[i];
      take = k.at < limit && key_less(k, thr);
    }
    const uint64_t mask = __ballot(take);
    if (!mask) continue; // (uniform)
    if (!loaded) {
      for (int j = lane; j < cnt; j += 64) S[j] = tk[j];
      loaded = true;
    }
    const int cn = __popcll(mask);
    if (take) C[__popcll(mask & below)] = k;
    wave_sync();
    TargetKey c{~0ull, ~0u, 0};
    if (lane < cn) c = C[lane];
    c = wave_sort(c, lane);
    wave_sync();
    if (lane < cn) C[lane] = c;
    wave_sync();
    // the newcomers' places and slots, while S is as it was
    int cpos = n;
    if (lane < cn) cpos = lane + count_below(S, cnt, c);
    const int kept_new = __popcll(__ballot(cpos < n));
    const int new_cnt = min(n, cnt + cn), kept_old = new_cnt - kept_new;
    uint32_t slot = 0;
    if (cpos < n) slot = cnt + lane < n ? (uint32_t)(cnt + lane) : S[kept_old + (lane - (n - cnt))].at;
    wave_sync();
    for (int r0 = cnt > 0 ? ((cnt - 1) / 64) * 64 : -1; r0 >= 0; r0 -= 64) {
      const int j = r0 + lane;
      TargetKey x{0, 0, 0};
      int pos = n;
      if (j < cnt) {
        x = S[j];
        pos = j + count_below(C, cn, x);
      }
      wave_sync();
      if (pos < n) S[pos] = x;
      wave_sync();
    }
    if (cpos < n) {
      S[cpos] = TargetKey{c.e, c.id, slot};
      src.put(ts + slot, c);
    }
    wave_sync();
    cnt = new_cnt;
    if (cnt == n) thr = S[n - 1];
    if (base + 64 < b) __threadfence(); // (a slot may be handed on by the next step)
  }
  if (!loaded) return;
  for (int j = lane; j < cnt; j += 64) tk[j] = S[j];
  if (lane == 0) fill[t] = cnt;
}

// ---- two tables over disjoint sets of query identifiers into one ----
// One wavefront per list.  The list's two ranked key lists - the table's (D) and src's (X) - go to LDS; no two of their
// keys are equal, so an entry's place in the union is its index plus the entries of the other list below it, and the
// first n places are kept.  A kept entry of src takes a payload slot as a newcomer of merge_runs does, and its payload
// is copied.  The new keys go straight to the table (both lists are read from LDS).  Nothing for a list that src has
// nothing of; a copy for one that the table has nothing of.
template <class Payload>
__device__ __forceinline__ void join_lists(TargetKey *lds, TargetKey *__restrict__ keys, Payload *__restrict__ slots, int32_t *__restrict__ fill,
                                           const TargetKey *__restrict__ skeys, const Payload *__restrict__ sslots,
                                           const int32_t *__restrict__ sfill, int64_t nlists, int32_t n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (t >= nlists) return; // (uniform over the wavefront)
  const int cs = min(max(sfill[t], 0), n);
  if (cs == 0) return;
  const int cd = min(max(fill[t], 0), n);
  TargetKey *const D = lds + (size_t)wave * 2 * (size_t)n, *const X = D + n;
  TargetKey *const tk = keys + t * n;
  for (int j = lane; j < cd; j += 64) D[j] = tk[j];
  for (int j = lane; j < cs; j += 64) X[j] = skeys[t * n + j];
  wave_sync();
  const int new_cnt = min(n, cd + cs);
  int kept_old = 0;
  for (int r0 = 0; r0 < cd; r0 += 64) {
    const int j = r0 + lane;
    int pos = n;
    if (j < cd) pos = j + count_below(X, cs, D[j]);
    if (pos < n) tk[pos] = D[j];
    kept_old += __popcll(__ballot(pos < n));
  }
  for (int r0 = 0; r0 < cs; r0 += 64) {
    const int j = r0 + lane;
    int pos = n;
    if (j < cs) pos = j + count_below(D, cd, X[j]);
    if (pos < n) {
      const uint32_t slot = cd + j < n ? (uint32_t)(cd + j) : D[kept_old + (j - (n - cd))].at;
      const uint32_t from = min(X[j].at, (uint32_t)(n - 1));
      tk[pos] = TargetKey{X[j].e, X[j].id, slot};
      copy_payload(slots + t * n + slot, sslots + t * n + from);
    }
  }
  if (lane == 0) fill[t] = new_cnt;
}

// ---- the finish ----
// out[i] = the record of rank r of list t, where off[t] <= i < off[t + 1] (off = the exclusive scan of the fills,
// nlists + 1 values) and r = i - off[t]: the filled slots by list, then rank, without gaps; a lane per record
template <class Payload>
__device__ __forceinline__ void gather_ranked(const TargetKey *__restrict__ keys, const Payload *__restrict__ slots, const int64_t *__restrict__ off,
                                              int64_t nlists, int32_t n, int64_t total, Payload *__restrict__ out, int64_t i) {
  if (i >= total) return;
  int64_t lo = 0, hi = nlists; // the last t with off[t] <= i
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (off[m] <= i) lo = m;
    else hi = m - 1;
  }
  const int64_t t = lo < nlists ? lo : nlists - 1;
  const int32_t r = i - off[t] < n ? (int32_t)(i - off[t]) : n - 1;
  const uint32_t at = min(keys[t * n + r].at, (uint32_t)(n - 1));
  const uint2 *s = reinterpret_cast<const uint2 *>(slots + t * n + at);
  uint2 *d = reinterpret_cast<uint2 *>(out + i);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Payload) / 8); k++) d[k] = s[k];
  out[i].rank = r;
}

// wavefronts per workgroup for `per_wave` bytes of LDS each
inline int waves_for(size_t per_wave) { return (int)std::min<size_t>(kWaves, std::max<size_t>(1, kLdsMax / per_wave)); }
// the dynamic LDS of a wavefront of merge_runs / join_lists
inline size_t merge_lds(int32_t n) { return (size_t)(n + 64) * sizeof(TargetKey); } // at most 17 KB (n = 1024)
inline size_t join_lds(int32_t n) { return 2 * (size_t)n * sizeof(TargetKey); }     // at most 32 KB (n = 1024)

} // namespace ranked
} // namespace prb
