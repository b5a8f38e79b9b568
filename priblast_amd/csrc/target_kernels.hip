// The per-target table on gfx950: each database sequence's N best queries (prb_search_page_targets, `ris -r`) over all
// the queries of a run, ranked on the device; the merge of two such tables (prb_targetset_merge) and the gather of the
// finish.  The reference has no counterpart: the records and the order are defined in include/priblast_hip.h.
//
// A target t (its page's first target + db_id) owns n ranked keys keys[t * n ..), n payload slots slots[t * n ..) and
// fill[t].  A key is (energy key, query id, payload slot); the keys in use are keys[t * n, t * n + fill[t]) in rank
// order, and the slots they name are - as a set - 0 .. fill[t] - 1.  Payloads never move: a newcomer takes a slot that
// was never used, or the slot of an entry that the same merge pushed out, and the finish gathers in rank order.
#include <algorithm>

#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_target_pair) == 72 && sizeof(TargetKey) == 16,
              "a payload moves as 8 (+ 1) x 8 bytes, a key as 16");
constexpr int kTargetWaves = 4;             // target runs per workgroup, at most
constexpr size_t kTargetLdsMax = 64 * 1024; // dynamic LDS of a workgroup

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
// a pair record into a payload slot (8-byte aligned in both places)
__device__ __forceinline__ void put_payload(prb_target_pair *to, const prb_pair_summary *from, int32_t page) {
  uint2 v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(from)[k];
  uint2 *d = reinterpret_cast<uint2 *>(&to->s);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = v[k];
  to->page = page;
  to->rank = 0;
}

// ---- a sub-batch's pair records grouped by target ----
// rec[i].query becomes the caller's identifier of the query; key[i] = its db_id, val[i] = i: what the stable sort takes
__global__ __launch_bounds__(kBlock) void k_target_ids(prb_pair_summary *__restrict__ rec, int64_t nrec, const int32_t *__restrict__ ids,
                                                       int32_t nq, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int32_t q = rec[i].query;
  rec[i].query = q >= 0 && q < nq ? ids[q] : -1;
  key[i] = (uint32_t)rec[i].db_id;
  val[i] = (uint32_t)i;
}
// behind the sort: rkey[i] = the rank key of the i-th record in target order (`at` = its index in rec), head[i] = 1
// where a target's run begins
__global__ __launch_bounds__(kBlock) void k_target_runs(const prb_pair_summary *__restrict__ rec, int64_t nrec, const uint32_t *__restrict__ key,
                                                        const uint32_t *__restrict__ val, TargetKey *__restrict__ rkey,
                                                        uint8_t *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const uint32_t at = val[i];
  TargetKey k;
  k.e = energy_key(rec[at].e_min);
  k.id = (uint32_t)rec[at].query;
  k.at = at;
  rkey[i] = k;
  head[i] = i == 0 || key[i] != key[i - 1];
}

// ---- the merge of a sub-batch into the table ----
// One wavefront per target run [start[run], start[run + 1]) of rkey, blockDim.x / 64 runs per workgroup; no workgroup
// barrier anywhere.  Fast path: the target's table is full and no key of the run beats its last kept key - the
// wavefront has read the run's 16-byte keys and one key of the table.  Else the target's keys go to LDS (S, n entries)
// and the run is streamed 64 keys a step: those that beat the threshold are appended to C by ballot and ordered (a
// bitonic network over the lanes); either list's entries find their new places by rank - own index plus the other
// list's keys below it -, S moving in rounds of 64 from the top down (an entry only moves up, so a round never
// overwrites one that a later round reads), the result cut to n; the threshold drops to the new last key.  A newcomer
// kept takes payload slot cnt + j while there are unused ones, then the slots of the entries pushed out (both are
// prefixes / suffixes of their lists).  Its payload is written at once; a later step may hand the slot on, so the
// steps' writes are kept in order by a fence.
__global__ __launch_bounds__(64 * kTargetWaves) void k_target_merge(const prb_pair_summary *__restrict__ rec, const TargetKey *__restrict__ rkey,
                                                                   const uint32_t *__restrict__ db_of, const uint32_t *__restrict__ start,
                                                                   int64_t nruns, int64_t nrec, int32_t page, int64_t tbase, int32_t nseq,
                                                                   int32_t n, TargetKey *__restrict__ keys, prb_target_pair *__restrict__ slots,
                                                                   int32_t *__restrict__ fill) {
  extern __shared__ TargetKey tgt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t run = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (run >= nruns) return; // (uniform over the wavefront)
  TargetKey *const S = tgt_lds + (size_t)wave * (size_t)(n + 64), *const C = S + n;
  const int64_t a = start[run], b = run + 1 < nruns ? (int64_t)start[run + 1] : nrec;
  if (a >= b || b > nrec) return;
  const uint32_t db_id = db_of[a];
  if (db_id >= (uint32_t)nseq) return;
  const int64_t t = tbase + db_id;
  TargetKey *const tk = keys + t * n;
  prb_target_pair *const ts = slots + t * n;
  int cnt = min(max(fill[t], 0), n);
  TargetKey thr{~0ull, ~0u, 0};
  if (cnt == n) thr = tk[n - 1];
  const uint64_t below = (1ull << lane) - 1;
  bool loaded = false;
  for (int64_t base = a; base < b; base += 64) {
    const int64_t i = base + lane;
    TargetKey k{~0ull, ~0u, 0};
    bool take = false;
    if (i < b) {
      k = rkey[i];
      take = k.at < (uint64_t)nrec && key_less(k, thr);
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
      put_payload(ts + slot, rec + c.at, page);
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

// ---- two tables over disjoint (query id, page) sets into one (prb_targetset_merge) ----
// One wavefront per target.  The target's two ranked key lists - the table's (D) and src's (X) - go to LDS; no two of
// their keys are equal, so an entry's place in the union is its index plus the entries of the other list below it, and
// the first n places are kept.  A kept entry of src takes a payload slot as a newcomer of k_target_merge does, and its
// payload is copied.  The new keys go straight to the table (both lists are read from LDS).  Nothing for a target that
// src has nothing of; a copy for one that the table has nothing of.
__global__ __launch_bounds__(64 * kTargetWaves) void k_target_join(TargetKey *__restrict__ keys, prb_target_pair *__restrict__ slots,
                                                                  int32_t *__restrict__ fill, const TargetKey *__restrict__ skeys,
                                                                  const prb_target_pair *__restrict__ sslots, const int32_t *__restrict__ sfill,
                                                                  int64_t ntargets, int32_t n) {
  extern __shared__ TargetKey tgt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (t >= ntargets) return; // (uniform over the wavefront)
  const int cs = min(max(sfill[t], 0), n);
  if (cs == 0) return;
  const int cd = min(max(fill[t], 0), n);
  TargetKey *const D = tgt_lds + (size_t)wave * 2 * (size_t)n, *const X = D + n;
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
      const uint2 *s = reinterpret_cast<const uint2 *>(sslots + t * n + from);
      uint2 *d = reinterpret_cast<uint2 *>(slots + t * n + slot);
      uint2 v[9];
#pragma unroll
      for (int k = 0; k < 9; k++) v[k] = s[k];
#pragma unroll
      for (int k = 0; k < 9; k++) d[k] = v[k];
    }
  }
  if (lane == 0) fill[t] = new_cnt;
}

// ---- the finish ----
// out[i] = the record of rank r of target t, where off[t] <= i < off[t + 1] (off = the exclusive scan of the fills,
// ntargets + 1 values) and r = i - off[t]: the filled slots by target, then rank, without gaps
__global__ __launch_bounds__(kBlock) void k_target_gather(const TargetKey *__restrict__ keys, const prb_target_pair *__restrict__ slots,
                                                          const int64_t *__restrict__ off, int64_t ntargets, int32_t n, int64_t total,
                                                          prb_target_pair *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  int64_t lo = 0, hi = ntargets; // the last t with off[t] <= i
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (off[m] <= i) lo = m;
    else hi = m - 1;
  }
  const int64_t t = lo < ntargets ? lo : ntargets - 1;
  const int32_t r = i - off[t] < n ? (int32_t)(i - off[t]) : n - 1;
  const uint32_t at = min(keys[t * n + r].at, (uint32_t)(n - 1));
  const uint2 *s = reinterpret_cast<const uint2 *>(slots + t * n + at);
  uint2 *d = reinterpret_cast<uint2 *>(out + i);
#pragma unroll
  for (int k = 0; k < 9; k++) d[k] = s[k];
  out[i].rank = r;
}

// wavefronts per workgroup for `per_wave` bytes of LDS each
int target_waves(size_t per_wave) { return (int)std::min<size_t>(kTargetWaves, std::max<size_t>(1, kTargetLdsMax / per_wave)); }

} // namespace

hipError_t launch_target_ids(void *rec, int64_t nrec, const int32_t *ids, int32_t nq, uint32_t *key, uint32_t *val, hipStream_t s) {
  return launch_1d(k_target_ids, nrec, kBlock, 0, s, static_cast<prb_pair_summary *>(rec), nrec, ids, nq, key, val);
}
hipError_t launch_target_runs(const void *rec, int64_t nrec, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head,
                              hipStream_t s) {
  return launch_1d(k_target_runs, nrec, kBlock, 0, s, static_cast<const prb_pair_summary *>(rec), nrec, key, val, rkey, head);
}
hipError_t launch_target_merge(const void *rec, const TargetKey *rkey, const uint32_t *db_of, const uint32_t *start, int64_t nruns,
                               int64_t nrec, int32_t page, int64_t tbase, int32_t nseq, int32_t n, TargetKey *keys, void *slots, int32_t *fill,
                               hipStream_t s) {
  if (nruns <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN || nrec > INT32_MAX) return hipErrorInvalidValue;
  const size_t per_wave = (size_t)(n + 64) * sizeof(TargetKey); // at most 17 KB (n = 1024)
  const int waves = target_waves(per_wave);
  return launch_1d(k_target_merge, nruns * 64, 64 * waves, per_wave * waves, s, static_cast<const prb_pair_summary *>(rec), rkey, db_of, start,
                   nruns, nrec, page, tbase, nseq, n, keys, static_cast<prb_target_pair *>(slots), fill);
}
hipError_t launch_target_join(TargetKey *keys, void *slots, int32_t *fill, const TargetKey *skeys, const void *sslots, const int32_t *sfill,
                              int64_t ntargets, int32_t n, hipStream_t s) {
  if (ntargets <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t per_wave = 2 * (size_t)n * sizeof(TargetKey); // at most 32 KB (n = 1024)
  const int waves = target_waves(per_wave);
  return launch_1d(k_target_join, ntargets * 64, 64 * waves, per_wave * waves, s, keys, static_cast<prb_target_pair *>(slots), fill, skeys,
                   static_cast<const prb_target_pair *>(sslots), sfill, ntargets, n);
}
hipError_t launch_target_gather(const TargetKey *keys, const void *slots, const int64_t *off, int64_t ntargets, int32_t n, int64_t total,
                                void *out, hipStream_t s) {
  if (ntargets <= 0 || n < 1) return total > 0 ? hipErrorInvalidValue : hipSuccess;
  return launch_1d(k_target_gather, total, kBlock, 0, s, keys, static_cast<const prb_target_pair *>(slots), off, ntargets, n, total,
                   static_cast<prb_target_pair *>(out));
}

} // namespace prb
