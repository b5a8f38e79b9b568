// The null table on gfx950: per observed (query, target) pair of one batch, how its decoys - shuffles of the query -
// fare against the same target (prb_nullset_*, `ris -t -z N`).  The reference has no counterpart: the columns and the
// record are defined in include/priblast_hip.h.
//
// A slot per (query q, target t): slot q * ntargets + t, targets numbered page by page, all arithmetic in int64_t.  A
// slot holds the observed pair's summary record and the counters; every counter is an integer sum or an integer
// minimum, built with integer atomics only.  Every kernel checks its records against the table's ranges before it
// writes: a record out of range raises `bad`, is counted nowhere and writes nothing (the next host call fails).
//
// Sequential p-values (`ris -t -z N -H H`): a byte per slot, `live`, says that the slot still takes decoys.  It is set
// with `observed`; k_null_retire clears it for the slots whose null_le has reached the caller's bound, between two rounds
// of decoys, and k_null_count leaves a slot that is not live alone.  k_null_live_mask turns the live bytes of a decoy
// batch's owners into the rows of the pair mask that the next round is searched under.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(NullSlot) == 96 && sizeof(prb_null_pair) == 96, "a record moves as 8 x 8 bytes");

// the observed pair's record of a slot
__device__ __forceinline__ const prb_pair_summary &null_rec(const NullSlot &s) { return *reinterpret_cast<const prb_pair_summary *>(s.s); }

// the slot of (query q, sequence db_id of the page), or -1 when either is out of range
__device__ __forceinline__ int64_t null_slot(const NullTab &t, const NullPage &pg, int32_t q, int32_t db_id) {
  if (q < 0 || q >= t.nq || db_id < 0 || db_id >= pg.nseq) return -1;
  const int64_t target = pg.target0 + (int64_t)db_id;
  if (target < 0 || target >= t.ntargets) return -1;
  const int64_t slot = (int64_t)q * t.ntargets + target;
  return slot < t.nslots ? slot : -1;
}

// prb_search_page_observed / prb_nullset_observe: the pair records rec[0, nrec) of the real batch against one page, a
// lane per record, into their slots.  A (query, page) is observed once and a record is the only one of its pair, so a
// slot has one writer.
__global__ __launch_bounds__(kBlock) void k_null_observe(const prb_pair_summary *__restrict__ rec, int64_t nrec, NullTab t, NullPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int64_t slot = null_slot(t, pg, rec[i].query, rec[i].db_id);
  if (slot < 0 || rec[i].hits < 1) {
    atomicOr(t.bad, 1u);
    return;
  }
  uint2 v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(rec + i)[k];
  uint2 *d = reinterpret_cast<uint2 *>(t.slot[slot].s);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = v[k];
  t.slot[slot].observed = 1u;
  t.obs[slot] = 1;
  t.live[slot] = 1;
}

// prb_search_page_decoys / prb_nullset_add_pairs: the pair records rec[0, nrec) of a batch of ndq decoys against one
// page, a lane per record; record i belongs to decoy decoy[query] of the real query owner[query].  The page was
// observed by an earlier launch on the same stream, so the slot's e_min is final.
__global__ __launch_bounds__(kBlock) void k_null_count(const prb_pair_summary *__restrict__ rec, int64_t nrec,
                                                       const int32_t *__restrict__ owner, const int32_t *__restrict__ decoy, int32_t ndq,
                                                       NullTab t, NullPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int32_t dq = rec[i].query;
  if (dq < 0 || dq >= ndq) {
    atomicOr(t.bad, 1u);
    return;
  }
  const int32_t d = decoy[dq];
  const int64_t slot = null_slot(t, pg, owner[dq], rec[i].db_id);
  if (slot < 0 || d < 0 || d >= t.ndecoys || rec[i].hits < 1) {
    atomicOr(t.bad, 1u);
    return;
  }
  // (a decoy's pair that the real query does not have, or whose slot has retired, is counted nowhere)
  if (!t.live[slot]) return;
  NullSlot &s = t.slot[slot];
  const unsigned long long ek = energy_key(rec[i].e_min);
  atomicAdd(&s.null_hits, 1ull);
  if (ek <= energy_key(null_rec(s).e_min)) atomicAdd(&s.null_le, 1ull);
  atomicMin(&s.null_min, ek);
}

// prb_nullset_finish: out[j] = the record of the observed slot idx[j]; tbase[npages + 1] = the pages' first targets
__global__ __launch_bounds__(kBlock) void k_null_gather(NullTab t, const uint32_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ tbase,
                                                        int32_t npages, prb_null_pair *out) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int64_t slot = (int64_t)idx[j];
  if (slot >= t.nslots) {
    atomicOr(t.bad, 1u);
    return;
  }
  const NullSlot &s = t.slot[slot];
  const int64_t target = slot % t.ntargets;
  int32_t lo = 0, hi = npages; // the page of the target: tbase[lo] <= target < tbase[lo + 1]
  while (hi - lo > 1) {
    const int32_t m = (lo + hi) >> 1;
    if (tbase[m] <= target) lo = m;
    else hi = m;
  }
  prb_null_pair r;
  r.s = null_rec(s);
  r.page = lo;
  r.decoys = s.seen ? (int32_t)s.seen : t.ndecoys;
  r.null_hits = (int64_t)s.null_hits;
  r.null_le = (int64_t)s.null_le;
  // the energy key back to its double (energy_key: negative values are stored inverted, the others with the top bit set)
  const unsigned long long k = s.null_min;
  r.null_min = __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
  out[j] = r;
}

// every slot back to "not observed": zero, and null_min = the key of +infinity
__global__ __launch_bounds__(kBlock) void k_null_clear(NullTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= t.nslots) return;
  uint2 *d = reinterpret_cast<uint2 *>(&t.slot[i]);
#pragma unroll
  for (int k = 0; k < 12; k++) d[k] = make_uint2(0u, 0u);
  t.slot[i].null_min = 0xFFF0000000000000ull; // energy_key(+inf)
  t.obs[i] = 0;
  t.live[i] = 0;
}

// prb_nullset_retire: a lane per slot.  A live slot whose null_le has reached min_le retires: live = 0, seen = upto (a
// slot retired earlier is not live, so it keeps its seen).  The slots that stay live are counted per query: the lanes of
// a wavefront that hold slots of one query are found by ballot, and their first lane adds the popcount - a wavefront's
// 64 slots lie in as many queries' rows as ntargets lets them, so the loop runs once per query present.  No lane leaves
// before the ballots.
__global__ __launch_bounds__(kBlock) void k_null_retire(NullTab t, unsigned long long min_le, uint32_t upto, unsigned long long *live_q) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < t.nslots;
  bool live = in && t.live[i];
  if (live && t.slot[i].null_le >= min_le) {
    t.live[i] = 0;
    t.slot[i].seen = upto;
    live = false;
  }
  const int32_t q = in ? (int32_t)(i / t.ntargets) : -1;
  unsigned long long todo = __ballot(live);
  while (todo) { // (wavefront-uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const int32_t ql = __shfl(q, lead);
    const unsigned long long same = __ballot(live && q == ql);
    if (lane == lead) atomicAdd(&live_q[ql], (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// prb_pairmask_create_live: wavefront w of the grid takes the 64 targets [64 c, 64 c + 64) of owner r.uowner[u], u = w / C,
// c = w % C, C = the 64-target chunks of a row.  A lane reads one live byte - a target at or beyond ntargets reads as 0 -,
// the ballot is the 64 bits, and the lanes share out the owner's rows: the low word to word 2 c of each, the high word
// to word 2 c + 1 where the row has one (row_words may be odd).  Every word of every row is written by one wavefront.
__global__ __launch_bounds__(kBlock) void k_null_live_mask(NullTab t, LiveMaskRows r, uint32_t *__restrict__ bits, int64_t row_words,
                                                           unsigned long long *count) {
  const int64_t chunks = (t.ntargets + 63) >> 6;
  const int64_t w = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)r.nown * chunks) return; // (a whole wavefront)
  const int32_t u = (int32_t)(w / chunks);
  const int64_t c = w % chunks, target = c * 64 + lane;
  const int32_t own = r.uowner[u];
  const bool own_ok = own >= 0 && own < t.nq;
  if (!own_ok && lane == 0) atomicOr(t.bad, 1u);
  const bool bit = own_ok && target < t.ntargets && t.live[(int64_t)own * t.ntargets + target];
  const unsigned long long m = __ballot(bit);
  const int32_t row0 = r.rowoff[u], nrows = r.rowoff[u + 1] - row0;
  for (int32_t x = lane; x < 2 * nrows; x += 64) {
    const int64_t word = 2 * c + (x & 1);
    if (word < row_words) bits[(int64_t)r.rows[row0 + (x >> 1)] * row_words + word] = (uint32_t)((x & 1) ? m >> 32 : m);
  }
  if (lane == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m) * (unsigned long long)nrows);
}

} // namespace

hipError_t launch_null_clear(const NullTab &t, hipStream_t s) { return launch_1d(k_null_clear, t.nslots, kBlock, 0, s, t); }
hipError_t launch_null_observe(const void *rec, int64_t nrec, const NullTab &t, const NullPage &pg, hipStream_t s) {
  return launch_1d(k_null_observe, nrec, kBlock, 0, s, static_cast<const prb_pair_summary *>(rec), nrec, t, pg);
}
hipError_t launch_null_count(const void *rec, int64_t nrec, const int32_t *owner, const int32_t *decoy, int32_t ndq, const NullTab &t,
                             const NullPage &pg, hipStream_t s) {
  return launch_1d(k_null_count, nrec, kBlock, 0, s, static_cast<const prb_pair_summary *>(rec), nrec, owner, decoy, ndq, t, pg);
}
hipError_t launch_null_retire(const NullTab &t, unsigned long long min_le, uint32_t upto, unsigned long long *live_q, hipStream_t s) {
  return launch_1d(k_null_retire, t.nslots, kBlock, 0, s, t, min_le, upto, live_q);
}
hipError_t launch_null_live_mask(const NullTab &t, const LiveMaskRows &r, uint32_t *bits, int64_t row_words, unsigned long long *count,
                                 hipStream_t s) {
  return launch_1d(k_null_live_mask, (int64_t)r.nown * ((t.ntargets + 63) >> 6) * 64, kBlock, 0, s, t, r, bits, row_words, count);
}
hipError_t launch_null_gather(const NullTab &t, const uint32_t *idx, int64_t n, const int64_t *tbase, int32_t npages, void *out, hipStream_t s) {
  return launch_1d(k_null_gather, n, kBlock, 0, s, t, idx, n, tbase, npages, static_cast<prb_null_pair *>(out));
}

} // namespace prb
