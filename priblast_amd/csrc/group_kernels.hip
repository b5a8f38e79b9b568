// The group table on gfx950: per (query, group of database sequences) of one batch, the group's best member pair and
// the integer sums over its members (prb_groupset_*, `ris -t -G FILE`).  The reference has no counterpart: the columns
// and the record are defined in include/priblast_hip.h.
//
// A slot per (query q, group g): slot q * ngroups + g, all arithmetic in int64_t.  The best member is the minimum over
// the 128-bit key (energy key of e_min, page << 32 | db_id), a total order that the records themselves carry, so every
// column is an integer sum or a minimum over a total order, built with integer atomics only.  Every kernel checks its
// records and slots against the table's ranges before it writes: a violation raises `bad` and writes nothing (the next
// host call fails).
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(GroupSlot) == 96 && sizeof(prb_group_pair) == 88, "a record moves as 8 x 8 bytes");

constexpr unsigned long long kNoKey = ~0ull; // both keys of an empty slot; above every record's

// the slot of (query q, sequence db_id of the page), or -1 when the query, the sequence, the page or its group is out of range
__device__ __forceinline__ int64_t group_slot(const GroupTab &t, const GroupPage &pg, int32_t q, int32_t db_id) {
  if (q < 0 || q >= t.nq || db_id < 0 || db_id >= pg.nseq || pg.page < 0 || pg.page >= t.npages) return -1;
  const int32_t g = pg.group_of[db_id];
  if (g < 0 || g >= t.ngroups) return -1;
  const int64_t slot = (int64_t)q * t.ngroups + g;
  return slot < t.nslots ? slot : -1;
}
// the tie key of a record of the page
__device__ __forceinline__ unsigned long long tie_key(const GroupPage &pg, int32_t db_id) {
  return (unsigned long long)(uint32_t)pg.page << 32 | (uint32_t)db_id;
}

// Fold, step 1: a lane per record.  The counters, and the minimum energy key of the slot.  A lane that lowers the key
// resets the slot's tie key: whatever tie the slot held belongs to a higher energy (of an earlier launch, or of this
// one); the record in the slot stays until step 3 replaces it.  Every such lane stores the same value.
__global__ __launch_bounds__(kBlock) void k_group_energy(const prb_pair_summary *__restrict__ rec, int64_t nrec, GroupTab t, GroupPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int64_t slot = group_slot(t, pg, rec[i].query, rec[i].db_id);
  if (slot < 0 || rec[i].hits < 1) {
    atomicOr(t.bad, 1u);
    return;
  }
  GroupSlot &s = t.slot[slot];
  atomicAdd(&s.members, 1u);
  atomicAdd(&s.hits, (unsigned long long)rec[i].hits);
  const unsigned long long ek = energy_key(rec[i].e_min);
  if (ek < atomicMin(&s.ekey, ek)) s.tie = kNoKey;
}

// Fold, step 2: among the records that hold their slot's energy key - and the slot's own record, if it does - the
// minimum tie key
__global__ __launch_bounds__(kBlock) void k_group_tie(const prb_pair_summary *__restrict__ rec, int64_t nrec, GroupTab t, GroupPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int64_t slot = group_slot(t, pg, rec[i].query, rec[i].db_id);
  if (slot < 0 || rec[i].hits < 1) return; // (step 1 has raised `bad`)
  GroupSlot &s = t.slot[slot];
  if (energy_key(rec[i].e_min) == s.ekey) atomicMin(&s.tie, tie_key(pg, rec[i].db_id));
}

// Fold, step 3: the record that holds both keys of its slot - one at most, a (page, db_id) comes once per query -
// writes itself there, with the bits it came with
__global__ __launch_bounds__(kBlock) void k_group_take(const prb_pair_summary *__restrict__ rec, int64_t nrec, GroupTab t, GroupPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int64_t slot = group_slot(t, pg, rec[i].query, rec[i].db_id);
  if (slot < 0 || rec[i].hits < 1) return;
  GroupSlot &s = t.slot[slot];
  if (energy_key(rec[i].e_min) != s.ekey || tie_key(pg, rec[i].db_id) != s.tie) return;
  uint2 v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(rec + i)[k];
  uint2 *d = reinterpret_cast<uint2 *>(s.s);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = v[k];
}

// prb_groupset_merge: a lane per slot; src's counters added, and its record taken where its key is the lower one (an
// empty slot's keys are above every record's, and two tables over disjoint pages never hold the same key)
__global__ __launch_bounds__(kBlock) void k_group_join(GroupTab t, const GroupSlot *__restrict__ src) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= t.nslots) return;
  const GroupSlot &a = src[i];
  if (!a.members) return;
  GroupSlot &d = t.slot[i];
  d.members += a.members;
  d.hits += a.hits;
  if (a.ekey < d.ekey || (a.ekey == d.ekey && a.tie < d.tie)) {
    uint2 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(a.s)[k];
#pragma unroll
    for (int k = 0; k < 8; k++) reinterpret_cast<uint2 *>(d.s)[k] = v[k];
    d.ekey = a.ekey;
    d.tie = a.tie;
  }
}

__global__ __launch_bounds__(kBlock) void k_group_flags(GroupTab t, uint8_t *occ) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < t.nslots) occ[i] = t.slot[i].members != 0;
}

__global__ __launch_bounds__(kBlock) void k_group_clear(GroupTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= t.nslots) return;
  uint2 *d = reinterpret_cast<uint2 *>(&t.slot[i]);
#pragma unroll
  for (int k = 0; k < 12; k++) d[k] = make_uint2(0u, 0u);
  t.slot[i].ekey = kNoKey;
  t.slot[i].tie = kNoKey;
}

// the first place of occ[0, n) whose slot is not below `slot`
__device__ __forceinline__ int64_t first_at_least(const uint32_t *__restrict__ occ, int64_t n, int64_t slot) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if ((int64_t)occ[m] < slot) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// prb_groupset_finish with n > 0: workgroup q takes query q's occupied slots - a run of occ, which ascends - and keeps
// the n of lowest (energy key, tie key) in LDS: kGroupSelect entries of 20 B; the kept ones stay in front, the rest of
// the buffer is refilled from the run and the whole is sorted again (bitonic, ascending; an entry without a slot has
// all-ones keys and the slot 2^32 - 1, which no table has, and sorts behind every other).  Two groups of a query never
// hold the same key: their best members differ.
__global__ __launch_bounds__(kBlock) void k_group_select(GroupTab t, const uint32_t *__restrict__ occ, int64_t nocc, int32_t n,
                                                         uint32_t *__restrict__ top, uint8_t *__restrict__ keep) {
  __shared__ unsigned long long s_e[kGroupSelect], s_t[kGroupSelect];
  __shared__ uint32_t s_slot[kGroupSelect];
  const int32_t q = blockIdx.x;
  const int64_t slot0 = (int64_t)q * t.ngroups;
  const int64_t lo = first_at_least(occ, nocc, slot0), hi = first_at_least(occ, nocc, slot0 + t.ngroups);
  int kept = 0; // entries in front that stay
  int64_t at = lo;
  do {
    const int room = kGroupSelect - kept;
    for (int x = threadIdx.x; x < room; x += kBlock) {
      unsigned long long e = kNoKey, tk = kNoKey;
      uint32_t sl = 0xFFFFFFFFu;
      if (at + x < hi) {
        sl = occ[at + x];
        if ((int64_t)sl < t.nslots) {
          e = t.slot[sl].ekey;
          tk = t.slot[sl].tie;
        } else {
          atomicOr(t.bad, 1u);
          sl = 0xFFFFFFFFu;
        }
      }
      s_e[kept + x] = e;
      s_t[kept + x] = tk;
      s_slot[kept + x] = sl;
    }
    at += room;
    __syncthreads();
    for (int k = 2; k <= kGroupSelect; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int x = threadIdx.x; x < kGroupSelect; x += kBlock) {
          const int y = x ^ j;
          if (y > x) {
            const bool up = (x & k) == 0;
            const unsigned long long ex = s_e[x], ey = s_e[y], tx = s_t[x], ty = s_t[y];
            const uint32_t sx = s_slot[x], sy = s_slot[y];
            const bool x_above = ex > ey || (ex == ey && (tx > ty || (tx == ty && sx > sy)));
            if (x_above == up) {
              s_e[x] = ey, s_e[y] = ex;
              s_t[x] = ty, s_t[y] = tx;
              s_slot[x] = sy, s_slot[y] = sx;
            }
          }
        }
        __syncthreads();
      }
    kept = n;
  } while (at < hi);
  for (int r = threadIdx.x; r < n; r += kBlock) {
    const uint32_t sl = s_slot[r];
    top[(int64_t)q * n + r] = sl;
    keep[(int64_t)q * n + r] = sl != 0xFFFFFFFFu;
  }
}

// prb_groupset_finish: out[j] = the record of the slot idx[j], or of the slot top[idx[j]] with the rank idx[j] % n
__global__ __launch_bounds__(kBlock) void k_group_gather(GroupTab t, const uint32_t *__restrict__ idx, int64_t nrec, const uint32_t *__restrict__ top,
                                                         int32_t n, prb_group_pair *out) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nrec) return;
  int64_t slot = (int64_t)idx[j];
  int32_t rank = 0;
  if (top) {
    if (slot >= (int64_t)t.nq * n) {
      atomicOr(t.bad, 1u);
      return;
    }
    rank = (int32_t)(slot % n);
    slot = (int64_t)top[slot];
  }
  if (slot >= t.nslots) {
    atomicOr(t.bad, 1u);
    return;
  }
  const GroupSlot &s = t.slot[slot];
  prb_group_pair r;
  r.s = *reinterpret_cast<const prb_pair_summary *>(s.s);
  r.page = (int32_t)(s.tie >> 32);
  r.group = (int32_t)(slot % t.ngroups);
  r.members = (int32_t)s.members;
  r.rank = rank;
  r.hits = (int64_t)s.hits;
  out[j] = r;
}

} // namespace

hipError_t launch_group_clear(const GroupTab &t, hipStream_t s) { return launch_1d(k_group_clear, t.nslots, kBlock, 0, s, t); }
hipError_t launch_group_fold(const void *rec, int64_t nrec, const GroupTab &t, const GroupPage &pg, hipStream_t s) {
  const prb_pair_summary *r = static_cast<const prb_pair_summary *>(rec);
  if (hipError_t e = launch_1d(k_group_energy, nrec, kBlock, 0, s, r, nrec, t, pg); e != hipSuccess) return e;
  if (hipError_t e = launch_1d(k_group_tie, nrec, kBlock, 0, s, r, nrec, t, pg); e != hipSuccess) return e;
  return launch_1d(k_group_take, nrec, kBlock, 0, s, r, nrec, t, pg);
}
hipError_t launch_group_join(const GroupTab &t, const GroupSlot *src, hipStream_t s) { return launch_1d(k_group_join, t.nslots, kBlock, 0, s, t, src); }
hipError_t launch_group_flags(const GroupTab &t, uint8_t *occ, hipStream_t s) { return launch_1d(k_group_flags, t.nslots, kBlock, 0, s, t, occ); }
hipError_t launch_group_select(const GroupTab &t, const uint32_t *occ, int64_t nocc, int32_t n, uint32_t *top, uint8_t *keep, hipStream_t s) {
  if (n < 1 || n > kTopMaxN || t.nq < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_group_select, dim3((unsigned)t.nq), dim3(kBlock), 0, s, t, occ, nocc, n, top, keep);
  return hipGetLastError();
}
hipError_t launch_group_gather(const GroupTab &t, const uint32_t *idx, int64_t nrec, const uint32_t *top, int32_t n, void *out, hipStream_t s) {
  return launch_1d(k_group_gather, nrec, kBlock, 0, s, t, idx, nrec, top, n, static_cast<prb_group_pair *>(out));
}

} // namespace prb
