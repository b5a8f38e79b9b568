// The group null table on gfx950: per kept (query, group of database sequences) record of one batch, how the query's
// decoys - shuffles of it - fare against the same group (prb_gnullset_*, `ris -t -G FILE -P N`).  The reference has no
// counterpart: the columns and the record are defined in include/priblast_hip.h.
//
// A kept record k has four 8-byte words: the energy key of its e_min and the three counters.  lookup[q * ngroups + g] = the
// record of (query q, group g), or all ones when that group is not kept for q.  A decoy's minimum over the members of a
// group is built in a scratch cell per (decoy of the open batch d, group g), cell d * ngroups + g: the pages of the batch
// fold their records into it with an atomic minimum of the energy key, and once the batch's last page is in, every cell
// that holds a key is counted into its record - once, however many members the decoy reached - and set back to empty.
// Every column is an integer sum or an integer minimum, built with integer atomics only; all index arithmetic is in
// int64_t.  Every kernel checks its records and cells against the table's ranges before it writes: a violation raises
// `bad`, is counted nowhere and writes nothing (the next host call fails).
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_group_pair) == 88 && sizeof(prb_gnull_pair) == 120 && sizeof(GNullCount) == 32,
              "a record moves as 8-byte words");

constexpr unsigned long long kNoKey = ~0ull;                // an empty cell; above every record's key
constexpr unsigned long long kInfKey = 0xFFF0000000000000ull; // energy_key(+inf): no decoy minimum yet
constexpr uint32_t kNotKept = 0xFFFFFFFFu;

// the record of (query q, group g), or -1 when the group is not kept for the query; -2 when either is out of range or
// the lookup names a record outside the table
__device__ __forceinline__ int64_t kept_record(const GNullTab &t, int32_t q, int32_t g) {
  if (q < 0 || q >= t.nq || g < 0 || g >= t.ngroups) return -2;
  const uint32_t k = t.lookup[(int64_t)q * t.ngroups + g];
  if (k == kNotKept) return -1;
  return (int64_t)k < t.nkept ? (int64_t)k : -2;
}

// prb_gnullset_create: rec[0, nkept) = the kept records as prb_groupset_finish gathered them, a lane per record: its
// place into the lookup (already all ones), its energy key and empty counters.  A (query, group) comes once.
__global__ __launch_bounds__(kBlock) void k_gnull_keep(const prb_group_pair *__restrict__ rec, GNullTab t, prb_group_pair *__restrict__ kept) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= t.nkept) return;
  const int32_t q = rec[k].s.query, g = rec[k].group;
  if (q < 0 || q >= t.nq || g < 0 || g >= t.ngroups) {
    atomicOr(t.bad, 1u);
    return;
  }
  uint2 v[11];
#pragma unroll
  for (int w = 0; w < 11; w++) v[w] = reinterpret_cast<const uint2 *>(rec + k)[w];
#pragma unroll
  for (int w = 0; w < 11; w++) reinterpret_cast<uint2 *>(kept + k)[w] = v[w];
  t.lookup[(int64_t)q * t.ngroups + g] = (uint32_t)k;
  t.cnt[k] = GNullCount{energy_key(rec[k].s.e_min), 0ull, 0ull, kInfKey};
}

// prb_search_page_gnull / prb_gnullset_add_pairs: the pair records rec[0, nrec) of the open batch of ndq decoys against
// one page, a lane per record; record i belongs to decoy query rec[i].query of the batch, a decoy of the real query
// owner[query].  The record's energy key into the cell of (decoy, group of db_id) - unless the group is not kept for the
// owner: such a record is counted nowhere.
__global__ __launch_bounds__(kBlock) void k_gnull_fold(const prb_pair_summary *__restrict__ rec, int64_t nrec, GNullTab t, GroupPage pg) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int32_t dq = rec[i].query, db_id = rec[i].db_id;
  if (dq < 0 || dq >= t.ndq || db_id < 0 || db_id >= pg.nseq || pg.page < 0 || pg.page >= t.npages || rec[i].hits < 1) {
    atomicOr(t.bad, 1u);
    return;
  }
  const int32_t d = t.decoy[dq], g = pg.group_of[db_id];
  const int64_t k = kept_record(t, t.owner[dq], g);
  if (k == -2 || d < 0 || d >= t.ndecoys) {
    atomicOr(t.bad, 1u);
    return;
  }
  if (k < 0) return;
  atomicMin(&t.cell[(int64_t)dq * t.ngroups + g], (unsigned long long)energy_key(rec[i].e_min));
}

// prb_gnullset_end: a lane per cell of the open batch, the group fastest - a wavefront reads 512 contiguous bytes, and
// its atomics go to the records of 64 groups, which differ unless the batch has several decoys of one owner in a row.  A
// cell that holds a key is the minimum of one decoy over one kept group: it counts once, and the lane that counted it
// empties it, so the scratch is all empty again when the kernel is over - whatever the size of the next batch.
__global__ __launch_bounds__(kBlock) void k_gnull_close(GNullTab t) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= (int64_t)t.ndq * t.ngroups) return;
  const unsigned long long key = t.cell[c];
  if (key == kNoKey) return;
  const int64_t k = kept_record(t, t.owner[c / t.ngroups], (int32_t)(c % t.ngroups));
  if (k < 0) { // (the fold writes the cells of kept groups only)
    atomicOr(t.bad, 1u);
    return;
  }
  t.cell[c] = kNoKey;
  GNullCount &n = t.cnt[k];
  atomicAdd(&n.null_hits, 1ull);
  if (key <= n.ekey) atomicAdd(&n.null_le, 1ull);
  atomicMin(&n.null_min, key);
}

// prb_gnullset_finish: out[k] = the kept record k with its counters
__global__ __launch_bounds__(kBlock) void k_gnull_gather(GNullTab t, const prb_group_pair *__restrict__ kept, prb_gnull_pair *out) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= t.nkept) return;
  const GNullCount n = t.cnt[k];
  prb_gnull_pair r;
  r.g = kept[k];
  r.decoys = t.ndecoys;
  r.pad = 0;
  r.null_hits = (int64_t)n.null_hits;
  r.null_le = (int64_t)n.null_le;
  // the energy key back to its double (energy_key: negative values are stored inverted, the others with the top bit set)
  r.null_min = __longlong_as_double((long long)((n.null_min >> 63) ? n.null_min & 0x7FFFFFFFFFFFFFFFull : ~n.null_min));
  out[k] = r;
}

} // namespace

hipError_t launch_gnull_keep(const void *rec, const GNullTab &t, void *kept, hipStream_t s) {
  return launch_1d(k_gnull_keep, t.nkept, kBlock, 0, s, static_cast<const prb_group_pair *>(rec), t, static_cast<prb_group_pair *>(kept));
}
hipError_t launch_gnull_fold(const void *rec, int64_t nrec, const GNullTab &t, const GroupPage &pg, hipStream_t s) {
  return launch_1d(k_gnull_fold, nrec, kBlock, 0, s, static_cast<const prb_pair_summary *>(rec), nrec, t, pg);
}
hipError_t launch_gnull_close(const GNullTab &t, hipStream_t s) { return launch_1d(k_gnull_close, (int64_t)t.ndq * t.ngroups, kBlock, 0, s, t); }
hipError_t launch_gnull_gather(const GNullTab &t, const void *kept, void *out, hipStream_t s) {
  return launch_1d(k_gnull_gather, t.nkept, kBlock, 0, s, t, static_cast<const prb_group_pair *>(kept), static_cast<prb_gnull_pair *>(out));
}

} // namespace prb
