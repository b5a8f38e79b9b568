// The group ranking table on gfx950: each group's N best queries (prb_grouprank_*, `ris -t -G FILE -R N`) over all the
// queries of a run, ranked on the device.  The reference has no counterpart: the records and the order are defined in
// include/priblast_hip.h.
//
// A group g is a list of rank_kernels.hpp - ranked keys, payload slots that never move, a fill count -, and the merges
// and the gather are that file's, shared with the per-target table.  Here are the payload (prb_group_pair), the two
// sources of newcomers - the occupied slots of a batch's group table (group_kernels.hip), and a caller's records - and
// the grouping of the candidates by group: their group as the sort key, then, behind the stable sort, their rank keys
// and the heads of the groups' runs.  A candidate that names a group, a query or an identifier outside the table raises
// `bad` and is skipped: its key's `at` is all ones, which no source has.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "rank_kernels.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_group_pair) == 88 && sizeof(GroupSlot) == 96 && sizeof(TargetKey) == 16, "a payload moves as 11 x 8 bytes, a key as 16");
constexpr uint32_t kNoCandidate = ~0u;

// the occupied slots of a batch's group table, named by their slot index; ids[q] = the identifier of query q
struct SlotSource {
  GroupTab t;
  const int32_t *ids;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)t.nslots; }
  // candidate c of the list cand[] = a slot index
  __device__ __forceinline__ bool locate(const uint32_t *cand, int64_t c, uint32_t *group, uint32_t *at) const {
    const uint32_t sl = cand[c];
    if ((int64_t)sl >= t.nslots) return false;
    *group = (uint32_t)(sl % (uint32_t)t.ngroups);
    *at = sl;
    return true;
  }
  __device__ __forceinline__ bool key(uint32_t at, TargetKey *k) const {
    if ((int64_t)at >= t.nslots) return false;
    const int64_t q = (int64_t)at / t.ngroups;
    const GroupSlot &s = t.slot[at];
    if (q >= t.nq || !s.members || ids[q] < 0) return false;
    *k = TargetKey{s.ekey, (uint32_t)ids[q], at};
    return true;
  }
  // the record that prb_groupset_finish(gs, 0) gathers of the slot, under the query's identifier
  __device__ __forceinline__ void put(prb_group_pair *to, const TargetKey &c) const {
    const GroupSlot &s = t.slot[c.at];
    uint2 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(s.s)[k];
    v[0].x = c.id; // (s.query)
    uint2 *d = reinterpret_cast<uint2 *>(&to->s);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = v[k];
    to->page = (int32_t)(s.tie >> 32);
    to->group = (int32_t)(c.at % (uint32_t)t.ngroups);
    to->members = (int32_t)s.members;
    to->rank = 0;
    to->hits = (int64_t)s.hits;
  }
};

// a caller's records, whose s.query is the identifier already, named by their index
struct RecordSource {
  const prb_group_pair *rec;
  int64_t nrec;
  int32_t ngroups;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __device__ __forceinline__ bool locate(const uint32_t *, int64_t c, uint32_t *group, uint32_t *at) const {
    const int32_t g = rec[c].group;
    if (g < 0 || g >= ngroups) return false;
    *group = (uint32_t)g;
    *at = (uint32_t)c;
    return true;
  }
  __device__ __forceinline__ bool key(uint32_t at, TargetKey *k) const {
    if ((int64_t)at >= nrec || rec[at].s.query < 0) return false;
    *k = TargetKey{energy_key(rec[at].s.e_min), (uint32_t)rec[at].s.query, at};
    return true;
  }
  __device__ __forceinline__ void put(prb_group_pair *to, const TargetKey &c) const {
    ranked::copy_payload(to, rec + c.at);
    to->rank = 0;
  }
};

// key[c] = the group of candidate c, val[c] = its name at its source: what the stable sort by group takes
template <class Source>
__global__ __launch_bounds__(kBlock) void k_grouprank_groups(Source src, const uint32_t *__restrict__ cand, int64_t ncand, uint32_t *__restrict__ key,
                                                             uint32_t *__restrict__ val, uint32_t *__restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncand) return;
  uint32_t g = 0, at = kNoCandidate;
  if (!src.locate(cand, c, &g, &at)) {
    atomicOr(bad, 1u);
    g = 0;
    at = kNoCandidate;
  }
  key[c] = g;
  val[c] = at;
}
// behind the sort: rkey[i] = the rank key of the i-th candidate in group order, head[i] = 1 where a group's run begins
template <class Source>
__global__ __launch_bounds__(kBlock) void k_grouprank_runs(Source src, int64_t ncand, const uint32_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                           TargetKey *__restrict__ rkey, uint8_t *__restrict__ head, uint32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncand) return;
  TargetKey k{~0ull, ~0u, kNoCandidate};
  if (val[i] != kNoCandidate && !src.key(val[i], &k)) {
    atomicOr(bad, 1u);
    k = TargetKey{~0ull, ~0u, kNoCandidate};
  }
  rkey[i] = k;
  head[i] = i == 0 || key[i] != key[i - 1];
}

// run r of rkey is group group_of[start[r]]
template <class Source>
__global__ __launch_bounds__(64 * ranked::kWaves) void k_grouprank_merge(Source src, const TargetKey *__restrict__ rkey,
                                                                        const uint32_t *__restrict__ group_of, const uint32_t *__restrict__ start,
                                                                        int64_t nruns, int64_t ncand, int32_t ngroups, int32_t n,
                                                                        TargetKey *__restrict__ keys, prb_group_pair *__restrict__ slots,
                                                                        int32_t *__restrict__ fill) {
  extern __shared__ TargetKey grk_lds[];
  ranked::merge_runs(grk_lds, src, rkey, group_of, start, nruns, ncand, (int64_t)0, ngroups, n, keys, slots, fill);
}
__global__ __launch_bounds__(64 * ranked::kWaves) void k_grouprank_join(TargetKey *__restrict__ keys, prb_group_pair *__restrict__ slots,
                                                                       int32_t *__restrict__ fill, const TargetKey *__restrict__ skeys,
                                                                       const prb_group_pair *__restrict__ sslots, const int32_t *__restrict__ sfill,
                                                                       int64_t ngroups, int32_t n) {
  extern __shared__ TargetKey grk_lds[];
  ranked::join_lists(grk_lds, keys, slots, fill, skeys, sslots, sfill, ngroups, n);
}
__global__ __launch_bounds__(kBlock) void k_grouprank_gather(const TargetKey *__restrict__ keys, const prb_group_pair *__restrict__ slots,
                                                             const int64_t *__restrict__ off, int64_t ngroups, int32_t n, int64_t total,
                                                             prb_group_pair *__restrict__ out) {
  ranked::gather_ranked(keys, slots, off, ngroups, n, total, out, (int64_t)blockIdx.x * kBlock + threadIdx.x);
}

template <class Source>
hipError_t launch_merge(const Source &src, const GroupRankRuns &r, int32_t ngroups, int32_t n, TargetKey *keys, void *slots, int32_t *fill,
                        hipStream_t s) {
  if (r.nruns <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN || ngroups < 1 || r.ncand > INT32_MAX || r.nruns > r.ncand) return hipErrorInvalidValue;
  const size_t per_wave = ranked::merge_lds(n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_grouprank_merge<Source>, r.nruns * 64, 64 * waves, per_wave * waves, s, src, r.rkey, r.group_of, r.start, r.nruns, r.ncand,
                   ngroups, n, keys, static_cast<prb_group_pair *>(slots), fill);
}

} // namespace

hipError_t launch_grouprank_slot_groups(const GroupTab &t, const uint32_t *cand, int64_t ncand, uint32_t *key, uint32_t *val, uint32_t *bad,
                                        hipStream_t s) {
  if (t.ngroups < 1) return hipErrorInvalidValue;
  return launch_1d(k_grouprank_groups<SlotSource>, ncand, kBlock, 0, s, SlotSource{t, nullptr}, cand, ncand, key, val, bad);
}
hipError_t launch_grouprank_slot_runs(const GroupTab &t, const int32_t *ids, int64_t ncand, const uint32_t *key, const uint32_t *val,
                                      TargetKey *rkey, uint8_t *head, uint32_t *bad, hipStream_t s) {
  if (t.ngroups < 1) return hipErrorInvalidValue;
  return launch_1d(k_grouprank_runs<SlotSource>, ncand, kBlock, 0, s, SlotSource{t, ids}, ncand, key, val, rkey, head, bad);
}
hipError_t launch_grouprank_slot_merge(const GroupTab &t, const int32_t *ids, const GroupRankRuns &r, int32_t n, TargetKey *keys, void *slots,
                                       int32_t *fill, hipStream_t s) {
  return launch_merge(SlotSource{t, ids}, r, t.ngroups, n, keys, slots, fill, s);
}
hipError_t launch_grouprank_record_groups(const void *rec, int64_t nrec, int32_t ngroups, uint32_t *key, uint32_t *val, uint32_t *bad,
                                          hipStream_t s) {
  return launch_1d(k_grouprank_groups<RecordSource>, nrec, kBlock, 0, s, RecordSource{static_cast<const prb_group_pair *>(rec), nrec, ngroups}, nullptr,
                   nrec, key, val, bad);
}
hipError_t launch_grouprank_record_runs(const void *rec, int64_t nrec, int32_t ngroups, const uint32_t *key, const uint32_t *val, TargetKey *rkey,
                                        uint8_t *head, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_grouprank_runs<RecordSource>, nrec, kBlock, 0, s, RecordSource{static_cast<const prb_group_pair *>(rec), nrec, ngroups}, nrec, key,
                   val, rkey, head, bad);
}
hipError_t launch_grouprank_record_merge(const void *rec, int64_t nrec, const GroupRankRuns &r, int32_t ngroups, int32_t n, TargetKey *keys,
                                         void *slots, int32_t *fill, hipStream_t s) {
  return launch_merge(RecordSource{static_cast<const prb_group_pair *>(rec), nrec, ngroups}, r, ngroups, n, keys, slots, fill, s);
}
hipError_t launch_grouprank_join(TargetKey *keys, void *slots, int32_t *fill, const TargetKey *skeys, const void *sslots, const int32_t *sfill,
                                 int64_t ngroups, int32_t n, hipStream_t s) {
  if (ngroups <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t per_wave = ranked::join_lds(n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_grouprank_join, ngroups * 64, 64 * waves, per_wave * waves, s, keys, static_cast<prb_group_pair *>(slots), fill, skeys,
                   static_cast<const prb_group_pair *>(sslots), sfill, ngroups, n);
}
hipError_t launch_grouprank_gather(const TargetKey *keys, const void *slots, const int64_t *off, int64_t ngroups, int32_t n, int64_t total,
                                   void *out, hipStream_t s) {
  if (ngroups <= 0 || n < 1) return total > 0 ? hipErrorInvalidValue : hipSuccess;
  return launch_1d(k_grouprank_gather, total, kBlock, 0, s, keys, static_cast<const prb_group_pair *>(slots), off, ngroups, n, total,
                   static_cast<prb_group_pair *>(out));
}

} // namespace prb
