// The ranked run tables on gfx950, over all the queries of a run and ranked on the device: each database sequence's N
// best queries (the per-target table, prb_search_page_targets, `ris -r`), each group's (the group ranking table,
// prb_grouprank_*, `ris -t -G FILE -R N`) and each annotated feature's (the feature ranking table, prb_featrank_*,
// `ris -t -A FILE -B N`).  The reference has no counterpart: the records and the order are defined in
// include/priblast_hip.h.
//
// A target, a group, a feature is a list of rank_kernels.hpp - ranked keys, payload slots that never move, a fill count -,
// and the merges and the gather are that file's.  Here are the three payloads, the five sources of newcomers, and one
// kernel template and one launch for each step: the grouping of a merge's candidates by list - their list as the sort
// key, then, behind the stable sort, their rank keys and the heads of the lists' runs -, the merge of the runs, the join
// of two tables and the gather.  A candidate that names a list, a query or an identifier outside the table raises `bad`
// and is skipped: its key's `at` is all ones, which no source has.  The per-target table groups its candidates with two
// kernels of its own: nothing a search hands it can be refused, and its records take their identifiers in place; and it
// keeps its merge kernel's argument list, which the compiler's registers depend on.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "rank_kernels.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_target_pair) == 72 && sizeof(prb_feature_pair) == 80 && sizeof(prb_group_pair) == 88 &&
                  sizeof(prb_featrank_pair) == 88 && sizeof(GroupSlot) == 96 && sizeof(TargetKey) == 16,
              "a pair record moves as 8 x 8 bytes, a feature record as 10, the payloads as 9 and 11, a key as 16");
constexpr uint32_t kNoCandidate = ~0u;

// ---- the five sources of newcomers (rank_kernels.hpp: Source) ----
// the pair records of a sub-batch, all of `page`, named by their index; the page's first target is tbase
struct PairSource {
  using Payload = prb_target_pair;
  const prb_pair_summary *rec;
  int64_t nrec;
  int32_t page;
  int64_t tbase;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __host__ __device__ __forceinline__ int64_t first() const { return tbase; }
  __device__ __forceinline__ void put(prb_target_pair *to, const TargetKey &c) const {
    uint2 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(rec + c.at)[k];
    uint2 *d = reinterpret_cast<uint2 *>(&to->s);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = v[k];
    to->page = page;
    to->rank = 0;
  }
};

// the occupied slots of a batch's group table, named by their slot index; ids[q] = the identifier of query q
struct GroupSlotSource {
  using Payload = prb_group_pair;
  GroupTab t;
  const uint32_t *cand;
  const int32_t *ids;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)t.nslots; }
  __host__ __device__ __forceinline__ int64_t first() const { return 0; }
  // candidate c of the list cand[] = a slot index
  __device__ __forceinline__ bool locate(int64_t c, uint32_t *group, uint32_t *at) const {
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

// a caller's group records, whose s.query is the identifier already, named by their index
struct GroupRecordSource {
  using Payload = prb_group_pair;
  const prb_group_pair *rec;
  int64_t nrec;
  int32_t ngroups;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __host__ __device__ __forceinline__ int64_t first() const { return 0; }
  __device__ __forceinline__ bool locate(int64_t c, uint32_t *group, uint32_t *at) const {
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

// the records of a batch's unfinished feature table, named by their place in its block; ids[q] = the identifier of query q
struct FeatTableSource {
  using Payload = prb_featrank_pair;
  const prb_feature_pair *rec;
  int64_t nrec;
  const int32_t *ids;
  int32_t nq, nfeat;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __host__ __device__ __forceinline__ int64_t first() const { return 0; }
  // candidate c = the record at place c
  __device__ __forceinline__ bool locate(int64_t c, uint32_t *feature, uint32_t *at) const {
    if (c >= nrec) return false;
    const int32_t f = rec[c].feature;
    if (f < 0 || f >= nfeat) return false;
    *feature = (uint32_t)f;
    *at = (uint32_t)c;
    return true;
  }
  __device__ __forceinline__ bool key(uint32_t at, TargetKey *k) const {
    if ((int64_t)at >= nrec) return false;
    const int32_t q = rec[at].s.query;
    if (q < 0 || q >= nq || ids[q] < 0) return false;
    *k = TargetKey{energy_key(rec[at].s.e_min), (uint32_t)ids[q], at};
    return true;
  }
  // the record that prb_featset_finish returns of that place, under the query's identifier
  __device__ __forceinline__ void put(prb_featrank_pair *to, const TargetKey &c) const {
    uint2 v[10];
#pragma unroll
    for (int k = 0; k < 10; k++) v[k] = reinterpret_cast<const uint2 *>(rec + c.at)[k];
    v[0].x = c.id; // (s.query)
    uint2 *d = reinterpret_cast<uint2 *>(&to->f);
#pragma unroll
    for (int k = 0; k < 10; k++) d[k] = v[k];
    to->rank = 0;
    to->reserved = 0;
  }
};

// a caller's feature records, whose f.s.query is the identifier already, named by their index
struct FeatRecordSource {
  using Payload = prb_featrank_pair;
  const prb_featrank_pair *rec;
  int64_t nrec;
  int32_t nfeat;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __host__ __device__ __forceinline__ int64_t first() const { return 0; }
  __device__ __forceinline__ bool locate(int64_t c, uint32_t *feature, uint32_t *at) const {
    if (c >= nrec) return false;
    const int32_t f = rec[c].f.feature;
    if (f < 0 || f >= nfeat) return false;
    *feature = (uint32_t)f;
    *at = (uint32_t)c;
    return true;
  }
  __device__ __forceinline__ bool key(uint32_t at, TargetKey *k) const {
    if ((int64_t)at >= nrec || rec[at].f.s.query < 0) return false;
    *k = TargetKey{energy_key(rec[at].f.s.e_min), (uint32_t)rec[at].f.s.query, at};
    return true;
  }
  __device__ __forceinline__ void put(prb_featrank_pair *to, const TargetKey &c) const {
    ranked::copy_payload(to, rec + c.at);
    to->rank = 0;
    to->reserved = 0;
  }
};

// ---- a merge's candidates grouped by list ----
// key[c] = the list of candidate c, val[c] = its name at its source: what the stable sort by list takes
template <class Source>
__global__ __launch_bounds__(kBlock) void k_ranked_lists(Source src, int64_t ncand, uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                         uint32_t *__restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncand) return;
  uint32_t l = 0, at = kNoCandidate;
  if (!src.locate(c, &l, &at)) {
    atomicOr(bad, 1u);
    l = 0;
    at = kNoCandidate;
  }
  key[c] = l;
  val[c] = at;
}
// behind the sort: rkey[i] = the rank key of the i-th candidate in list order, head[i] = 1 where a list's run begins
template <class Source>
__global__ __launch_bounds__(kBlock) void k_ranked_runs(Source src, int64_t ncand, const uint32_t *__restrict__ key, const uint32_t *__restrict__ val,
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
// ... of the per-target table: rec[i].query becomes the caller's identifier of the query; key[i] = its db_id, val[i] = i
__global__ __launch_bounds__(kBlock) void k_target_ids(prb_pair_summary *__restrict__ rec, int64_t nrec, const int32_t *__restrict__ ids,
                                                       int32_t nq, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nrec) return;
  const int32_t q = rec[i].query;
  rec[i].query = q >= 0 && q < nq ? ids[q] : -1;
  key[i] = (uint32_t)rec[i].db_id;
  val[i] = (uint32_t)i;
}
// ... and behind the sort: rkey[i] = the rank key of the i-th record in target order (`at` = its index in rec), head[i]
// = 1 where a target's run begins
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

// ---- the merge of the runs into the table, of two tables, and the finish: rank_kernels.hpp ----
// run r of rkey is list src.first() + list_of[start[r]]
template <class Payload, class Source>
__global__ __launch_bounds__(64 * ranked::kWaves) void k_ranked_merge(Source src, const TargetKey *__restrict__ rkey,
                                                                     const uint32_t *__restrict__ list_of, const uint32_t *__restrict__ start,
                                                                     int64_t nruns, int64_t ncand, int32_t nlists, int32_t n,
                                                                     TargetKey *__restrict__ keys, Payload *__restrict__ slots,
                                                                     int32_t *__restrict__ fill) {
  extern __shared__ TargetKey ranked_lds[];
  ranked::merge_runs(ranked_lds, src, rkey, list_of, start, nruns, ncand, nlists, n, keys, slots, fill);
}
// ... of the per-target table, whose pair records keep their `__restrict__`: a source by value has none, which costs this
// kernel two registers
__global__ __launch_bounds__(64 * ranked::kWaves) void k_target_merge(const prb_pair_summary *__restrict__ rec, const TargetKey *__restrict__ rkey,
                                                                     const uint32_t *__restrict__ db_of, const uint32_t *__restrict__ start,
                                                                     int64_t nruns, int64_t nrec, int32_t page, int64_t tbase, int32_t nseq,
                                                                     int32_t n, TargetKey *__restrict__ keys, prb_target_pair *__restrict__ slots,
                                                                     int32_t *__restrict__ fill) {
  extern __shared__ TargetKey ranked_lds[];
  ranked::merge_runs(ranked_lds, PairSource{rec, nrec, page, tbase}, rkey, db_of, start, nruns, nrec, nseq, n, keys, slots, fill);
}
template <class Payload>
__global__ __launch_bounds__(64 * ranked::kWaves) void k_ranked_join(TargetKey *__restrict__ keys, Payload *__restrict__ slots,
                                                                    int32_t *__restrict__ fill, const TargetKey *__restrict__ skeys,
                                                                    const Payload *__restrict__ sslots, const int32_t *__restrict__ sfill,
                                                                    int64_t nlists, int32_t n) {
  extern __shared__ TargetKey ranked_lds[];
  ranked::join_lists(ranked_lds, keys, slots, fill, skeys, sslots, sfill, nlists, n);
}
template <class Payload>
__global__ __launch_bounds__(kBlock) void k_ranked_gather(const TargetKey *__restrict__ keys, const Payload *__restrict__ slots,
                                                          const int64_t *__restrict__ off, int64_t nlists, int32_t n, int64_t total,
                                                          Payload *__restrict__ out) {
  ranked::gather_ranked(keys, slots, off, nlists, n, total, out, (int64_t)blockIdx.x * kBlock + threadIdx.x);
}

// ---- a feed's candidates: its source, their number, the lists they may name, the flag, and the feed's own check ----
template <class Source> struct Candidates {
  Source src;
  int64_t ncand;
  int32_t nlists;
  uint32_t *bad;
  bool ok;
};
Candidates<PairSource> candidates(const PairFeed &f) {
  return {{static_cast<const prb_pair_summary *>(f.rec), f.nrec, f.page, f.tbase}, f.nrec, f.nseq, nullptr, f.ids && f.nq >= 1 && f.tbase >= 0};
}
Candidates<GroupSlotSource> candidates(const GroupSlotFeed &f) { return {{f.t, f.cand, f.ids}, f.ncand, f.t.ngroups, f.bad, f.cand && f.ids && f.bad}; }
Candidates<FeatTableSource> candidates(const FeatTableFeed &f) {
  return {{static_cast<const prb_feature_pair *>(f.rec), f.nrec, f.ids, f.nq, f.nfeat}, f.nrec, f.nfeat, f.bad, f.ids && f.nq >= 1 && f.bad};
}
Candidates<GroupRecordSource> candidates(const RecordFeed<prb_group_pair> &f) {
  return {{static_cast<const prb_group_pair *>(f.rec), f.nrec, f.nlists}, f.nrec, f.nlists, f.bad, f.bad != nullptr};
}
Candidates<FeatRecordSource> candidates(const RecordFeed<prb_featrank_pair> &f) {
  return {{static_cast<const prb_featrank_pair *>(f.rec), f.nrec, f.nlists}, f.nrec, f.nlists, f.bad, f.bad != nullptr};
}
// what every launch over candidates checks of them: a candidate's name is 32 bits, all ones = none
template <class Source> bool candidates_ok(const Candidates<Source> &c) { return c.ok && c.ncand >= 0 && c.ncand <= INT32_MAX && c.nlists >= 1; }

} // namespace

template <class Feed> hipError_t launch_ranked_lists(const Feed &f, uint32_t *key, uint32_t *val, hipStream_t s) {
  const auto c = candidates(f);
  if (!candidates_ok(c)) return hipErrorInvalidValue;
  return launch_1d(k_ranked_lists<decltype(c.src)>, c.ncand, kBlock, 0, s, c.src, c.ncand, key, val, c.bad);
}
template <> hipError_t launch_ranked_lists(const PairFeed &f, uint32_t *key, uint32_t *val, hipStream_t s) {
  if (!candidates_ok(candidates(f))) return hipErrorInvalidValue;
  return launch_1d(k_target_ids, f.nrec, kBlock, 0, s, static_cast<prb_pair_summary *>(f.rec), f.nrec, f.ids, f.nq, key, val);
}
template <class Feed>
hipError_t launch_ranked_runs(const Feed &f, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head, hipStream_t s) {
  const auto c = candidates(f);
  if (!candidates_ok(c)) return hipErrorInvalidValue;
  return launch_1d(k_ranked_runs<decltype(c.src)>, c.ncand, kBlock, 0, s, c.src, c.ncand, key, val, rkey, head, c.bad);
}
template <> hipError_t launch_ranked_runs(const PairFeed &f, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head, hipStream_t s) {
  if (!candidates_ok(candidates(f))) return hipErrorInvalidValue;
  return launch_1d(k_target_runs, f.nrec, kBlock, 0, s, static_cast<const prb_pair_summary *>(f.rec), f.nrec, key, val, rkey, head);
}
// the merge kernel of a source, `block` threads and `lds` bytes to a workgroup
template <class Source, class Payload>
hipError_t enqueue_merge(const Source &src, int32_t nlists, const RankedRuns &r, int32_t n, TargetKey *keys, Payload *slots, int32_t *fill, int block,
                         size_t lds, hipStream_t s) {
  return launch_1d(k_ranked_merge<Payload, Source>, r.nruns * 64, block, lds, s, src, r.rkey, r.list_of, r.start, r.nruns, r.ncand, nlists, n, keys,
                   slots, fill);
}
hipError_t enqueue_merge(const PairSource &src, int32_t nseq, const RankedRuns &r, int32_t n, TargetKey *keys, prb_target_pair *slots, int32_t *fill,
                         int block, size_t lds, hipStream_t s) {
  return launch_1d(k_target_merge, r.nruns * 64, block, lds, s, src.rec, r.rkey, r.list_of, r.start, r.nruns, r.ncand, src.page, src.tbase, nseq, n,
                   keys, slots, fill);
}
template <class Feed> hipError_t launch_ranked_merge(const Feed &f, const RankedRuns &r, const RankedLists &l, hipStream_t s) {
  const auto c = candidates(f);
  using Source = decltype(c.src);
  using Payload = typename Source::Payload;
  if (r.nruns <= 0) return hipSuccess;
  if (!candidates_ok(c) || r.ncand != c.ncand || r.nruns > r.ncand || l.n < 1 || l.n > kTopMaxN || c.src.first() + c.nlists > l.nlists)
    return hipErrorInvalidValue;
  const size_t per_wave = ranked::merge_lds(l.n);
  const int waves = ranked::waves_for(per_wave);
  return enqueue_merge(c.src, c.nlists, r, l.n, l.keys, static_cast<Payload *>(l.slots), l.fill, 64 * waves, per_wave * waves, s);
}
template <class Payload> hipError_t launch_ranked_join(const RankedLists &l, const RankedLists &src, hipStream_t s) {
  if (l.nlists <= 0) return hipSuccess;
  if (l.n < 1 || l.n > kTopMaxN || src.nlists != l.nlists || src.n != l.n) return hipErrorInvalidValue;
  const size_t per_wave = ranked::join_lds(l.n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_ranked_join<Payload>, l.nlists * 64, 64 * waves, per_wave * waves, s, l.keys, static_cast<Payload *>(l.slots), l.fill, src.keys,
                   static_cast<const Payload *>(src.slots), src.fill, l.nlists, l.n);
}
template <class Payload> hipError_t launch_ranked_gather(const RankedLists &l, const int64_t *off, int64_t total, void *out, hipStream_t s) {
  if (l.nlists <= 0 || l.n < 1) return total > 0 ? hipErrorInvalidValue : hipSuccess;
  return launch_1d(k_ranked_gather<Payload>, total, kBlock, 0, s, l.keys, static_cast<const Payload *>(l.slots), off, l.nlists, l.n, total,
                   static_cast<Payload *>(out));
}

// every feed and every payload there is
#define PRB_RANKED_FEED(Feed)                                                                                                             \
  template hipError_t launch_ranked_lists(const Feed &, uint32_t *, uint32_t *, hipStream_t);                                             \
  template hipError_t launch_ranked_runs(const Feed &, const uint32_t *, const uint32_t *, TargetKey *, uint8_t *, hipStream_t);          \
  template hipError_t launch_ranked_merge(const Feed &, const RankedRuns &, const RankedLists &, hipStream_t);
PRB_RANKED_FEED(GroupSlotFeed)
PRB_RANKED_FEED(FeatTableFeed)
PRB_RANKED_FEED(RecordFeed<prb_group_pair>)
PRB_RANKED_FEED(RecordFeed<prb_featrank_pair>)
template hipError_t launch_ranked_merge(const PairFeed &, const RankedRuns &, const RankedLists &, hipStream_t);
#undef PRB_RANKED_FEED
#define PRB_RANKED_PAYLOAD(Payload)                                                                              \
  template hipError_t launch_ranked_join<Payload>(const RankedLists &, const RankedLists &, hipStream_t);        \
  template hipError_t launch_ranked_gather<Payload>(const RankedLists &, const int64_t *, int64_t, void *, hipStream_t);
PRB_RANKED_PAYLOAD(prb_target_pair)
PRB_RANKED_PAYLOAD(prb_group_pair)
PRB_RANKED_PAYLOAD(prb_featrank_pair)
#undef PRB_RANKED_PAYLOAD

} // namespace prb
