// The feature ranking table on gfx950: each annotated feature's N best queries (prb_featrank_*, `ris -t -A FILE -B N`)
// over all the queries of a run, ranked on the device.  The reference has no counterpart: the records and the order are
// defined in include/priblast_hip.h.
//
// A feature f is a list of rank_kernels.hpp - ranked keys, payload slots that never move, a fill count -, and the merges
// and the gather are that file's, shared with the per-target table and the group ranking table.  Here are the payload
// (prb_featrank_pair), the two sources of newcomers - the records of a batch's unfinished feature table
// (feature_kernels.hip), and a caller's records - and the grouping of the candidates by feature: their feature as the
// sort key, then, behind the stable sort, their rank keys and the heads of the features' runs.  A candidate that names a
// feature, a query or an identifier outside the table raises `bad` and is skipped: its key's `at` is all ones, which no
// source has.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "rank_kernels.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_feature_pair) == 80 && sizeof(prb_featrank_pair) == 88 && sizeof(TargetKey) == 16,
              "a record moves as 10 x 8 bytes, a payload as 11, a key as 16");
constexpr uint32_t kNoCandidate = ~0u;

// the records of a batch's unfinished feature table, named by their place in its block; ids[q] = the identifier of query q
struct TableSource {
  const prb_feature_pair *rec;
  int64_t nrec;
  const int32_t *ids;
  int32_t nq, nfeat;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
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

// a caller's records, whose f.s.query is the identifier already, named by their index
struct RecordSource {
  const prb_featrank_pair *rec;
  int64_t nrec;
  int32_t nfeat;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
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

// key[c] = the feature of candidate c, val[c] = its name at its source: what the stable sort by feature takes
template <class Source>
__global__ __launch_bounds__(kBlock) void k_featrank_features(Source src, int64_t ncand, uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                              uint32_t *__restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncand) return;
  uint32_t f = 0, at = kNoCandidate;
  if (!src.locate(c, &f, &at)) {
    atomicOr(bad, 1u);
    f = 0;
    at = kNoCandidate;
  }
  key[c] = f;
  val[c] = at;
}
// behind the sort: rkey[i] = the rank key of the i-th candidate in feature order, head[i] = 1 where a feature's run begins
template <class Source>
__global__ __launch_bounds__(kBlock) void k_featrank_runs(Source src, int64_t ncand, const uint32_t *__restrict__ key, const uint32_t *__restrict__ val,
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

// run r of rkey is feature feature_of[start[r]]
template <class Source>
__global__ __launch_bounds__(64 * ranked::kWaves) void k_featrank_merge(Source src, const TargetKey *__restrict__ rkey,
                                                                       const uint32_t *__restrict__ feature_of, const uint32_t *__restrict__ start,
                                                                       int64_t nruns, int64_t ncand, int32_t nfeat, int32_t n,
                                                                       TargetKey *__restrict__ keys, prb_featrank_pair *__restrict__ slots,
                                                                       int32_t *__restrict__ fill) {
  extern __shared__ TargetKey frk_lds[];
  ranked::merge_runs(frk_lds, src, rkey, feature_of, start, nruns, ncand, (int64_t)0, nfeat, n, keys, slots, fill);
}
__global__ __launch_bounds__(64 * ranked::kWaves) void k_featrank_join(TargetKey *__restrict__ keys, prb_featrank_pair *__restrict__ slots,
                                                                      int32_t *__restrict__ fill, const TargetKey *__restrict__ skeys,
                                                                      const prb_featrank_pair *__restrict__ sslots, const int32_t *__restrict__ sfill,
                                                                      int64_t nfeat, int32_t n) {
  extern __shared__ TargetKey frk_lds[];
  ranked::join_lists(frk_lds, keys, slots, fill, skeys, sslots, sfill, nfeat, n);
}
__global__ __launch_bounds__(kBlock) void k_featrank_gather(const TargetKey *__restrict__ keys, const prb_featrank_pair *__restrict__ slots,
                                                            const int64_t *__restrict__ off, int64_t nfeat, int32_t n, int64_t total,
                                                            prb_featrank_pair *__restrict__ out) {
  ranked::gather_ranked(keys, slots, off, nfeat, n, total, out, (int64_t)blockIdx.x * kBlock + threadIdx.x);
}

TableSource table_source(const FeatRankFeed &t) {
  return TableSource{static_cast<const prb_feature_pair *>(t.rec), t.nrec, t.ids, t.nq, t.nfeat};
}
RecordSource record_source(const void *rec, int64_t nrec, int32_t nfeat) {
  return RecordSource{static_cast<const prb_featrank_pair *>(rec), nrec, nfeat};
}
// what every launch over candidates checks of their number: a candidate's name is 32 bits, all ones = none
bool candidates_ok(int64_t ncand, int32_t nfeat) { return ncand >= 0 && ncand <= INT32_MAX && nfeat >= 1; }

template <class Source>
hipError_t launch_merge(const Source &src, const GroupRankRuns &r, int32_t nfeat, int32_t n, TargetKey *keys, void *slots, int32_t *fill,
                        hipStream_t s) {
  if (r.nruns <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN || nfeat < 1 || r.ncand > INT32_MAX || r.nruns > r.ncand) return hipErrorInvalidValue;
  const size_t per_wave = ranked::merge_lds(n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_featrank_merge<Source>, r.nruns * 64, 64 * waves, per_wave * waves, s, src, r.rkey, r.group_of, r.start, r.nruns, r.ncand,
                   nfeat, n, keys, static_cast<prb_featrank_pair *>(slots), fill);
}

} // namespace

hipError_t launch_featrank_table_features(const FeatRankFeed &t, uint32_t *key, uint32_t *val, uint32_t *bad, hipStream_t s) {
  if (!candidates_ok(t.nrec, t.nfeat)) return hipErrorInvalidValue;
  return launch_1d(k_featrank_features<TableSource>, t.nrec, kBlock, 0, s, table_source(t), t.nrec, key, val, bad);
}
hipError_t launch_featrank_table_runs(const FeatRankFeed &t, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head,
                                      uint32_t *bad, hipStream_t s) {
  if (!candidates_ok(t.nrec, t.nfeat) || t.nq < 1 || !t.ids) return hipErrorInvalidValue;
  return launch_1d(k_featrank_runs<TableSource>, t.nrec, kBlock, 0, s, table_source(t), t.nrec, key, val, rkey, head, bad);
}
hipError_t launch_featrank_table_merge(const FeatRankFeed &t, const GroupRankRuns &r, int32_t n, TargetKey *keys, void *slots, int32_t *fill,
                                       hipStream_t s) {
  if (r.ncand != t.nrec || !t.ids) return hipErrorInvalidValue;
  return launch_merge(table_source(t), r, t.nfeat, n, keys, slots, fill, s);
}
hipError_t launch_featrank_record_features(const void *rec, int64_t nrec, int32_t nfeat, uint32_t *key, uint32_t *val, uint32_t *bad,
                                           hipStream_t s) {
  if (!candidates_ok(nrec, nfeat)) return hipErrorInvalidValue;
  return launch_1d(k_featrank_features<RecordSource>, nrec, kBlock, 0, s, record_source(rec, nrec, nfeat), nrec, key, val, bad);
}
hipError_t launch_featrank_record_runs(const void *rec, int64_t nrec, int32_t nfeat, const uint32_t *key, const uint32_t *val, TargetKey *rkey,
                                       uint8_t *head, uint32_t *bad, hipStream_t s) {
  if (!candidates_ok(nrec, nfeat)) return hipErrorInvalidValue;
  return launch_1d(k_featrank_runs<RecordSource>, nrec, kBlock, 0, s, record_source(rec, nrec, nfeat), nrec, key, val, rkey, head, bad);
}
hipError_t launch_featrank_record_merge(const void *rec, int64_t nrec, const GroupRankRuns &r, int32_t nfeat, int32_t n, TargetKey *keys,
                                        void *slots, int32_t *fill, hipStream_t s) {
  if (r.ncand != nrec) return hipErrorInvalidValue;
  return launch_merge(record_source(rec, nrec, nfeat), r, nfeat, n, keys, slots, fill, s);
}
hipError_t launch_featrank_join(TargetKey *keys, void *slots, int32_t *fill, const TargetKey *skeys, const void *sslots, const int32_t *sfill,
                                int64_t nfeat, int32_t n, hipStream_t s) {
  if (nfeat <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t per_wave = ranked::join_lds(n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_featrank_join, nfeat * 64, 64 * waves, per_wave * waves, s, keys, static_cast<prb_featrank_pair *>(slots), fill, skeys,
                   static_cast<const prb_featrank_pair *>(sslots), sfill, nfeat, n);
}
hipError_t launch_featrank_gather(const TargetKey *keys, const void *slots, const int64_t *off, int64_t nfeat, int32_t n, int64_t total,
                                  void *out, hipStream_t s) {
  if (nfeat <= 0 || n < 1) return total > 0 ? hipErrorInvalidValue : hipSuccess;
  return launch_1d(k_featrank_gather, total, kBlock, 0, s, keys, static_cast<const prb_featrank_pair *>(slots), off, nfeat, n, total,
                   static_cast<prb_featrank_pair *>(out));
}

} // namespace prb
