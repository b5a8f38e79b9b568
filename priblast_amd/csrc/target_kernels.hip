// The per-target table on gfx950: each database sequence's N best queries (prb_search_page_targets, `ris -r`) over all
// the queries of a run, ranked on the device; the merge of two such tables (prb_targetset_merge) and the gather of the
// finish.  The reference has no counterpart: the records and the order are defined in include/priblast_hip.h.
//
// A target t (its page's first target + db_id) is a list of rank_kernels.hpp - ranked keys, payload slots that never
// move, a fill count -, and the merges and the gather are that file's; here are the payload (prb_target_pair), where a
// newcomer's comes from (the sub-batch's pair records) and the grouping of a sub-batch's records by target.
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "rank_kernels.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_target_pair) == 72 && sizeof(TargetKey) == 16,
              "a payload moves as 8 (+ 1) x 8 bytes, a key as 16");
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

// the newcomers of a sub-batch: its pair records, all of `page`
struct PairSource {
  const prb_pair_summary *rec;
  int64_t nrec;
  int32_t page;
  __device__ __forceinline__ uint32_t limit() const { return (uint32_t)nrec; }
  __device__ __forceinline__ void put(prb_target_pair *to, const TargetKey &c) const { put_payload(to, rec + c.at, page); }
};

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

// ---- the merge of a sub-batch into the table, of two tables, and the finish: rank_kernels.hpp ----
// run r of rkey is target tbase + db_of[start[r]] of `page`
__global__ __launch_bounds__(64 * ranked::kWaves) void k_target_merge(const prb_pair_summary *__restrict__ rec, const TargetKey *__restrict__ rkey,
                                                                     const uint32_t *__restrict__ db_of, const uint32_t *__restrict__ start,
                                                                     int64_t nruns, int64_t nrec, int32_t page, int64_t tbase, int32_t nseq,
                                                                     int32_t n, TargetKey *__restrict__ keys, prb_target_pair *__restrict__ slots,
                                                                     int32_t *__restrict__ fill) {
  extern __shared__ TargetKey tgt_lds[];
  ranked::merge_runs(tgt_lds, PairSource{rec, nrec, page}, rkey, db_of, start, nruns, nrec, tbase, nseq, n, keys, slots, fill);
}
__global__ __launch_bounds__(64 * ranked::kWaves) void k_target_join(TargetKey *__restrict__ keys, prb_target_pair *__restrict__ slots,
                                                                    int32_t *__restrict__ fill, const TargetKey *__restrict__ skeys,
                                                                    const prb_target_pair *__restrict__ sslots, const int32_t *__restrict__ sfill,
                                                                    int64_t ntargets, int32_t n) {
  extern __shared__ TargetKey tgt_lds[];
  ranked::join_lists(tgt_lds, keys, slots, fill, skeys, sslots, sfill, ntargets, n);
}
__global__ __launch_bounds__(kBlock) void k_target_gather(const TargetKey *__restrict__ keys, const prb_target_pair *__restrict__ slots,
                                                          const int64_t *__restrict__ off, int64_t ntargets, int32_t n, int64_t total,
                                                          prb_target_pair *__restrict__ out) {
  ranked::gather_ranked(keys, slots, off, ntargets, n, total, out, (int64_t)blockIdx.x * kBlock + threadIdx.x);
}

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
  const size_t per_wave = ranked::merge_lds(n);
  const int waves = ranked::waves_for(per_wave);
  return launch_1d(k_target_merge, nruns * 64, 64 * waves, per_wave * waves, s, static_cast<const prb_pair_summary *>(rec), rkey, db_of, start,
                   nruns, nrec, page, tbase, nseq, n, keys, static_cast<prb_target_pair *>(slots), fill);
}
hipError_t launch_target_join(TargetKey *keys, void *slots, int32_t *fill, const TargetKey *skeys, const void *sslots, const int32_t *sfill,
                              int64_t ntargets, int32_t n, hipStream_t s) {
  if (ntargets <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t per_wave = ranked::join_lds(n);
  const int waves = ranked::waves_for(per_wave);
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
