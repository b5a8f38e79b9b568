// The evalset on gfx950: an E-value and an FDR q-value for every interaction site of a batch from the pooled hits of its
// decoys (prb_evalset_*, `ris -k N -E M`).  The reference has no counterpart: the definitions are in
// include/priblast_hip.h.
//
// Two lists of (owner query, energy key).  They only grow until the close, which sorts both by (query, key) - the sorts
// are the host's (capi_eval.hip) - and then works on sorted segments: ranks are upper bounds, the q-value is a suffix
// minimum of fractions compared by cross-multiplication in 64 bits.  Integers only.  Every kernel checks what it indexes
// with against the table's ranges before it writes: a violation raises `bad` and writes nothing (the next host call fails).
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"
#include "stepup_device.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_eval_score) == 32, "a score moves as 4 x 8 bytes");
static_assert(kEvalChunk % 64 == 0 && kEvalChunk <= 1024, "k_eval_qmin: whole wavefronts, one workgroup");

// prb_search_page_scored / _null_hits (per sub-batch) and prb_evalset_add_keys: hit i of n to place i behind the list's end
__global__ __launch_bounds__(kBlock) void k_eval_append(const int32_t *__restrict__ ids, const double *__restrict__ energy, int64_t n,
                                                        const int32_t *__restrict__ owner, const int32_t *__restrict__ decoy, int32_t ndq,
                                                        int32_t nq, int32_t ndecoys, unsigned long long *__restrict__ key,
                                                        uint32_t *__restrict__ own, uint32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int32_t q = ids[i];
  if (owner) { // a decoy batch's query: its owner, and its decoy number within the table's
    if (q < 0 || q >= ndq) {
      atomicOr(bad, 1u);
      return;
    }
    const int32_t d = decoy[q];
    q = owner[q];
    if (d < 0 || d >= ndecoys) {
      atomicOr(bad, 1u);
      return;
    }
  }
  if (q < 0 || q >= nq) {
    atomicOr(bad, 1u);
    return;
  }
  key[i] = energy_key(energy[i]);
  own[i] = (uint32_t)q;
}

__global__ __launch_bounds__(kBlock) void k_eval_iota(uint32_t *v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// dst[i] = src[idx[i]]: the lists permuted by what a sort left
template <class T>
__global__ __launch_bounds__(kBlock) void k_eval_gather(const T *__restrict__ src, const uint32_t *__restrict__ idx, T *__restrict__ dst, int64_t n,
                                                        uint32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t j = (int64_t)idx[i];
  if (j >= n) {
    atomicOr(bad, 1u);
    return;
  }
  dst[i] = src[j];
}

// the queries' segment sizes
__global__ __launch_bounds__(kBlock) void k_eval_count(const uint32_t *__restrict__ own, int64_t n, int32_t nq, uint32_t *cnt, uint32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = own[i];
  if (q >= (uint32_t)nq) {
    atomicOr(bad, 1u);
    return;
  }
  atomicAdd(&cnt[q], 1u);
}

// k_eval_rank: a lane per real entry i.  Its query is the segment that i lies in; its rank the upper bound of its key in
// that segment - so equal keys share it -, its null_le the upper bound in the same query's decoy segment.
__global__ __launch_bounds__(kBlock) void k_eval_rank(EvalTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= t.nreal) return;
  int32_t lo = 0, hi = t.nq; // roff[lo] <= i < roff[hi] (empty segments have equal bounds: the last one at or below i is i's)
  while (hi - lo > 1) {
    const int32_t m = (lo + hi) >> 1;
    if (t.roff[m] <= i) lo = m;
    else hi = m;
  }
  int64_t r0, r1, d0, d1;
  if (!segment_bounds(t.roff, lo, t.nreal, &r0, &r1) || i < r0 || i >= r1 || !segment_bounds(t.doff, lo, t.ndecoy, &d0, &d1)) {
    atomicOr(t.bad, 1u);
    return;
  }
  const unsigned long long k = t.rkey[i];
  t.rank[i] = (uint32_t)(sorted_upper(t.rkey, i + 1, r1, k) - r0);
  t.null_le[i] = (uint32_t)(sorted_upper(t.dkey, d0, d1, k) - d0);
}

// A fraction x / y of the suffix minimum: null_le / rank of one real entry (rank >= 1), or "none" = (all ones) / 0, which
// compares above every entry.  a <= b by cross-multiplication: both factors are below 2^32.
constexpr uint32_t kEvalNoneNum = 0xFFFFFFFFu;
__device__ __forceinline__ bool eval_le(uint2 a, uint2 b) { return (uint64_t)a.x * b.y <= (uint64_t)b.x * a.y; }
// the minimum of `above` (entries of higher keys) and `below` (of lower keys): equal fractions go to the lower key
__device__ __forceinline__ uint2 eval_min(uint2 above, uint2 below) { return eval_le(below, above) ? below : above; }

// k_eval_qmin: the workgroup of query blockIdx.x walks the query's segment from its end in chunks of kEvalChunk.  Thread
// t of a chunk has the entry t places below the chunk's top; the chunk's suffix minimum and the carry over the chunks
// above are chunk_suffix_min's (stepup_device.hpp).
__global__ __launch_bounds__(kEvalChunk) void k_eval_qmin(EvalTab t) {
  constexpr int kWaves = kEvalChunk / 64;
  __shared__ uint2 wave_total[kWaves];
  const int32_t q = (int32_t)blockIdx.x;
  int64_t lo, hi;
  if (!segment_bounds(t.roff, q, t.nreal, &lo, &hi)) { // (the same for every thread)
    if (threadIdx.x == 0) atomicOr(t.bad, 1u);
    return;
  }
  uint2 carry = make_uint2(kEvalNoneNum, 0u);
  for (int64_t top = hi; top > lo; top -= kEvalChunk) {
    const int64_t p = top - 1 - (int64_t)threadIdx.x;
    const bool live = p >= lo;
    uint2 v = live ? make_uint2(t.null_le[p], t.rank[p]) : make_uint2(kEvalNoneNum, 0u);
    v = chunk_suffix_min<kWaves>(v, carry, wave_total, [](uint2 above, uint2 below) { return eval_min(above, below); });
    if (live) {
      // min(1, v): a minimum above 1 is stored as ndecoys / (ndecoys * 1)
      if ((uint64_t)v.x > (uint64_t)t.ndecoys * v.y) v = make_uint2((uint32_t)t.ndecoys, 1u);
      t.qnum[p] = v.x;
      t.qden[p] = v.y;
    }
  }
}

// prb_evalset_score: the first entry of the query's segment that holds the key (equal keys hold equal figures)
__global__ __launch_bounds__(kBlock) void k_eval_lookup(EvalTab t, const int32_t *__restrict__ query, const double *__restrict__ energy, int64_t n,
                                                        prb_eval_score *out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  prb_eval_score r{};
  const int32_t q = query[i];
  int64_t s0, s1;
  if (q < 0 || q >= t.nq || !segment_bounds(t.roff, q, t.nreal, &s0, &s1)) {
    atomicOr(t.bad, 1u);
    out[i] = r;
    return;
  }
  const unsigned long long k = energy_key(energy[i]);
  int64_t a = s0, b = s1;
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (t.rkey[m] < k) a = m + 1;
    else b = m;
  }
  if (a >= s1 || t.rkey[a] != k) {
    atomicOr(t.bad, 1u);
    out[i] = r;
    return;
  }
  r.decoys = t.ndecoys;
  r.null_le = (int64_t)t.null_le[a];
  r.rank = (int64_t)t.rank[a];
  r.q_num = t.qnum[a];
  r.q_den = t.qden[a];
  out[i] = r;
}

} // namespace

hipError_t launch_eval_append(const int32_t *ids, const double *energy, int64_t n, const int32_t *owner, const int32_t *decoy, int32_t ndq,
                              int32_t nq, int32_t ndecoys, unsigned long long *key, uint32_t *own, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_eval_append, n, kBlock, 0, s, ids, energy, n, owner, decoy, ndq, nq, ndecoys, key, own, bad);
}
hipError_t launch_eval_iota(uint32_t *v, int64_t n, hipStream_t s) { return launch_1d(k_eval_iota, n, kBlock, 0, s, v, n); }
hipError_t launch_eval_gather32(const uint32_t *src, const uint32_t *idx, uint32_t *dst, int64_t n, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_eval_gather<uint32_t>, n, kBlock, 0, s, src, idx, dst, n, bad);
}
hipError_t launch_eval_gather64(const unsigned long long *src, const uint32_t *idx, unsigned long long *dst, int64_t n, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_eval_gather<unsigned long long>, n, kBlock, 0, s, src, idx, dst, n, bad);
}
hipError_t launch_eval_count(const uint32_t *own, int64_t n, int32_t nq, uint32_t *cnt, uint32_t *bad, hipStream_t s) {
  return launch_1d(k_eval_count, n, kBlock, 0, s, own, n, nq, cnt, bad);
}
hipError_t launch_eval_rank(const EvalTab &t, hipStream_t s) { return launch_1d(k_eval_rank, t.nreal, kBlock, 0, s, t); }
hipError_t launch_eval_qmin(const EvalTab &t, hipStream_t s) {
  if (t.nq <= 0 || t.nreal <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_eval_qmin, dim3((unsigned)t.nq), dim3(kEvalChunk), 0, s, t);
  return hipGetLastError();
}
hipError_t launch_eval_lookup(const EvalTab &t, const int32_t *query, const double *energy, int64_t n, void *out, hipStream_t s) {
  return launch_1d(k_eval_lookup, n, kBlock, 0, s, t, query, energy, n, static_cast<prb_eval_score *>(out));
}

} // namespace prb
