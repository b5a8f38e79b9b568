// Benjamini-Hochberg q-values of the null table on gfx950: per observed (query, target) pair the rank of its p-value
// among its query's pairs and the step-up minimum of tests * num / (den * rank) (prb_nullset_finish_fdr, `ris -t -z N -Q`).
// The reference has no counterpart: the definitions are in include/priblast_hip.h, the exactness argument in DESIGN.md.
//
// A p-value is the rational (null_le + 1) / (decoys + 1) of a slot.  The host sorts the pairs by (query, p-key) - the
// sort is capi_search.hip's -, then the passes work on sorted segments as the evalset's do (eval_kernels.hip): ranks are
// the ends of runs of equal keys, the q-value is a suffix minimum of fractions compared by cross-multiplication in 64
// bits.  Integers only.  Every kernel checks what it indexes with against the table's ranges before it writes: a
// violation raises `bad` and writes nothing (the host call fails).
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"
#include "stepup_device.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_null_fdr) == 24, "a figure moves as 3 x 8 bytes");
static_assert(kFdrChunk % 64 == 0 && kFdrChunk <= 1024, "k_fdr_stepup: whole wavefronts, one workgroup");

// k_fdr_keys: a lane per place j of the selection.  The lanes of a wavefront that hold pairs of one query are found by
// ballot, and their first lane adds the popcount to the query's count (the places ascend by slot, so a wavefront holds
// few queries: the loop runs once per query present).  No lane leaves before the ballots.
__global__ __launch_bounds__(kBlock) void k_fdr_keys(NullTab t, const uint32_t *__restrict__ sel, int64_t n, unsigned long long *__restrict__ key,
                                                     uint32_t *__restrict__ place, uint2 *__restrict__ frac, uint32_t *cnt) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool ok = j < n;
  int32_t q = -1;
  if (ok) {
    const int64_t slot = (int64_t)sel[j];
    ok = slot < t.nslots && t.ntargets > 0;
    if (ok) {
      const NullSlot &s = t.slot[slot];
      q = (int32_t)(slot / t.ntargets);
      const unsigned long long num = s.null_le + 1ull, den = (unsigned long long)(s.seen ? s.seen : (uint32_t)t.ndecoys) + 1ull;
      ok = q < t.nq && s.observed && den <= kFdrMaxDen && num <= den;
      if (ok) {
        key[j] = ((unsigned long long)q << kFdrKeyBits) | ((num << 40) / den);
        place[j] = (uint32_t)j;
        frac[j] = make_uint2((uint32_t)num, (uint32_t)den);
      }
    }
    if (!ok) atomicOr(t.bad, 1u);
  }
  unsigned long long todo = __ballot(ok);
  while (todo) { // (wavefront-uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const int32_t ql = __shfl(q, lead);
    const unsigned long long same = __ballot(ok && q == ql);
    if (lane == lead) atomicAdd(&cnt[ql], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// k_fdr_rank: a lane per sorted entry i.  Its query is in its key; its run of equal keys - equal p-values - ends at the
// upper bound of the key in the query's segment and starts at the lower bound.
__global__ __launch_bounds__(kBlock) void k_fdr_rank(FdrTab f) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= f.n) return;
  const unsigned long long k = f.key[i];
  const unsigned long long q = k >> kFdrKeyBits;
  const int64_t p = (int64_t)f.place[i];
  int64_t s0, s1;
  if (q >= (unsigned long long)f.nq || p >= f.n || !segment_bounds(f.off, (int32_t)q, f.n, &s0, &s1) || i < s0 || i >= s1) {
    atomicOr(f.bad, 1u);
    return;
  }
  int64_t a = s0, b = i; // the first place in [s0, i] whose key is not below k
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (f.key[m] < k) a = m + 1;
    else b = m;
  }
  const uint2 x = f.frac[p];
  f.ent[i] = make_uint4(x.x, x.y, (uint32_t)(sorted_upper(f.key, i + 1, s1, k) - s0), (uint32_t)(a - s0));
}

// An entry (num, den, rank, .) of the suffix minimum stands for the fraction num / (den * rank) - the query's tests are a
// common factor -; den = 0 is "none", which compares above every entry.  A total order: the fraction by
// cross-multiplication (num, den <= kFdrMaxDen and rank < 2^30, so both products are below 2^64), then the lower rank,
// then the lower den.
__device__ __forceinline__ bool fdr_below(uint4 a, uint4 b) {
  if (a.y == 0u) return false;
  if (b.y == 0u) return true;
  const uint64_t l = (uint64_t)a.x * ((uint64_t)b.y * b.z), r = (uint64_t)b.x * ((uint64_t)a.y * a.z);
  if (l != r) return l < r;
  if (a.z != b.z) return a.z < b.z;
  return a.y < b.y;
}

// k_fdr_stepup: the workgroup of query blockIdx.x walks the query's segment from its end in chunks of kFdrChunk, thread
// t of a chunk at the entry t places below the chunk's top (chunk_suffix_min, stepup_device.hpp).
__global__ __launch_bounds__(kFdrChunk) void k_fdr_stepup(FdrTab f) {
  constexpr int kWaves = kFdrChunk / 64;
  __shared__ uint4 wave_total[kWaves];
  const int32_t q = (int32_t)blockIdx.x;
  int64_t lo, hi;
  if (q >= f.nq || !segment_bounds(f.off, q, f.n, &lo, &hi)) { // (the same for every thread)
    if (threadIdx.x == 0) atomicOr(f.bad, 1u);
    return;
  }
  const int64_t tests = f.tests[q];
  uint4 carry = make_uint4(0u, 0u, 0u, 0u);
  for (int64_t top = hi; top > lo; top -= kFdrChunk) {
    const int64_t p = top - 1 - (int64_t)threadIdx.x;
    const bool live = p >= lo;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
      v = f.ent[p];
      v.w = 0u;
    }
    v = chunk_suffix_min<kWaves>(v, carry, wave_total, [](uint4 above, uint4 below) { return fdr_below(below, above) ? below : above; });
    if (live) {
      // min(1, v): a minimum above 1 is stored as (0, 0, 0)
      if ((uint64_t)tests * v.x > (uint64_t)v.y * v.z) v = make_uint4(0u, 0u, 0u, 0u);
      f.qv[p] = make_uint4(v.x, v.y, v.z, 0u);
    }
  }
}

// k_fdr_scatter: a lane per sorted entry i: the figures of its pair to the pair's place in record order.  The triple is
// the one at the start of its run: the minimum over every pair whose p-value is not below its own.
__global__ __launch_bounds__(kBlock) void k_fdr_scatter(FdrTab f, prb_null_fdr *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= f.n) return;
  const unsigned long long q = f.key[i] >> kFdrKeyBits;
  const int64_t p = (int64_t)f.place[i];
  int64_t s0, s1;
  if (q >= (unsigned long long)f.nq || p >= f.n || !segment_bounds(f.off, (int32_t)q, f.n, &s0, &s1) || i < s0 || i >= s1) {
    atomicOr(f.bad, 1u);
    return;
  }
  const uint4 e = f.ent[i];
  const int64_t first = s0 + (int64_t)e.w;
  if (first > i) {
    atomicOr(f.bad, 1u);
    return;
  }
  const uint4 v = f.qv[first];
  prb_null_fdr r;
  r.tests = f.tests[q];
  r.rank = e.z;
  r.q_rank = v.z;
  r.q_num = v.x;
  r.q_den = v.y;
  out[p] = r;
}

} // namespace

hipError_t launch_fdr_keys(const NullTab &t, const uint32_t *sel, int64_t n, unsigned long long *key, uint32_t *place, uint2 *frac,
                           uint32_t *cnt, hipStream_t s) {
  return launch_1d(k_fdr_keys, n, kBlock, 0, s, t, sel, n, key, place, frac, cnt);
}
hipError_t launch_fdr_rank(const FdrTab &f, hipStream_t s) { return launch_1d(k_fdr_rank, f.n, kBlock, 0, s, f); }
hipError_t launch_fdr_stepup(const FdrTab &f, hipStream_t s) {
  if (f.nq <= 0 || f.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fdr_stepup, dim3((unsigned)f.nq), dim3(kFdrChunk), 0, s, f);
  return hipGetLastError();
}
hipError_t launch_fdr_scatter(const FdrTab &f, void *out, hipStream_t s) {
  return launch_1d(k_fdr_scatter, f.n, kBlock, 0, s, f, static_cast<prb_null_fdr *>(out));
}

} // namespace prb
