// The per-query cut of the feature table on gfx950: each query's n best (query, feature) records
// (prb_featset_finish_top, prb_fnullset_create_top, `ris -t -A FILE -N K`), selected on the device before the records
// leave it.  The reference has no counterpart: the rank key and the order are defined in include/priblast_hip.h.
//
// The selection works on the records as k_feat_gather leaves them - query q's records are the segment
// [ioff[q * npages], ioff[(q + 1) * npages]) of them - and ranks by (energy_key(e_min), place in the segment): a total
// order without equal keys, so every pass is a count or a comparison and the result does not depend on how the work is
// cut.  A feature table is not dense and one query may own all of it, so a workgroup per query is not enough: the
// segments are cut into chunks of kFtopChunk records, a workgroup per (query, chunk) orders its chunk in LDS and writes
// the chunk's min(n, length) lowest keys to a partials buffer; then a workgroup per query folds its chunks' lists into
// the final n (k_group_select's scheme: the kept keys stay in front, the rest of the buffer is refilled from the next
// partials, the whole is ordered again); then a lane per kept record gathers it in (query, rank) order.
//
// LDS: a key is 8 B of energy key and 4 B of place, kept as two arrays so that the lanes of a compare-exchange step touch
// consecutive words: kFtopChunk x 12 B = 24 KiB per workgroup, in both ordering kernels (six such workgroups fit a
// compute unit's 160 KiB).  Every kernel checks its indices against the table's ranges before it writes: a violation
// raises `bad` and writes nothing.
#include "../../include/priblast_hip.h"

#include "feature_device.hpp"
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

static_assert(sizeof(prb_feature_pair) == 80, "a record moves as 10 x 8 bytes");
static_assert((kFtopChunk & (kFtopChunk - 1)) == 0 && kFtopChunk >= 2 * kTopMaxN, "a chunk holds n candidates beside n kept keys");

constexpr unsigned long long kNoKey = ~0ull; // an entry without a record: with the place 2^32 - 1, behind every other
constexpr uint32_t kNoPlace = ~0u;

// query q's segment of the gathered records: false (and `bad` raised by the caller) when it lies outside them
__device__ __forceinline__ bool ftop_segment(const FtopTab &t, int64_t q, int64_t *s0, int64_t *len) {
  const int64_t a = t.ioff[q * t.npages], b = t.ioff[(q + 1) * t.npages];
  *s0 = a;
  *len = b - a;
  return a >= 0 && a <= b && b <= t.total && b - a < (int64_t)kNoPlace;
}

// s_e / s_p [kFtopChunk] ascending by (energy key, place): bitonic, every thread of the workgroup takes part
__device__ __forceinline__ void ftop_sort(unsigned long long *s_e, uint32_t *s_p) {
  for (int k = 2; k <= kFtopChunk; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = threadIdx.x; x < kFtopChunk; x += kBlock) {
        const int y = x ^ j;
        if (y > x) {
          const bool up = (x & k) == 0;
          const unsigned long long ex = s_e[x], ey = s_e[y];
          const uint32_t px = s_p[x], py = s_p[y];
          const bool x_above = ex > ey || (ex == ey && px > py);
          if (x_above == up) {
            s_e[x] = ey, s_e[y] = ex;
            s_p[x] = py, s_p[y] = px;
          }
        }
      }
      __syncthreads();
    }
}

// a lane per query (and one more, which writes the scans' last element): its chunks and its kept records
__global__ __launch_bounds__(kBlock) void k_ftop_counts(FtopTab t, int64_t *__restrict__ nchunk, int64_t *__restrict__ nkeep) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q > t.nq) return;
  int64_t c = 0, k = 0;
  if (q < t.nq) {
    int64_t s0, len;
    if (!ftop_segment(t, q, &s0, &len)) atomicOr(t.bad, 1u);
    else {
      c = (len + kFtopChunk - 1) / kFtopChunk;
      k = min(len, (int64_t)t.n);
    }
  }
  nchunk[q] = c;
  nkeep[q] = k;
}

// workgroup w = chunk w - choff[q] of the query q whose chunks begin at choff[q]: its keys ordered, the lowest
// min(n, length) to pe / pp [w * n + r]
__global__ __launch_bounds__(kBlock) void k_ftop_chunks(FtopTab t, const prb_feature_pair *__restrict__ rec, const int64_t *__restrict__ choff,
                                                        int64_t nchunks, unsigned long long *__restrict__ pe, uint32_t *__restrict__ pp) {
  __shared__ unsigned long long s_e[kFtopChunk];
  __shared__ uint32_t s_p[kFtopChunk];
  const int64_t w = blockIdx.x;
  if (w >= nchunks) return; // (uniform over the workgroup, as every exit below)
  const int64_t q = item_run(choff, (int64_t)t.nq, w);
  int64_t s0, len;
  if (!ftop_segment(t, q, &s0, &len)) {
    if (threadIdx.x == 0) atomicOr(t.bad, 1u);
    return;
  }
  const int64_t p0 = (w - choff[q]) * kFtopChunk; // the chunk's first place
  if (w < choff[q] || w >= choff[q + 1] || p0 >= len) {
    if (threadIdx.x == 0) atomicOr(t.bad, 1u);
    return;
  }
  const int64_t m = min(len - p0, (int64_t)kFtopChunk);
  for (int x = threadIdx.x; x < kFtopChunk; x += kBlock) {
    const bool in = x < m;
    s_e[x] = in ? (unsigned long long)energy_key(rec[s0 + p0 + x].s.e_min) : kNoKey;
    s_p[x] = in ? (uint32_t)(p0 + x) : kNoPlace;
  }
  __syncthreads();
  ftop_sort(s_e, s_p);
  const int out = (int)min(m, (int64_t)t.n);
  for (int r = threadIdx.x; r < out; r += kBlock) {
    pe[w * t.n + r] = s_e[r];
    pp[w * t.n + r] = s_p[r];
  }
}

// workgroup q folds the lists of query q's chunks: top[q * n + r] = the place of its record of rank r.  Every chunk but
// the last is full and has written n keys, so candidate x of the query is key x % n of its chunk x / n.
__global__ __launch_bounds__(kBlock) void k_ftop_merge(FtopTab t, const int64_t *__restrict__ choff, int64_t nchunks,
                                                       const unsigned long long *__restrict__ pe, const uint32_t *__restrict__ pp,
                                                       uint32_t *__restrict__ top) {
  __shared__ unsigned long long s_e[kFtopChunk];
  __shared__ uint32_t s_p[kFtopChunk];
  const int64_t q = blockIdx.x;
  if (q >= t.nq) return;
  int64_t s0, len;
  const int64_t w0 = choff[q], nch = choff[q + 1] - w0;
  if (nch == 0) return;
  if (!ftop_segment(t, q, &s0, &len) || w0 < 0 || nch < 0 || w0 + nch > nchunks || nch != (len + kFtopChunk - 1) / kFtopChunk) {
    if (threadIdx.x == 0) atomicOr(t.bad, 1u);
    return;
  }
  const int n = t.n;
  const int64_t last = min(len - (nch - 1) * kFtopChunk, (int64_t)n); // the keys of the last chunk
  const int64_t ncand = (nch - 1) * n + last;
  const int keep = (int)min(len, (int64_t)n);
  if (nch == 1) { // (one list, ordered already)
    for (int r = threadIdx.x; r < keep; r += kBlock) {
      const uint32_t p = pp[w0 * n + r];
      if ((int64_t)p < len) top[q * n + r] = p;
      else atomicOr(t.bad, 1u);
    }
    return;
  }
  int kept = 0; // entries in front that stay
  int64_t at = 0;
  do {
    const int room = kFtopChunk - kept;
    for (int x = threadIdx.x; x < room; x += kBlock) {
      unsigned long long e = kNoKey;
      uint32_t p = kNoPlace;
      if (at + x < ncand) {
        const int64_t src = w0 * n + at + x; // (the lists of a query's full chunks stand one behind the other)
        e = pe[src];
        p = pp[src];
        if ((int64_t)p >= len) {
          atomicOr(t.bad, 1u);
          e = kNoKey;
          p = kNoPlace;
        }
      }
      s_e[kept + x] = e;
      s_p[kept + x] = p;
    }
    at += room;
    __syncthreads();
    ftop_sort(s_e, s_p);
    kept = n;
  } while (at < ncand);
  for (int r = threadIdx.x; r < keep; r += kBlock) {
    const uint32_t p = s_p[r];
    if ((int64_t)p < len) top[q * n + r] = p;
    else atomicOr(t.bad, 1u);
  }
}

// out[o] = the record of rank o - koff[q] of the query q whose kept records begin at koff[q]
__global__ __launch_bounds__(kBlock) void k_ftop_gather(FtopTab t, const prb_feature_pair *__restrict__ rec, const int64_t *__restrict__ koff,
                                                        const uint32_t *__restrict__ top, int64_t nkept, prb_feature_pair *__restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o >= nkept) return;
  const int64_t q = item_run(koff, (int64_t)t.nq, o);
  const int64_t r = o - koff[q];
  int64_t s0, len;
  if (!ftop_segment(t, q, &s0, &len) || r < 0 || r >= t.n || o >= koff[q + 1]) {
    atomicOr(t.bad, 1u);
    return;
  }
  const int64_t p = (int64_t)top[q * t.n + r];
  if (p >= len || rec[s0 + p].s.query != (int32_t)q) {
    atomicOr(t.bad, 1u);
    return;
  }
  uint2 v[10];
#pragma unroll
  for (int w = 0; w < 10; w++) v[w] = reinterpret_cast<const uint2 *>(rec + s0 + p)[w];
#pragma unroll
  for (int w = 0; w < 10; w++) reinterpret_cast<uint2 *>(out + o)[w] = v[w];
}

bool tab_ok(const FtopTab &t) { return t.nq >= 1 && t.npages >= 1 && t.n >= 1 && t.n <= kTopMaxN && t.total >= 0; }

} // namespace

hipError_t launch_ftop_counts(const FtopTab &t, int64_t *nchunk, int64_t *nkeep, hipStream_t s) {
  if (!tab_ok(t)) return hipErrorInvalidValue;
  return launch_1d(k_ftop_counts, (int64_t)t.nq + 1, kBlock, 0, s, t, nchunk, nkeep);
}
hipError_t launch_ftop_chunks(const FtopTab &t, const void *rec, const int64_t *choff, int64_t nchunks, unsigned long long *pe, uint32_t *pp,
                              hipStream_t s) {
  if (nchunks <= 0) return hipSuccess;
  if (!tab_ok(t) || nchunks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ftop_chunks, dim3((unsigned)nchunks), dim3(kBlock), 0, s, t, static_cast<const prb_feature_pair *>(rec), choff, nchunks, pe, pp);
  return hipGetLastError();
}
hipError_t launch_ftop_merge(const FtopTab &t, const int64_t *choff, int64_t nchunks, const unsigned long long *pe, const uint32_t *pp,
                             uint32_t *top, hipStream_t s) {
  if (nchunks <= 0) return hipSuccess;
  if (!tab_ok(t)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ftop_merge, dim3((unsigned)t.nq), dim3(kBlock), 0, s, t, choff, nchunks, pe, pp, top);
  return hipGetLastError();
}
hipError_t launch_ftop_gather(const FtopTab &t, const void *rec, const int64_t *koff, const uint32_t *top, int64_t nkept, void *out,
                              hipStream_t s) {
  if (!tab_ok(t)) return hipErrorInvalidValue;
  return launch_1d(k_ftop_gather, nkept, kBlock, 0, s, t, static_cast<const prb_feature_pair *>(rec), koff, top, nkept,
                   static_cast<prb_feature_pair *>(out));
}

} // namespace prb
