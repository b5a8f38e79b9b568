// What the two step-up kernels share (k_eval_qmin, eval_kernels.hip; k_fdr_stepup, fdr_kernels.hip): the suffix minimum
// of one chunk of a sorted segment, taken by a workgroup of whole wavefronts that walks the segment from its end.
#pragma once
#include <hip/hip_runtime.h>

namespace prb {

// the first place in key[a, b) whose key is above k (b when there is none)
__device__ __forceinline__ int64_t sorted_upper(const unsigned long long *__restrict__ key, int64_t a, int64_t b, unsigned long long k) {
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (key[m] <= k) a = m + 1;
    else b = m;
  }
  return a;
}

// the bounds [*s0, *s1) of query q's segment in a list of n entries, or false when they are not an order within the list
__device__ __forceinline__ bool segment_bounds(const int64_t *__restrict__ off, int32_t q, int64_t n, int64_t *s0, int64_t *s1) {
  *s0 = off[q];
  *s1 = off[q + 1];
  return *s0 >= 0 && *s0 <= *s1 && *s1 <= n;
}

// v of the lane d places below (a lane below d gets its own back)
__device__ __forceinline__ uint2 lane_up(uint2 v, int d) { return make_uint2(__shfl_up(v.x, d), __shfl_up(v.y, d)); }
__device__ __forceinline__ uint4 lane_up(uint4 v, int d) {
  return make_uint4(__shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.w, d));
}

// Thread t of the workgroup holds the entry t places below the chunk's top, so an inclusive scan in thread order is a
// suffix minimum in key order: __shfl_up within the wavefront, the wavefronts' totals through LDS (wave_total[kWaves]),
// and `carry` = the minimum over all the chunks above, which every thread keeps in registers and which leaves as the
// minimum over this chunk too.  min_of(above, below) = the minimum of entries of higher keys and of lower keys.  Every
// thread of the workgroup calls it; wave_total is free again on return.
template <int kWaves, class T, class Min> __device__ __forceinline__ T chunk_suffix_min(T v, T &carry, T *wave_total, Min min_of) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T above = lane_up(v, d);
    if (lane >= d) v = min_of(above, v);
  }
  if (lane == 63) wave_total[wave] = v;
  __syncthreads();
  T pre = carry; // everything above this wavefront's entries
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    if (w == wave) v = min_of(pre, v);
    pre = min_of(pre, wave_total[w]);
  }
  carry = pre; // ... and above the next chunk's
  __syncthreads(); // (wave_total is written again)
  return v;
}

} // namespace prb
