// The launch that nearly every launch_* wrapper of the search kernels is: one thread per element of a list.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace prb {

// Nothing for n <= 0; else `kernel` over ceil(n / block) workgroups of `block` threads with `lds` bytes of dynamic LDS
// on stream s, and what the launch reported.  Wrappers whose grid is something else, or that launch whatever n is,
// launch by themselves.
template <class... P, class... A>
hipError_t launch_1d(void (*kernel)(P...), int64_t n, int block, size_t lds, hipStream_t s, const A &...args) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), lds, s, args...);
  return hipGetLastError();
}

} // namespace prb
