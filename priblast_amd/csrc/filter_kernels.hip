// The redundancy filter on gfx950, on a sorted hit list.
//
//   k_filter_* <-> CheckRedundancy  rna_interaction_search.cpp:387-424
//
// The driver (filter_hits, capi_search.hip) runs k_filter_init, a max-scan of the end keys, k_filter_round* until
// nothing is pending and k_filter_final*; `tiles` selects the forms that scan a window of the list in LDS (the default)
// or the plain ones (PRB_FILTER_TILES=0: the older form, which the tests compare against).
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// CheckRedundancy (rna_interaction_search.cpp:387-424) is a sequential sweep over the sorted
// list.  Its result has a closed form (DESIGN.md "redundancy filter"): with
//   R(a,b)  = a before b, a.q range contains b.q range, a.db_end >= b.db_end
//   over(i) = E_i > threshold
//   active(i) = !over(i) and no active a<i with R(a,i) and E_a <= E_i       (i scans)
//   flagA(i)  = active(i) and exists b>i: R(i,b), E_i > E_b, and no active a<i with R(a,b), E_a <= E_b
// the survivors are exactly active(i) && !flagA(i).  `active` is resolved by rounds that
// only ever turn "unknown" into a final state, so any interleaving of threads is safe.
constexpr uint8_t kUnknown = 0, kActive = 1, kInactive = 2;

struct Box {
  int qs, qe, ds, de, query;
  double e;
};
__device__ __forceinline__ Box box_of(const HitSoA &h, int64_t i) {
  Box b;
  b.qs = h.q_sp[i];
  b.ds = h.db_sp[i];
  b.qe = b.qs + US(h.q_len[i]) - 1;
  b.de = b.ds + US(h.db_len[i]) - 1;
  b.query = h.query[i];
  b.e = h.e_tot[i];
  return b;
}
__device__ __forceinline__ bool contains(const Box &a, const Box &b) { return a.qe >= b.qe && a.qs <= b.qs && a.de >= b.de; }
// running maximum of (query, db_end) packed so that a later query always dominates
__device__ __forceinline__ int64_t pack_end(int query, int de) { return ((int64_t)query << 32) | (uint32_t)de; }

__global__ __launch_bounds__(kBlock) void k_filter_init(HitSoA h, int64_t n, double thr, int64_t *end_key, uint8_t *state) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Box b = box_of(h, i);
  end_key[i] = pack_end(b.query, b.de);
  state[i] = b.e > thr ? kInactive : kUnknown;
  // (state of an over-threshold hit is "inactive": it never scans)
}

__global__ __launch_bounds__(kBlock) void k_filter_round(HitSoA h, int64_t n, const int64_t *__restrict__ pmax,
                                                         uint8_t *state, int32_t *pending) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (state[i] != kUnknown) return;
  const Box b = box_of(h, i);
  const int64_t need = pack_end(b.query, b.de);
  bool wait = false;
  uint8_t res = kActive;
  for (int64_t a = i - 1; a >= 0; a--) {
    if (pmax[a] < need) break; // nothing at or before a (in this query) reaches b's db end
    const Box c = box_of(h, a);
    if (c.query != b.query) break;
    if (contains(c, b) && c.e <= b.e) {
      const uint8_t sa = state[a];
      if (sa == kActive) {
        res = kInactive;
        wait = false;
        break;
      }
      if (sa == kUnknown) wait = true;
    }
  }
  if (wait) {
    *pending = 1;
  } else {
    state[i] = res;
  }
}

__global__ __launch_bounds__(kBlock) void k_filter_final(HitSoA h, int64_t n, const int64_t *__restrict__ pmax,
                                                         const uint8_t *__restrict__ state, uint8_t *keep) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint8_t k = 0;
  if (state[i] == kActive) {
    k = 1;
    const Box a = box_of(h, i);
    for (int64_t j = i + 1; j < n && k; j++) {
      const Box b = box_of(h, j);
      if (b.query != a.query || b.ds > a.de) break;
      if (contains(a, b) && a.e > b.e) {
        // was b already flagged when a's scan reached it?  (by an active hit before a)
        const int64_t need = pack_end(b.query, b.de);
        bool flagged = false;
        for (int64_t c = i - 1; c >= 0; c--) {
          if (pmax[c] < need) break;
          const Box x = box_of(h, c);
          if (x.query != b.query) break;
          if (state[c] == kActive && contains(x, b) && x.e <= b.e) {
            flagged = true;
            break;
          }
        }
        if (!flagged) k = 0;
      }
    }
  }
  keep[i] = k;
}

// The same two scans on a WINDOW of the list held in LDS.  A scan is a chain of dependent loads - the running maximum,
// the box, the state of the hit before, and so on, ~4 hits back and ~4 forward - and as loads from L2 that chain is what
// the kernels above cost (0.96 / 1.5 ms per 23 M hits where the list itself is 0.1 ms of HBM traffic).  A workgroup
// loads the boxes of its 256 hits and of the neighbours on both sides once, coalesced, and scans in LDS; a scan that
// leaves the window goes on in memory.  k_filter_round_tile also repeats its round within the window until nothing
// changes (a state only ever goes from unknown to final, so more rounds, in any interleaving, give the same result):
// what is left for the next launch are the chains that cross a window.
constexpr int kFilterBack = 128, kFilterFwd = 128, kFilterWin = kFilterBack + kBlock + kFilterFwd;
struct FilterWindow {
  int qs[kFilterWin], qe[kFilterWin], ds[kFilterWin], de[kFilterWin], query[kFilterWin];
  double e[kFilterWin];
  int64_t pmax[kFilterWin];
  uint8_t state[kFilterWin];
  int64_t w0, w1; // the hits [w0, w1) of the list
};
__device__ __forceinline__ void window_load(FilterWindow &w, const HitSoA &h, int64_t n, const int64_t *__restrict__ pmax,
                                            const uint8_t *state, int64_t t0, int fwd) {
  const int64_t w0 = t0 > kFilterBack ? t0 - kFilterBack : 0;
  const int64_t w1 = t0 + kBlock + fwd < n ? t0 + kBlock + fwd : n;
  if (threadIdx.x == 0) {
    w.w0 = w0;
    w.w1 = w1;
  }
  for (int64_t g = w0 + threadIdx.x; g < w1; g += kBlock) {
    const int k = (int)(g - w0);
    const int qs = h.q_sp[g], ds = h.db_sp[g];
    w.qs[k] = qs;
    w.ds[k] = ds;
    w.qe[k] = qs + US(h.q_len[g]) - 1;
    w.de[k] = ds + US(h.db_len[g]) - 1;
    w.query[k] = h.query[g];
    w.e[k] = h.e_tot[g];
    w.pmax[k] = pmax[g];
    w.state[k] = state[g];
  }
  __syncthreads();
}
__device__ __forceinline__ Box window_box(const FilterWindow &w, const HitSoA &h, int64_t g) {
  if (g >= w.w0 && g < w.w1) {
    const int k = (int)(g - w.w0);
    return Box{w.qs[k], w.qe[k], w.ds[k], w.de[k], w.query[k], w.e[k]};
  }
  return box_of(h, g);
}
__device__ __forceinline__ int64_t window_pmax(const FilterWindow &w, const int64_t *__restrict__ pmax, int64_t g) {
  return g >= w.w0 && g < w.w1 ? w.pmax[g - w.w0] : pmax[g];
}
__device__ __forceinline__ uint8_t window_state(const FilterWindow &w, const uint8_t *state, int64_t g) {
  return g >= w.w0 && g < w.w1 ? ((const volatile uint8_t *)w.state)[g - w.w0] : ((const volatile uint8_t *)state)[g];
}

__global__ __launch_bounds__(kBlock) void k_filter_round_tile(HitSoA h, int64_t n, const int64_t *__restrict__ pmax, uint8_t *state,
                                                              int32_t *pending) {
  __shared__ FilterWindow w;
  __shared__ int s_progress;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock, i = t0 + threadIdx.x;
  window_load(w, h, n, pmax, state, t0, 0);
  bool mine = i < n && window_state(w, state, i) == kUnknown;
  const Box b = i < n ? window_box(w, h, i) : Box{0, 0, 0, 0, 0, 0.0};
  const int64_t need = pack_end(b.query, b.de);
  for (int iter = 0; iter < 64; iter++) {
    if (threadIdx.x == 0) s_progress = 0;
    __syncthreads();
    if (mine) {
      bool wait = false;
      uint8_t res = kActive;
      for (int64_t a = i - 1; a >= 0; a--) {
        if (window_pmax(w, pmax, a) < need) break; // nothing at or before a (in this query) reaches b's db end
        const Box c = window_box(w, h, a);
        if (c.query != b.query) break;
        if (contains(c, b) && c.e <= b.e) {
          const uint8_t sa = window_state(w, state, a);
          if (sa == kActive) {
            res = kInactive;
            wait = false;
            break;
          }
          if (sa == kUnknown) wait = true;
        }
      }
      if (!wait) {
        ((volatile uint8_t *)w.state)[i - w.w0] = res;
        state[i] = res;
        mine = false;
        s_progress = 1;
      }
    }
    __syncthreads();
    const int p = s_progress;
    __syncthreads();
    if (!p) break;
  }
  if (mine) *pending = 1;
}

__global__ __launch_bounds__(kBlock) void k_filter_final_tile(HitSoA h, int64_t n, const int64_t *__restrict__ pmax,
                                                              const uint8_t *__restrict__ state, uint8_t *keep) {
  __shared__ FilterWindow w;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock, i = t0 + threadIdx.x;
  window_load(w, h, n, pmax, state, t0, kFilterFwd);
  if (i >= n) return;
  uint8_t k = 0;
  if (window_state(w, state, i) == kActive) {
    k = 1;
    const Box a = window_box(w, h, i);
    for (int64_t j = i + 1; j < n && k; j++) {
      const Box b = window_box(w, h, j);
      if (b.query != a.query || b.ds > a.de) break;
      if (contains(a, b) && a.e > b.e) {
        // was b already flagged when a's scan reached it?  (by an active hit before a)
        const int64_t need = pack_end(b.query, b.de);
        bool flagged = false;
        for (int64_t c = i - 1; c >= 0; c--) {
          if (window_pmax(w, pmax, c) < need) break;
          const Box x = window_box(w, h, c);
          if (x.query != b.query) break;
          if (window_state(w, state, c) == kActive && contains(x, b) && x.e <= b.e) {
            flagged = true;
            break;
          }
        }
        if (!flagged) k = 0;
      }
    }
  }
  keep[i] = k;
}

} // namespace

hipError_t launch_filter_init(const HitSoA &h, int64_t n, double thr, int64_t *end_key, uint8_t *state, hipStream_t s) {
  return launch_1d(k_filter_init, n, kBlock, 0, s, h, n, thr, end_key, state);
}
hipError_t launch_filter_round(const HitSoA &h, int64_t n, const int64_t *pmax, uint8_t *state, int32_t *pending, bool tiles,
                               hipStream_t s) {
  return launch_1d(tiles ? k_filter_round_tile : k_filter_round, n, kBlock, 0, s, h, n, pmax, state, pending);
}
hipError_t launch_filter_final(const HitSoA &h, int64_t n, const int64_t *pmax, const uint8_t *state, uint8_t *keep, bool tiles,
                               hipStream_t s) {
  return launch_1d(tiles ? k_filter_final_tile : k_filter_final, n, kBlock, 0, s, h, n, pmax, state, keep);
}

} // namespace prb
