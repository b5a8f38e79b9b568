// Sort keys, gathers and flags on gfx950: everything around the radix sorts (rocPRIM, on the host side) that put a hit
// list into the reference's order, and the small list utilities of the driver.
//
//   k_make_keys, k_make_packed_keys* <-> compare()  rna_interaction_search.cpp:45-55, made total by the hits' own
//                                        fields (k_fix_ties; DESIGN.md "total order")
//   k_flag_not_above                 <-> the threshold half of CheckRedundancy  rna_interaction_search.cpp:387-424
//   k_pack_hits                      ->  the C ABI's prb_hit records (include/priblast_hip.h)
#include "../../include/priblast_hip.h"

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// Monotone map of a double onto unsigned integers, for the energies of the sort keys.  -0.0 maps as +0.0: the
// comparator these keys restate compares with != and <, for which the zeros are equal, so the next field decides
// between them (the hits keep their energies as they are; only the keys are made alike).
__device__ __forceinline__ uint64_t order_bits(double v) {
  const uint64_t b = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(kBlock) void k_make_keys(HitSoA h, int64_t n, uint64_t *k_energy, uint32_t *k_len,
                                                      uint32_t *k_qsp, uint64_t *k_pos, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  // compare(): db_sp asc, q_sp asc, db_len desc, q_len desc (rna_interaction_search.cpp:45-55);
  // ties are then broken by energy asc, its two parts and input order (DESIGN.md "total order")
  k_energy[i] = order_bits(h.e_tot[i]);
  k_len[i] = ((uint32_t)(0xFFFF - US(h.db_len[i])) << 16) | (uint32_t)(0xFFFF - US(h.q_len[i]));
  k_qsp[i] = (uint32_t)h.q_sp[i];
  k_pos[i] = ((uint64_t)(uint32_t)h.query[i] << 32) | (uint32_t)h.db_sp[i];
  idx[i] = (uint32_t)i;
}

// The same order from ONE 64-bit key when the fields are narrow enough (they are for every page
// of up to 2^27 characters and sequences of up to a few thousand nucleotides): query (relative to
// the sub-batch) | db_sp | q_sp | lmax - db_len | lmax - q_len.  A single stable radix sort over
// the used bits then leaves only the hits with identical coordinates to be put in (energy, input
// order) order, which k_fix_ties does run by run.
__global__ __launch_bounds__(kBlock) void k_make_packed_keys(HitSoA h, int64_t n, PackedKeyInfo f, uint64_t *key,
                                                             uint64_t *k_energy, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  k_energy[i] = order_bits(h.e_tot[i]);
  uint64_t k = (uint64_t)(uint32_t)(h.query[i] - f.qmin);
  k = (k << f.bd) | (uint32_t)h.db_sp[i];
  k = (k << f.bq) | (uint32_t)h.q_sp[i];
  k = (k << f.bl) | (uint32_t)(f.lmax - US(h.db_len[i]));
  k = (k << f.bl) | (uint32_t)(f.lmax - US(h.q_len[i]));
  key[i] = k;
  idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_make_packed_keys_recs(const HitRec *__restrict__ h, int64_t n, PackedKeyInfo f,
                                                                  uint64_t *key, uint64_t *k_energy, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const HitRec r = h[i];
  k_energy[i] = order_bits(r.e_tot);
  uint64_t k = (uint64_t)(uint32_t)(r.query - f.qmin);
  k = (k << f.bd) | (uint32_t)r.db_sp;
  k = (k << f.bq) | (uint32_t)r.q_sp;
  k = (k << f.bl) | (uint32_t)(f.lmax - US(r.db_len));
  if (!f.one_len) k = (k << f.bl) | (uint32_t)(f.lmax - US(r.q_len)); // (one_len: q_len = db_len in every hit of the list)
  key[i] = k;
  idx[i] = (uint32_t)i;
}

constexpr int kMaxTieRun = 4096;
// Runs of identical coordinates are put in (energy, hybridization part, accessibility part, input index) order: two
// hits still tied after the three energies are identical records, so the result does not depend on the order in which
// the seeds were produced (chunks of candidates, pairs sorted by database position).  Every element of a run finds its
// own rank among the others (a run is several seeds of one duplex extended to the same hit: a few elements, the same
// total energy more often than not, so most comparisons go on to the records) - independent loads, where one thread
// per run sorting by insertion was a chain of dependent ones (2.1 ms per 2.5e7 hits; this: 1.6 ms).
__global__ __launch_bounds__(kBlock) void k_fix_ties(const uint64_t *__restrict__ key, const uint64_t *__restrict__ e,
                                                     const uint32_t *__restrict__ perm, int64_t n, const HitRec *__restrict__ recs,
                                                     uint32_t *__restrict__ perm_out, int32_t *too_long) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  const uint32_t pi = perm[i];
  const bool left = i > 0 && key[i - 1] == k, right = i + 1 < n && key[i + 1] == k;
  if (!left && !right) {
    perm_out[i] = pi;
    return;
  }
  int64_t s = i, t = i + 1;
  while (s > 0 && key[s - 1] == k && i - s <= kMaxTieRun) s--;
  while (t < n && key[t] == k && t - s <= kMaxTieRun) t++;
  if (t - s > kMaxTieRun) {
    *too_long = 1;
    perm_out[i] = pi;
    return;
  }
  const uint64_t ei = e[i];
  const uint64_t hi = order_bits(recs[pi].e_hyb), ai = order_bits(recs[pi].e_acc);
  int rank = 0;
  for (int64_t b = s; b < t; b++) {
    if (b == i) continue;
    const uint64_t eb = e[b];
    bool before = eb < ei; // element b sorts before this one
    if (eb == ei) {
      const uint32_t pb = perm[b];
      const uint64_t hb = order_bits(recs[pb].e_hyb);
      if (hb != hi) {
        before = hb < hi;
      } else {
        const uint64_t ab = order_bits(recs[pb].e_acc);
        before = ab != ai ? ab < ai : pb < pi;
      }
    }
    rank += before ? 1 : 0;
  }
  perm_out[s + rank] = pi;
}

__global__ __launch_bounds__(kBlock) void k_order_keys(const double *__restrict__ v, int64_t n, uint64_t *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) key[i] = order_bits(v[i]);
}

template <class T> __global__ __launch_bounds__(kBlock) void k_gather(const T *src, const uint32_t *idx, T *dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

__global__ __launch_bounds__(kBlock) void k_gather_hits(HitSoA s, const uint32_t *idx, HitSoA d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx[i];
  d.q_sp[i] = s.q_sp[j];
  d.db_sp[i] = s.db_sp[j];
  d.q_len[i] = s.q_len[j];
  d.db_len[i] = s.db_len[j];
  d.db_id[i] = s.db_id[j];
  d.db_id_start[i] = s.db_id_start[j];
  d.query[i] = s.query[j];
  d.e_acc[i] = s.e_acc[j];
  d.e_hyb[i] = s.e_hyb[j];
  d.e_tot[i] = s.e_tot[j];
}

__global__ __launch_bounds__(kBlock) void k_gather_hits_to_recs(HitSoA s, const uint32_t *idx, HitRec *d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx[i];
  HitRec r;
  r.q_sp = s.q_sp[j];
  r.db_sp = s.db_sp[j];
  r.q_len = s.q_len[j];
  r.db_len = s.db_len[j];
  r.db_id = s.db_id[j];
  r.db_id_start = s.db_id_start[j];
  r.query = s.query[j];
  r.pad0 = 0;
  r.e_acc = s.e_acc[j];
  r.e_hyb = s.e_hyb[j];
  r.e_tot = s.e_tot[j];
  r.pad1 = 0;
  d[i] = r;
}
__global__ __launch_bounds__(kBlock) void k_gather_recs_to_hits(const HitRec *__restrict__ s, const uint32_t *idx, HitSoA d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const HitRec r = s[idx ? (int64_t)idx[i] : i];
  d.q_sp[i] = r.q_sp;
  d.db_sp[i] = r.db_sp;
  d.q_len[i] = r.q_len;
  d.db_len[i] = r.db_len;
  d.db_id[i] = r.db_id;
  d.db_id_start[i] = r.db_id_start;
  d.query[i] = r.query;
  d.e_acc[i] = r.e_acc;
  d.e_hyb[i] = r.e_hyb;
  d.e_tot[i] = r.e_tot;
}

// SoA hits -> the C ABI's records (include/priblast_hip.h), so that one copy brings them to the host.
// bp_base >= 0: the records also get their range in the hit set's base-pair array: hit i has
// bp_count[i] pairs from pair index bp_base + bp_off[i] on (no arrays: the two end pairs, 2 per hit).
__global__ __launch_bounds__(kBlock) void k_pack_hits(HitSoA s, int64_t n, const int32_t *__restrict__ bp_count,
                                                      const int64_t *__restrict__ bp_off, int64_t bp_base, prb_hit *out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  prb_hit h;
  h.q_sp = s.q_sp[i];
  h.db_sp = s.db_sp[i];
  h.q_len = s.q_len[i];
  h.db_len = s.db_len[i];
  h.db_id = s.db_id[i];
  h.db_id_start = s.db_id_start[i];
  h.e_acc = s.e_acc[i];
  h.e_hyb = s.e_hyb[i];
  h.e_tot = s.e_tot[i];
  h.query = s.query[i];
  h.bp_count = bp_base < 0 ? 0 : bp_count ? bp_count[i] : 2;
  h.bp_offset = bp_base < 0 ? 0 : bp_base + (bp_off ? bp_off[i] : 2 * i);
  out[i] = h;
}

// keep[i] = 1 unless E_i > threshold.  A hit above the threshold is flagged by CheckRedundancy
// the moment the sweep reaches it and never flags anything else (as the contained hit of an
// earlier scan it loses: E_a <= threshold < E_b), so it can be dropped BEFORE the sort.
__global__ __launch_bounds__(kBlock) void k_flag_not_above(const double *e_tot, int64_t n, double thr, uint8_t *keep) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) keep[i] = !(e_tot[i] > thr);
}

// first[i] = 1 for the first hit of every query in a (query-sorted) list
__global__ __launch_bounds__(kBlock) void k_mark_first(const int32_t *query, int64_t n, uint8_t *first) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) first[i] = i == 0 || query[i] != query[i - 1];
}

__global__ __launch_bounds__(256) void k_iota_u32(uint32_t *dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (uint32_t)i;
}
// dst row r = src row idx[r]; rows of `words` 16-byte words, one thread per word
__global__ __launch_bounds__(256) void k_gather_rows(const uint4 *__restrict__ src, const uint32_t *__restrict__ idx, uint4 *dst, int64_t n,
                                                     int words) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = t / words;
  if (r >= n) return;
  const int wi = (int)(t - r * words);
  dst[r * words + wi] = src[(int64_t)idx[r] * words + wi];
}
__global__ __launch_bounds__(256) void k_flag_marked(const uint8_t *__restrict__ marks, const uint32_t *__restrict__ list, int64_t n, uint8_t mask,
                                                     uint8_t *flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = (marks[list[i]] & mask) ? 1 : 0;
}

} // namespace

hipError_t launch_make_keys(const HitSoA &hits, int64_t n, uint64_t *k_energy, uint32_t *k_len, uint32_t *k_qsp,
                            uint64_t *k_pos, uint32_t *idx, hipStream_t s) {
  return launch_1d(k_make_keys, n, kBlock, 0, s, hits, n, k_energy, k_len, k_qsp, k_pos, idx);
}
hipError_t launch_make_packed_keys(const HitSoA &hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                   uint32_t *idx, hipStream_t s) {
  return launch_1d(k_make_packed_keys, n, kBlock, 0, s, hits, n, f, key, k_energy, idx);
}
hipError_t launch_make_packed_keys_recs(const HitRec *hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                        uint32_t *idx, hipStream_t s) {
  return launch_1d(k_make_packed_keys_recs, n, kBlock, 0, s, hits, n, f, key, k_energy, idx);
}
hipError_t launch_fix_ties(const uint64_t *key_sorted, const uint64_t *e_sorted, const uint32_t *perm, int64_t n, const HitRec *recs,
                           uint32_t *perm_out, int32_t *too_long, hipStream_t s) {
  return launch_1d(k_fix_ties, n, kBlock, 0, s, key_sorted, e_sorted, perm, n, recs, perm_out, too_long);
}
hipError_t launch_order_keys(const double *v, int64_t n, uint64_t *key, hipStream_t s) {
  return launch_1d(k_order_keys, n, kBlock, 0, s, v, n, key);
}
hipError_t launch_gather_u64(const uint64_t *src, const uint32_t *idx, uint64_t *dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather<uint64_t>, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_u32(const uint32_t *src, const uint32_t *idx, uint32_t *dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather<uint32_t>, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_u8(const uint8_t *src, const uint32_t *idx, uint8_t *dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather<uint8_t>, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_hits(const HitSoA &src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather_hits, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_hits_to_recs(const HitSoA &src, const uint32_t *idx, HitRec *dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather_hits_to_recs, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_recs_to_hits(const HitRec *src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s) {
  return launch_1d(k_gather_recs_to_hits, n, kBlock, 0, s, src, idx, dst, n);
}
hipError_t launch_gather_rows(const void *src, const uint32_t *idx, void *dst, int64_t n, int row_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (row_bytes % 16 != 0) return hipErrorInvalidValue;
  const int words = row_bytes / 16;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n * words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, static_cast<const uint4 *>(src),
                     idx, static_cast<uint4 *>(dst), n, words);
  return hipGetLastError();
}
hipError_t launch_iota_u32(uint32_t *dst, int64_t n, hipStream_t s) { return launch_1d(k_iota_u32, n, kBlock, 0, s, dst, n); }
hipError_t launch_flag_marked(const uint8_t *marks, const uint32_t *list, int64_t n, uint8_t mask, uint8_t *flags, hipStream_t s) {
  return launch_1d(k_flag_marked, n, kBlock, 0, s, marks, list, n, mask, flags);
}
hipError_t launch_flag_not_above(const double *e_tot, int64_t n, double thr, uint8_t *keep, hipStream_t s) {
  return launch_1d(k_flag_not_above, n, kBlock, 0, s, e_tot, n, thr, keep);
}
hipError_t launch_mark_first(const int32_t *query, int64_t n, uint8_t *first, hipStream_t s) {
  return launch_1d(k_mark_first, n, kBlock, 0, s, query, n, first);
}
hipError_t launch_pack_hits(const HitSoA &src, int64_t n, const int32_t *bp_count, const int64_t *bp_off, int64_t bp_base,
                            void *out, hipStream_t s) {
  return launch_1d(k_pack_hits, n, kBlock, 0, s, src, n, bp_count, bp_off, bp_base, static_cast<prb_hit *>(out));
}

} // namespace prb
