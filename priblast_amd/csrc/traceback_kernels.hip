// Traceback on gfx950: the base pairs of the final hits, from what the gapped extension (gapped_lds.hip) left behind.
//
//   k_bp_count, k_bp_expand <-> GetBasePair and the traced pairs of the two extensions
//                                                                  rna_interaction_search.cpp:371-385
//   k_bp_ends               <-> the first and last pair of the simplified output  rna_interaction_search.cpp:355-363
//
// (k_bp_count alone has internal linkage: profiles and traces know the kernels by their symbol names, which a move
// into or out of the anonymous namespace would change.)
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

// total base pairs of list entry w = complementary positions of the ungapped diagonal
// (GetBasePair, rna_interaction_search.cpp:371-385) + the pairs traced by the two extensions
__global__ __launch_bounds__(256) void k_bp_count(HitSoA in, int64_t n, const uint32_t *__restrict__ subset, QBatchDev qb,
                                                  PageDev pg, SearchConst sc, const int32_t *__restrict__ ntrace,
                                                  int32_t *bp_count) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int64_t x = subset ? (int64_t)subset[w] : w;
  const uint8_t *qs = qb.enc + qb.off[in.query[x]] + in.q_sp[x];
  const uint8_t *ds = pg.seqs + in.db_sp[x];
  const int len = US(in.q_len[x]);
  int c = 0;
  for (int t = 0; t < len; t++) c += diag_pairs(sc, qs[t], ds[t]);
  bp_count[w] = c + (ntrace[x] & 0xFFFF) + (int)((uint32_t)ntrace[x] >> 16);
}

} // namespace

// slot[list[p]] = base + p
__global__ __launch_bounds__(256) void k_assign_slots(const uint32_t *__restrict__ list, int64_t n, int32_t base, int32_t *slot) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) slot[list[p]] = base + (int32_t)p;
}

// Base pairs of final hit w from the trace slot its extension pass left (same layout as mode 2
// of the gapped kernels writes).  Hits completed by the wave kernel (tier 3) or with a chain
// longer than the slot are left to the mode-2 pass.
__global__ __launch_bounds__(256) void k_bp_expand(HitSoA in, int64_t n, const uint32_t *__restrict__ subset, QBatchDev qb,
                                                   PageDev pg, SearchConst sc, const uint8_t *__restrict__ first_flag,
                                                   const int32_t *__restrict__ ntrace, const uint8_t *__restrict__ tier_of,
                                                   const uint16_t *__restrict__ trace, LongTrace lt, const int64_t *__restrict__ bp_off,
                                                   int32_t *bp_out) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int64_t x = subset[w];
  const int nleft = ntrace[x] & 0xFFFF, nright = (int)((uint32_t)ntrace[x] >> 16);
  // a hit of the wavefront-per-hit kernel with its chains on record (kLongTraceTier): the second direction from its long
  // trace, the first one from there too unless an LDS tier ran it (then from that tier's trace slot)
  const int ls = (tier_of[x] == kLongTraceTier && lt.slot) ? lt.slot[x] : -1;
  if (ls < 0 && (tier_of[x] >= kWaveTier || nleft > kTraceCap || nright > kTraceCap)) return;
  const uint32_t *lt_left = ls >= 0 && lt.count[ls * 2] >= 0 ? lt.trace + ((int64_t)ls * 2) * lt.cap : nullptr;
  const uint32_t *lt_right = ls >= 0 ? lt.trace + ((int64_t)ls * 2 + 1) * lt.cap : nullptr;
  const int q_sp = in.q_sp[x], db_sp = in.db_sp[x], len = US(in.q_len[x]);
  const uint8_t *qs = qb.enc + qb.off[in.query[x]] + q_sp;
  const uint8_t *ds = pg.seqs + db_sp;
  const bool unsorted = first_flag[x] != 0; // hit 0 of a query keeps the raw pair order
  const int64_t out0 = bp_off[w];
  int ndiag = 0;
  const int64_t d0 = unsorted ? out0 : out0 + nleft;
  for (int t = 0; t < len; t++)
    if (diag_pairs(sc, qs[t], ds[t])) {
      bp_out[2 * (d0 + ndiag)] = q_sp + t;
      bp_out[2 * (d0 + ndiag) + 1] = db_sp + t;
      ndiag++;
    }
  const uint16_t *sl = trace + x * 2 * kTraceCap;
  for (int t = 0; t < nleft; t++) {
    const int ci = lt_left ? (int)(lt_left[t] & 0xFFFF) : (sl[t] & 0xFF), cj = lt_left ? (int)(lt_left[t] >> 16) : (sl[t] >> 8);
    const int64_t pos = unsorted ? out0 + ndiag + t : out0 + t;
    bp_out[2 * pos] = q_sp - ci;
    bp_out[2 * pos + 1] = db_sp - cj;
  }
  const int q_end = q_sp + in.q_len[x] - 1, db_end = db_sp + in.db_len[x] - 1;
  for (int t = 0; t < nright; t++) {
    const int ci = lt_right ? (int)(lt_right[t] & 0xFFFF) : (sl[kTraceCap + t] & 0xFF),
              cj = lt_right ? (int)(lt_right[t] >> 16) : (sl[kTraceCap + t] >> 8);
    const int64_t pos = unsorted ? out0 + ndiag + nleft + t : out0 + nleft + ndiag + (nright - 1 - t);
    bp_out[2 * pos] = q_end + ci;
    bp_out[2 * pos + 1] = db_end + cj;
  }
}

// first and last pair of every list entry (all the simplified output prints,
// rna_interaction_search.cpp:355-363): ends[4w..4w+3] = (q0, db0, qN, dbN)
__global__ __launch_bounds__(256) void k_bp_ends(const int64_t *__restrict__ bp_off, int64_t n, const int32_t *__restrict__ bp,
                                                 int32_t *ends) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int64_t a = bp_off[w], b = bp_off[w + 1] - 1;
  ends[4 * w] = bp[2 * a];
  ends[4 * w + 1] = bp[2 * a + 1];
  ends[4 * w + 2] = bp[2 * b];
  ends[4 * w + 3] = bp[2 * b + 1];
}

hipError_t launch_bp_count(const HitSoA &in, int64_t n, const uint32_t *subset, const QBatchDev &qb, const PageDev &pg,
                           const SearchConst &sc, const int32_t *ntrace, int32_t *bp_count, hipStream_t s) {
  return launch_1d(k_bp_count, n, kBlock, 0, s, in, n, subset, qb, pg, sc, ntrace, bp_count);
}
hipError_t launch_assign_slots(const uint32_t *list, int64_t n, int32_t base, int32_t *slot, hipStream_t s) {
  return launch_1d(k_assign_slots, n, kBlock, 0, s, list, n, base, slot);
}
hipError_t launch_bp_expand(const HitSoA &in, int64_t n, const uint32_t *subset, const QBatchDev &qb, const PageDev &pg,
                            const SearchConst &sc, const uint8_t *first_flag, const int32_t *ntrace, const uint8_t *tier_of,
                            const uint16_t *trace, const LongTrace &lt, const int64_t *bp_off, int32_t *bp_out, hipStream_t s) {
  return launch_1d(k_bp_expand, n, kBlock, 0, s, in, n, subset, qb, pg, sc, first_flag, ntrace, tier_of, trace, lt, bp_off, bp_out);
}
hipError_t launch_bp_ends(const int64_t *bp_off, int64_t n, const int32_t *bp, int32_t *ends, hipStream_t s) {
  return launch_1d(k_bp_ends, n, kBlock, 0, s, bp_off, n, bp, ends);
}

} // namespace prb
