// Raccess on gfx950: windowed McCaskill inside/outside and the accessibility of every
// length-delta window (what Raccess::Run(seq, acc, cond) computes, raccess.cpp:42-50).
//
// Mapping (DESIGN.md "Raccess kernels"): one 64-lane wavefront owns one sequence and walks
// the DP column by column (column = end position); the <= W-1 cells of a column sit on the
// lanes (64 per pass).  A column is processed as phases that are parallel over cells, in
// the dependency order derived in SURVEY.md 8(a'); every sum is folded in the reference's
// order by the lane that owns the cell (bit-exact), and the (u1,u2) interior-loop
// enumeration is wave-uniform so the loop-energy branch never diverges.  Band tables live in
// HBM in END-MAJOR layout T[end][span], so the lanes of a column read and write contiguous
// doubles; the exp/log tables and the small Turner tables are staged in LDS once per
// workgroup (4 waves = 4 sequences share one image).
//
//   raccess_inside.hip   k_inside   <-> Raccess::CalcInsideVariable   raccess.cpp:99-242
//   raccess_outside.hip  k_outside  <-> Raccess::CalcOutsideVariable  raccess.cpp:258-412
//   raccess_biloop.hip   k_biloop   <-> CalcBulgeAndInternalProbability / CalcLogSum...  raccess.cpp:614-771
//   raccess_access.hip   k_access   <-> CalcAccessibility + Exterior/Hairpin/Multi probabilities  raccess.cpp:484-612
//
// This header is what those files share on the device: the workspace layout, the row masks of the two big folds, values
// kept on the lanes of a wavefront, and the LDS hand-over between the wavefronts of a workgroup (kH = 3).  Everything is in
// an anonymous namespace, so each file has its own copy of the developer counters below; the files are linked without
// relocatable device code and reach each other only through the host launchers of raccess_kernels.hpp.
#pragma once
#include "raccess_kernels.hpp"

#include "raccess_device.hpp"

namespace prb {

namespace {

// Developer-only cycle breakdown per phase (make prof; tools/raccess_profile.py): wave-cycles of the first
// wavefront of a launch, accumulated by lane 0 at every phase boundary.  Not part of the product build.
#ifdef PRB_GAP_PROFILE
__device__ unsigned long long g_ra_prof[32];
#define RA_COUNT(k, v)            \
  do {                            \
    if (ra_p_) g_ra_prof[k] += (v); \
  } while (0)
#define RA_PROF_DECL unsigned long long ra_t0_ = __builtin_amdgcn_s_memtime(); const bool ra_p_ = blockIdx.x == 0 && threadIdx.x == 0
#define RA_PROF(k)                                                  \
  do {                                                              \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();     \
    if (ra_p_) g_ra_prof[k] += t_ - ra_t0_;                         \
    ra_t0_ = t_;                                                    \
  } while (0)
#else
#define RA_PROF_DECL
#define RA_PROF(k)
#define RA_COUNT(k, v)
#endif

constexpr int kWave = 64;
#ifndef PRB_RA_AHEAD // (throughput-mode experiments: terms fetched ahead, wavefronts per workgroup, wavefronts per SIMD asked of the compiler)
#define PRB_RA_AHEAD 8
#define PRB_RA_WPB 4
#define PRB_RA_WPS 3
#endif
constexpr int kRaAhead = PRB_RA_AHEAD; // interior-loop terms fetched ahead of the fold in k_inside / k_outside
constexpr int kHB = 8;      // ... per batch when helper wavefronts prepare them (a barrier per batch: fewer, longer rounds)
constexpr int kWavesPerBlock = PRB_RA_WPB;
constexpr int kBlock = kWave * kWavesPerBlock;

// band table ids inside one sequence's workspace block
enum : int {
  A_STEM = 0, A_STEMEND, A_MULTI, A_MULTIBIF, A_MULTI1, A_MULTI2, A_MULTI1_T,
  B_STEM, B_STEMEND, B_MULTI, B_MULTIBIF, B_MULTI1, B_MULTI2
};
static_assert(B_MULTI2 + 1 == kRaBands, "band count");
enum : int { V_AO = 0, V_BO, V_BP, V_CBP, V_BFLAG, V_CFLAG };

struct SeqView {
  int L, W, S;  // S = W + 2 = row length of a band
  int64_t rows; // L + 2
  double *band;
  double *vec;
  const unsigned char *s; // codes 0..4: s[0] = 0, s[1..L], s[L+1] = 0
  int64_t out_off;
  __device__ __forceinline__ double *tab(int t) const { return band + (int64_t)t * rows * S; }
  __device__ __forceinline__ double *v(int t) const { return vec + (int64_t)t * rows; }
};

__device__ __forceinline__ SeqView make_view(const RaBatch &b, int idx) {
  const RaSeqDesc d = b.desc[idx];
  SeqView v;
  v.L = d.L;
  v.W = b.W;
  v.S = b.W + 2;
  v.rows = (int64_t)d.L + 2;
  v.band = b.band + d.band_off;
  v.vec = b.vec + d.vec_off;
  v.s = b.codes + d.code_off;
  v.out_off = d.out_off;
  return v;
}

// element (start, end) of an end-major band: row `end`, column `end - start`
#define EM(tab, start, end) ((tab)[(int64_t)(end) * S + ((end) - (start))])
// start-major copy (alpha_multi1 only): row `start`, column `end - start`
#define SM(tab, start, end) ((tab)[(int64_t)(start) * S + ((end) - (start))])

// Orders this wave's global stores before its later loads issued by other lanes.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Raccess::CalcDangleEnergy, raccess.cpp:244-256
__device__ __forceinline__ double dangle_energy(const RaLds &lds, const SeqView &v, int type, int a, int b) {
  using SL = RaSmallLayout;
  double x = 0;
  if (type != 0) {
    if (a > 0) x += lds.small[SL::kDangle5 + type * 5 + v.s[a]];
    if (b < v.L) x += lds.small[SL::kDangle3 + type * 5 + v.s[b + 1]];
    if (b == v.L && type > 2) x += lds.small[SL::kTermAU];
  }
  return x;
}

// Which cells of a band table hold a value: one 128-bit mask per START position (bit = span), kept in LDS for
// the last 128 starts.  The two big folds (Alpha_stemend over the enclosed stems, Beta_stem over the enclosing
// pairs) walk their <= 496 (u1, u2) terms in the reference's order; only the terms whose table entry is not
// -INF take part (about one in three for the cells that fold at all), and a lane finds them as the set bits of a
// window of the row masks instead of testing every term.
struct RowMasks {
  uint32_t m[128][5]; // 128 bits + a zero word, so that a 32-bit window may start in the last word
};
__device__ __forceinline__ void rowmask_clear(RowMasks &r, int start) {
#pragma unroll
  for (int k = 0; k < 5; k++) r.m[start & 127][k] = 0;
}
__device__ __forceinline__ void rowmask_set(RowMasks &r, int start, int span) { r.m[start & 127][span >> 5] |= 1u << (span & 31); }
// bits [lo, hi] of row `start` as a 32-bit word, bit 0 = span lo (0 <= lo <= 127, hi - lo <= 31; 0 if hi < lo)
__device__ __forceinline__ uint32_t rowmask_window(const RowMasks &r, int start, int lo, int hi) {
  if (hi < lo) return 0;
  const uint32_t *row = r.m[start & 127];
  const int k = lo >> 5;
  const uint32_t a = row[k], b = row[k + 1];
  const uint32_t w = __builtin_amdgcn_alignbit(b, a, (uint32_t)(lo & 31)); // (b:a) >> (lo & 31)
  const int width = hi - lo + 1;
  return width >= 32 ? w : (w & ((1u << width) - 1));
}

// lane `l` (wave-uniform) of a double, whatever the execution mask: two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
// Per-cell values kept in registers across the phases of a column: one double per pass over the cells (NP passes of
// 64 lanes; NP = 2 covers maximal spans up to 127, NP = 4 up to 255).  `pass` / the index are wave-uniform.
template <int NP>
__device__ __forceinline__ void reg_set(double (&reg)[NP], int pass, double v) {
#pragma unroll
  for (int k = 0; k < NP; k++)
    if (pass == k) reg[k] = v;
}
// element idx (0 .. 64 * NP - 1) of values laid out one per lane, pass after pass
template <int NP>
__device__ __forceinline__ double lane_value_asc(const double (&reg)[NP], int idx) {
  double r = readlane_f64(reg[0], idx & 63);
#pragma unroll
  for (int k = 1; k < NP; k++)
    if ((idx >> 6) == k) r = readlane_f64(reg[k], idx & 63);
  return r;
}
// the value the lane that owns cell `d` holds, for cells laid out d = dtop - lane (dtop = dmax, dmax - 64, ...)
template <int NP>
__device__ __forceinline__ double cell_value_desc(const double (&reg)[NP], int dmax, int d) {
  return lane_value_asc<NP>(reg, dmax - d);
}

// ---- kH = 3 (see k_inside): the wavefronts of a sequence's workgroup hand batches of terms to each other through LDS
// counters instead of workgroup barriers, so that the sequence's own wavefront is free to run its chains meanwhile.
// All wavefronts of a workgroup are resident together, so waiting on one another cannot deadlock; a wait that does not
// end (a bug) trips a watchdog: the wavefront raises the workgroup's abort flag and the launch's flag (RaBatch::watchdog) and ENDS - a barrier
// does not wait for ended wavefronts -, the others follow at their next wait, the host reports PRB_ERR_STATE.
struct FoldSync {
  int prod[2]; // batches helper 1 / helper 2 have written (running count over the whole sequence)
  int cons;    // batches the folding wavefront has taken
  int abort;
};
// false: give up (the caller returns from the kernel)
__device__ __forceinline__ bool fold_wait(FoldSync &fs, int &counter, int target, int *watchdog) {
  for (int n = 0;; n++) {
    if (__hip_atomic_load(&counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) return true;
    if (__hip_atomic_load(&fs.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0 || n > (1 << 21)) {
      __hip_atomic_store(&fs.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      *watchdog = 1;
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void fold_post(int &counter, int value, int lane) {
  // (the LDS operations of a wavefront complete in order: the batch written by all its lanes is there before the count)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0) __hip_atomic_store(&counter, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// ---- host side: what the launchers of the files share
// The form of the inside / outside passes a batch takes: passes over a column's cells (two of 64 lanes up to a maximal span
// of 127 - the default is 70 -, four up to kRaMaxSpan) and helper wavefronts.  Few sequences (a batch of queries): a
// workgroup per sequence, helper wavefronts for the big folds - the time is one wavefront's chain, the GPU otherwise idle.
// Many (a database): a wavefront per sequence, as many side by side as fit.  Helpers need the row masks.
struct RaForm {
  int np, helpers;
};
inline RaForm ra_form(const RaBatch &b) {
  if (b.W + 1 > 128) return {4, 0};
  const bool masks = b.W + 2 + kMaxLoop <= 128;
  return {2, masks && b.helpers >= 1 && b.helpers <= 3 ? b.helpers : 0};
}
template <typename K>
inline void ra_launch_form(K kernel, int helpers, const RaBatch &b, const RaConst &c, hipStream_t stream) {
  if (helpers) hipLaunchKernelGGL(kernel, dim3(b.nseq), dim3(kWave * (1 + helpers)), 0, stream, b, c);
  else hipLaunchKernelGGL(kernel, dim3((b.nseq + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, stream, b, c);
}

#ifdef PRB_GAP_PROFILE
// adds this file's counters to out[32] (the device is idle)
inline int ra_profile_add(unsigned long long *out, int reset) {
  unsigned long long mine[32];
  if (hipMemcpyFromSymbol(mine, HIP_SYMBOL(g_ra_prof), sizeof(mine)) != hipSuccess) return -1;
  for (int k = 0; k < 32; k++) out[k] += mine[k];
  if (reset) {
    const unsigned long long z[32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ra_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

} // namespace

} // namespace prb
