// Raccess, the last step and the whole launch: k_access <-> CalcAccessibility + Exterior/Hairpin/Multi probabilities,
// raccess.cpp:484-612; k_fill; ra_launch, which enqueues the passes of all four files (mapping: raccess_common.hpp).
#include "raccess_common.hpp"

namespace prb {

namespace {

__global__ void k_fill(double *p, int64_t n, double value) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = value;
}

// ---------------------------------------------------------------------- accessibility
// One lane per window start x (raccess.cpp:510-527); hairpin (:536-579), multi (:581-612)
// and exterior (:530-534) probabilities are gathers that are independent per x.
__device__ __forceinline__ double multi_prob(const RaLds &lds, const SeqView &v, int x, int w) {
  const int L = v.L, W = v.W, S = v.S;
  const double *a_multi = v.tab(A_MULTI), *a_multi2 = v.tab(A_MULTI2);
  const double *b_multi = v.tab(B_MULTI), *b_multi2 = v.tab(B_MULTI2);
  double temp = 0;
  bool flag = false;
  for (int i = x + w - 1; i <= imin(x + W, L); i++) {
    const double bb = EM(b_multi, x - 1, i), aa = EM(a_multi, x + w - 1, i);
    if (bb != kNegInf && aa != kNegInf) {
      temp = flag ? ra_lse(lds, temp, bb + aa) : bb + aa;
      flag = true;
    }
  }
  for (int i = imax(0, x + w - 1 - W); i < x; i++) {
    const double bb = EM(b_multi2, i, x + w - 1), aa = EM(a_multi2, i, x - 1);
    if (bb != kNegInf && aa != kNegInf) {
      temp = flag ? ra_lse(lds, temp, bb + aa) : bb + aa;
      flag = true;
    }
  }
  return flag ? ra_expd(lds, temp - v.v(V_AO)[L]) : 0.0;
}

// (a thread per window start: blockIdx.y = the sequence, blockIdx.x = its chunk of kBlock positions)
__global__ __launch_bounds__(kBlock) void k_access(RaBatch b, RaConst c) {
  __shared__ RaLds lds;
  const int idx = blockIdx.y;
  if (1 + (int)(blockIdx.x * kBlock) > b.desc[idx].L) return; // (the whole workgroup: before the barrier of the table load)
  ra_load_lds(lds, c);
  using SL = RaSmallLayout;
  const SeqView v = make_view(b, idx);
  const int L = v.L, W = v.W, S = v.S, delta = b.delta;
  const unsigned char *s = v.s;
  const double *b_stemend = v.tab(B_STEMEND);
  const double *ao = v.v(V_AO), *bo = v.v(V_BO);
  const double *bpv = v.v(V_BP), *cbpv = v.v(V_CBP), *bfl = v.v(V_BFLAG), *cfl = v.v(V_CFLAG);
  const double Z = ao[L];
  const double kT = lds.small[SL::kKT];
  const bool logsum = !(Z >= -690 && Z <= 690);
  float *acc = b.acc + v.out_off, *cond = b.cond + v.out_off;

  for (int x = 1 + (int)(blockIdx.x * kBlock + threadIdx.x); x <= L; x += L) { // (one position per thread)
    float acc_x = 0.0f;
    const bool has_acc = x + delta - 1 <= L;
    if (has_acc) {
      // hairpin loops enclosing [x, x+delta-1] (:536-579)
      double temp = 0, c_temp = 0;
      bool flag = false, c_flag = false;
      for (int i = imax(1, x - W); i < x; i++) {
        for (int j = x + delta; j <= imin(i + W, L); j++) {
          const double se = EM(b_stemend, i, j - 1);
          if (se != kNegInf) {
            const int type = ra_bp(lds, s[i], s[j]);
            const double h = se + ra_hairpin_energy(lds, type, j - i - 1, s[i + 1], s[j - 1]);
            if (j == x + delta) {
              temp = flag ? ra_lse(lds, temp, h) : h;
              flag = true;
            } else {
              c_temp = c_flag ? ra_lse(lds, c_temp, h) : h;
              c_flag = true;
            }
          }
        }
      }
      if (flag && c_flag) temp = ra_lse(lds, temp, c_temp);
      if (!flag && c_flag) {
        temp = c_temp;
        flag = true;
      }
      const double hp = flag ? ra_expd(lds, temp - Z) : 0.0;
      const double chp = c_flag ? ra_expd(lds, c_temp - Z) : 0.0;

      // bulge / interior loop terms: finalisation of the scatter sums (:667-680 / :754-770)
      double bl = bpv[x - 1], cbl = cbpv[x - 1];
      if (!logsum) {
        if (bl != 0) bl = ra_expd(lds, (double)ra_logf(lds, (float)(bl + cbl)) - Z);
        if (cbl != 0) cbl = ra_expd(lds, (double)ra_logf(lds, (float)cbl) - Z);
      } else {
        const bool f1 = bfl[x - 1] != 0, f2 = cfl[x - 1] != 0;
        if (f1 && f2) bl = ra_lse(lds, bl, cbl);
        if (!f1 && f2) bl = cbl;
        if (f1) bl = ra_expd(lds, bl - Z);
        if (f2) cbl = ra_expd(lds, cbl - Z);
      }

      double prob = 0.0;
      prob += ra_expd(lds, ao[x - 1] + bo[x + delta - 1] - Z);
      prob += hp;
      prob += bl;
      prob += multi_prob(lds, v, x, delta);
      acc_x = (float)(((double)(-ra_logf(lds, (float)prob)) * kT) / 1000);
      acc[x - 1] = acc_x;

      if (x + delta - 1 < L) {
        double cp = 0.0;
        cp += ra_expd(lds, ao[x - 1] + bo[x + delta] - Z);
        cp += chp;
        cp += cbl;
        cp += multi_prob(lds, v, x, delta + 1);
        cond[x + delta - 1] = (float)(((double)(-ra_logf(lds, (float)cp)) * kT) / 1000 - (double)acc_x);
      }
    }
  }
}

} // namespace

#ifdef PRB_GAP_PROFILE
// (the counters of the files that count: the slots of k_inside, 1 - 4, and of k_outside, 8 - 12, do not overlap)
extern "C" int prb_debug_ra_profile(unsigned long long *out, int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  for (int k = 0; k < 32; k++) out[k] = 0;
  return ra_inside_profile(out, reset) || ra_outside_profile(out, reset) ? -1 : 0;
}
#endif

hipError_t ra_launch(const RaBatch &b, const RaConst &c, int64_t band_elems, int64_t vec_elems,
                     hipStream_t stream) {
  if (b.nseq <= 0) return hipSuccess;
  const int fill_blocks = 2048;
  hipLaunchKernelGGL(k_fill, dim3(fill_blocks), dim3(256), 0, stream, b.band, band_elems, kNegInf);
  hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, stream, b.vec, vec_elems, 0.0);
  ra_launch_inside(b, c, stream);
  ra_launch_outside(b, c, stream);
  ra_launch_biloop(b, c, stream);
  hipLaunchKernelGGL(k_access, dim3((b.lmax + kBlock - 1) / kBlock, b.nseq), dim3(kBlock), 0, stream, b, c);
  return hipGetLastError();
}

} // namespace prb
