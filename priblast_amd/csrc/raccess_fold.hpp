// The pieces of the two big folds of Raccess - Alpha_stemend over the enclosed stems (k_inside, phase 4) and Beta_stem over
// the enclosing pairs (k_outside, phase E) - that the forms of the kernels share.  A lane owns a cell and folds the cell's
// interior-loop terms in the reference's order, a batch of N = 8 at a time:
//   a term iterator   which terms: the set bits of a window of the row masks, as (su1[t], sspan[t]); su1 < 0: no term
//   a term evaluator  the values of terms [T0, T1) of a batch: all fetches first, then all look-ups, each value to a sink
//   fold_batch        the chain of N dependent logsumexp
//   the closing term  what ends the cell's sum, and the per-cell prologue that starts it
// The helper forms of the kernels are built from these; what is left in their bodies is who does which and how a batch is
// handed over: helpers and a workgroup barrier per batch (kH = 1, 2), helpers, a folding wavefront and LDS counters
// (kH = 3).  The prologue and the closing term are their own functions so that every form can share them.  The throughput
// form (kH = 0, one wavefront one batch behind itself) and the form without row masks keep their own text in the kernels:
// built from these pieces the compiler gives kH = 0 more registers than three wavefronts per SIMD leave, and it spills.
#pragma once
#include "raccess_common.hpp"

namespace prb {

namespace {

// where a helper puts the value of term t and where the folding wavefront finds it: xbuf[buf][t][lane]
struct ToLds {
  double (&xb)[kHB][kWave];
  int lane;
  __device__ __forceinline__ void operator()(int t, double x) const { xb[t][lane] = x; }
  __device__ __forceinline__ double operator()(int t) const { return xb[t][lane]; }
};

// the fold of a batch, in order; a term that does not exist leaves the sum as it is
template <int N, typename Src>
__device__ __forceinline__ void fold_batch(const RaLds &lds, double &temp, Src src) {
#pragma unroll
  for (int t = 0; t < N; t++) {
    const double x = src(t);
    const double r = ra_lse(lds, temp, x);
    temp = x != kNegInf ? r : temp;
  }
}

// ------------------------------------------------------------------------------ inside
// The cell (i, j' = j + 1) of span d = dtop - lane that column j closes (a lane without a cell: type 0, no terms).
struct InsideCell {
  bool cell;
  int d, i, type, bi1, bj; // bj = s[j] = s[j' - 1]
  int m, span_lo;          // rows u1 = 0 .. m (p = i + u1 <= j - 5), spans max(5, d - 30) .. d - u1
  double start;            // the hairpin term, what the fold starts from
};
__device__ __forceinline__ InsideCell inside_cell(const RaLds &lds, const unsigned char *s, int j, int dtop, int lane) {
  InsideCell c;
  c.d = dtop - lane;
  c.cell = c.d >= kTurn;
  c.i = c.cell ? j - c.d : 0;
  c.type = c.cell ? ra_bp(lds, s[c.i], s[j + 1]) : 0;
  c.bi1 = c.cell ? s[c.i + 1] : 0;
  c.bj = s[j];
  c.start = c.type != 0 ? ra_hairpin_energy(lds, c.type, c.d, c.bi1, c.bj) : 0.0;
  c.m = c.type != 0 ? imin(kMaxLoop, c.d - (kTurn + 2)) : -1;
  c.span_lo = imax(kTurn + 2, c.d - kMaxLoop);
  return c;
}

// Which terms: rows of Alpha_stem, u1 ascending, within a row the span ascending (p ascending, q ascending).  Integer work
// and the row masks in LDS, without a branch: a step that finds its row used up moves on ONE row and may come back
// empty-handed.  Every wavefront that runs it sees the same terms.
struct InsideTerms {
  int u1;
  uint32_t wbits; // the terms left in row u1: bit b = span span_lo + b
  bool more;
  __device__ __forceinline__ explicit InsideTerms(const InsideCell &c) : u1(-1), wbits(0), more(c.m >= 0) {}
  template <int N>
  __device__ __forceinline__ void next(const RowMasks &rm, const InsideCell &c, int (&su1)[N], int (&sspan)[N]) {
#pragma unroll
    for (int t = 0; t < N; t++) {
      const bool adv = more && wbits == 0 && u1 < c.m;
      u1 += adv ? 1 : 0;
      const uint32_t wnew = rowmask_window(rm, c.i + (u1 < 0 ? 0 : u1), c.span_lo, c.d - u1 - (u1 == 0 ? 1 : 0)); // (p, q) == (i, j) is excluded (:207)
      wbits = adv ? wnew : wbits;
      const bool has = more && wbits != 0;
      sspan[t] = c.span_lo + __builtin_ctz(wbits | 0x80000000u);
      su1[t] = has ? u1 : -1;
      wbits = has ? (wbits & (wbits - 1)) : wbits;
      more = more && (wbits != 0 || u1 < c.m);
    }
  }
};

// Their values, terms [T0, T1) of a batch: the band entries and sequence codes, all fetched together (a lane without a
// term reads its own cell), then the values - the table look-ups are independent of each other.
template <int T0, int T1, int N, typename Sink>
__device__ __forceinline__ void inside_values(const RaLds &lds, const double *big, const double *a_stem, const unsigned char *s, int S,
                                              int j, const InsideCell &c, const int (&su1)[N], const int (&sspan)[N], Sink sink) {
  double sts[T1 - T0];
  int su2[T1 - T0], sq[T1 - T0], sq1[T1 - T0], sp0[T1 - T0], sp1[T1 - T0];
#pragma unroll
  for (int t = 0; t < T1 - T0; t++) {
    const bool ok = su1[T0 + t] >= 0;
    const int p = ok ? c.i + su1[T0 + t] : c.i, q = ok ? p + sspan[T0 + t] : j;
    su2[t] = j - q;
    sts[t] = EM(a_stem, p, q);
    sq[t] = s[q];
    sq1[t] = s[q + 1];
    sp0[t] = s[p];
    sp1[t] = s[p + 1];
  }
#pragma unroll
  for (int t = 0; t < T1 - T0; t++) {
    const int u = su1[T0 + t];
    const int type2 = ra_rtype(ra_bp(lds, sp1[t], sq[t])); // (not 0 where the stem exists)
    const double z = ra_loop_energy_bf(lds, big, c.type, type2, u < 0 ? 0 : u, su2[t], c.bi1, c.bj, sp0[t], sq1[t]);
    sink(T0 + t, (u >= 0 && sts[t] != kNegInf && type2 != 0) ? sts[t] + z : kNegInf);
  }
}

// The closing term (:217-226): Alpha_multi plus ML closing, ML intern and the dangles; the value of Alpha_stemend.
__device__ __forceinline__ double inside_close(const RaLds &lds, const double *a_multi, int S, int j, const InsideCell &c, double temp) {
  using SL = RaSmallLayout;
  if (c.type == 0) return kNegInf;
  const int tt = ra_rtype(c.type);
  return ra_lse(lds, temp,
                EM(a_multi, c.i, j) + lds.small[SL::kMLclosing] + lds.small[SL::kMLintern] + lds.small[SL::kDangle3 + tt * 5 + c.bi1] +
                    lds.small[SL::kDangle5 + tt * 5 + c.bj]);
}

// ----------------------------------------------------------------------------- outside
// The cell (p, q) of span d = dbot + lane of column q (a lane without a cell: no pair, no terms).
struct OutsideCell {
  bool cell;
  int d, p, t2raw, type2, bp0, bq1;
  int u1top; // one above the first row: rows u1 = u1top - 1 .. 0 (i = p - u1 >= 1)
};
__device__ __forceinline__ OutsideCell outside_cell(const RaLds &lds, const unsigned char *s, int q, int dbot, int dmax, int W, int lane) {
  OutsideCell c;
  c.d = dbot + lane;
  c.cell = c.d <= dmax;
  c.p = c.cell ? q - c.d : 1;
  c.t2raw = c.cell ? ra_bp(lds, s[c.p + 1], s[q]) : 0;
  c.type2 = ra_rtype(c.t2raw);
  c.bp0 = c.cell ? s[c.p] : 0;
  c.bq1 = c.cell ? s[q + 1] : 0;
  c.u1top = c.t2raw != 0 ? imin(imin(kMaxLoop, c.p - 1), W + 1 - c.d) + 1 : 0;
  return c;
}

// Which terms: rows of Beta_stemend, u1 descending (i ascending), within a row the span ascending (j ascending): spans
// d + u1 .. d + u1 + u2max with j <= L - 1 and j - i <= W + 1.  (See InsideTerms.)
struct OutsideTerms {
  int u1;
  uint32_t wbits;
  int span0; // span of bit 0 of wbits
  bool more;
  __device__ __forceinline__ explicit OutsideTerms(const OutsideCell &c) : u1(c.u1top), wbits(0), span0(0), more(c.t2raw != 0 && c.u1top > 0) {}
  template <int N>
  __device__ __forceinline__ void next(const RowMasks &rm, const OutsideCell &c, int q, int L, int W, int (&su1)[N], int (&sspan)[N]) {
#pragma unroll
    for (int t = 0; t < N; t++) {
      const bool adv = more && wbits == 0 && u1 > 0;
      u1 -= adv ? 1 : 0;
      const int u2max = imin(imin(kMaxLoop - u1, L - 1 - q), W + 1 - c.d - u1);
      const int s0 = c.d + u1 + (u1 == 0 ? 1 : 0); // (i, j) == (p, q) is excluded (:377)
      const uint32_t wnew = rowmask_window(rm, c.p - u1, s0, c.d + u1 + u2max);
      wbits = adv ? wnew : wbits;
      span0 = adv ? s0 : span0;
      const bool has = more && wbits != 0;
      sspan[t] = span0 + __builtin_ctz(wbits | 0x80000000u);
      su1[t] = has ? u1 : -1;
      wbits = has ? (wbits & (wbits - 1)) : wbits;
      more = more && (wbits != 0 || u1 > 0);
    }
  }
};

// Their values, terms [T0, T1) of a batch (see inside_values).
template <int T0, int T1, int N, typename Sink>
__device__ __forceinline__ void outside_values(const RaLds &lds, const double *big, const double *b_stemend, const unsigned char *s,
                                               int S, int q, const OutsideCell &c, const int (&su1)[N], const int (&sspan)[N], Sink sink) {
  double ses[T1 - T0];
  int su2[T1 - T0], sj[T1 - T0], sj1[T1 - T0], si0[T1 - T0], si1[T1 - T0];
#pragma unroll
  for (int t = 0; t < T1 - T0; t++) {
    const bool ok = su1[T0 + t] >= 0;
    const int i = ok ? c.p - su1[T0 + t] : c.p, j = ok ? i + sspan[T0 + t] : q; // (a lane without a term reads its own cell)
    su2[t] = j - q;
    ses[t] = EM(b_stemend, i, j);
    sj[t] = s[j];
    sj1[t] = s[j + 1];
    si0[t] = s[i];
    si1[t] = s[i + 1];
  }
#pragma unroll
  for (int t = 0; t < T1 - T0; t++) {
    const int u = su1[T0 + t];
    const int type = ra_bp(lds, si0[t], sj1[t]);
    const double z = ra_loop_energy_bf(lds, big, type, c.type2, u < 0 ? 0 : u, su2[t], si1[t], sj[t], c.bp0, c.bq1);
    sink(T0 + t, (u >= 0 && ses[t] != kNegInf && type != 0) ? ses[t] + z : kNegInf);
  }
}

// What the fold of Beta_stem starts from (:369-372): the exterior term.
__device__ __forceinline__ double outside_start(const RaLds &lds, const SeqView &v, int q, const OutsideCell &c) {
  return c.t2raw != 0 ? v.v(V_AO)[c.p] + v.v(V_BO)[q] + dangle_energy(lds, v, c.t2raw, c.p, q) : 0.0;
}

// The closing terms (:395-408): the stacked pair outside, then Beta_multi2; the value of Beta_stem.
__device__ __forceinline__ double outside_close(const RaLds &lds, const SeqView &v, int q, const OutsideCell &c, double temp) {
  using SL = RaSmallLayout;
  if (c.t2raw == 0) return kNegInf;
  const int S = v.S;
  if (c.p != 0 && q != v.L) {
    const int type = ra_bp(lds, c.bp0, c.bq1);
    if (type != 0 && c.d + 2 <= v.W + 1) {
      const double ps = EM(v.tab(B_STEM), c.p - 1, q + 1);
      if (ps != kNegInf) temp = ra_lse(lds, temp, ps + lds.small[SL::kStack + type * 7 + c.type2]);
    }
  }
  double out = temp;
  const double m2 = EM(v.tab(B_MULTI2), c.p, q);
  if (m2 != kNegInf) {
    const double x = m2 + lds.small[SL::kMLintern] + dangle_energy(lds, v, c.t2raw, c.p, q);
    out = ra_lse(lds, x, out);
  }
  return out;
}

} // namespace

} // namespace prb
