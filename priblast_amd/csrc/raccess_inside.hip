// Raccess, the inside pass: k_inside <-> Raccess::CalcInsideVariable, raccess.cpp:99-242 (mapping: raccess_common.hpp).
#include "raccess_fold.hpp"

namespace prb {

namespace {

// ------------------------------------------------------------------------------ inside
// kH = 0: a wavefront per sequence, four sequences per workgroup (throughput: thousands of sequences side by side).
// kH = 1, 2: a WORKGROUP per sequence - its first wavefront owns the sequence as before, the others are helpers for the
// one phase that is 35 % of a pass, the big fold: they walk the same row masks (the iterator is integer work, every
// wavefront runs it and so knows without a word how many rounds there are), evaluate the terms of the NEXT batch of eight -
// fetch, loop energies - into LDS while the owner folds the batch before; a workgroup barrier per batch.  The fold order
// is untouched.  For the few sequences of a query batch, whose time is the latency of one wavefront's chain.
// kH = 3: two helpers and a FOLDING wavefront; the sequence's own wavefront keeps phases 1 - 3 and the last step of phase 4.
// The big fold of column j needs nothing of phases 2 and 3 until its very end (Alpha_multi, one term), and they need nothing
// of it: phase 1, a barrier, then the fold (helpers -> folding wavefront, LDS counters) BESIDE phases 2 + 3, a barrier, the
// last term.  A column costs phase 1 + the longer of the two instead of their sum.
template <int NP, int kH>
__global__ __launch_bounds__(kH ? kWave * (1 + kH) : kBlock, kH ? 1 : PRB_RA_WPS) void k_inside(RaBatch b, RaConst c) {
  constexpr bool kF = kH == 3;
  __shared__ RaLds lds;
  __shared__ RowMasks rowmasks[kH ? 1 : kWavesPerBlock];
  __shared__ double xbuf[kH ? 2 : 1][kHB][kH ? kWave : 1]; // kH > 0: the terms of two batches, [batch & 1][term][lane]
  __shared__ int xflag[2];                                       // ... and whether there is a batch after them
  __shared__ FoldSync fsync;
  __shared__ double fold_out[kF ? NP : 1][kF ? kWave : 1]; // kF: the folds of a column's cells, [pass][lane]
  if (kF && threadIdx.x == 0) fsync.prod[0] = fsync.prod[1] = fsync.cons = fsync.abort = 0;
  int seq = 0; // kF: batches so far (the same count in the helpers and the folding wavefront)
  ra_load_lds(lds, c);
  const int lane = threadIdx.x & 63;
  const int role = kH ? (int)(threadIdx.x >> 6) : 0; // 0: the sequence's own wavefront
  const int idx = kH ? (int)blockIdx.x : (int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (idx >= b.nseq) return; // (kH > 0: the whole workgroup)
  RowMasks &rm = rowmasks[kH ? 0 : (threadIdx.x >> 6)]; // rows of Alpha_stem
  RA_PROF_DECL;
  const bool use_masks = b.W + 2 + kMaxLoop <= 128; // spans <= W + 1 fit a mask, live rows <= W + 2 + MAXLOOP fit the ring (kH > 0: the host made sure)
  if (role == 0)
    for (int t = lane; t < 128; t += kWave) rowmask_clear(rm, t);
  using SL = RaSmallLayout;
  const SeqView v = make_view(b, idx);
  const int L = v.L, W = v.W, S = v.S;
  const unsigned char *s = v.s;
  double *a_stem = v.tab(A_STEM), *a_stemend = v.tab(A_STEMEND), *a_multi = v.tab(A_MULTI);
  double *a_multibif = v.tab(A_MULTIBIF), *a_multi1 = v.tab(A_MULTI1), *a_multi2 = v.tab(A_MULTI2);
  double *a_multi1t = v.tab(A_MULTI1_T);
  double *ao = v.v(V_AO);
  const double MLbase = lds.small[SL::kMLbase], MLintern = lds.small[SL::kMLintern],
               MLclosing = lds.small[SL::kMLclosing];

  for (int j = kTurn + 1; j <= L; j++) {
    // cells of column j: spans d = 3..dmax, start i = j - d >= max(0, j-W-1).
    // lane mapping: d = dtop - lane, dtop = dmax, dmax-64, ...  (the last pass holds the
    // small spans, which are the cheap ones in every inside phase)
    const int dmax = imin(j, W + 1);
    double to_reg[NP], mb_reg[NP];
    if (role == 0) { // ---- phases 1 - 3: the sequence's own wavefront ----
    if (lane == 0) rowmask_clear(rm, j - 2); // the row that gets its first cell in column j + 1

    // phase 1: Alpha_stem (raccess.cpp:102-129) and Alpha_multi2 (:145-162): both need only
    // column j-1 and the cell itself.  Also, per cell, the term it contributes to Alpha_outer[j] (:230-241),
    // kept in a register for the chain of phase 3.
#pragma unroll
    for (int k = 0; k < NP; k++) to_reg[k] = mb_reg[k] = kNegInf;
    int pass = 0;
    for (int dtop = dmax; dtop >= kTurn; dtop -= kWave, pass++) {
      const int d = dtop - lane;
      if (d < kTurn) continue;
      const int i = j - d;
      const int type = ra_bp(lds, s[i + 1], s[j]);
      double stem = kNegInf;
      if (type != 0) {
        const int type2 = ra_rtype(ra_bp(lds, s[i + 2], s[j - 1]));
        double temp = 0;
        bool flag = false;
        const double ps = EM(a_stem, i + 1, j - 1), pe = EM(a_stemend, i + 1, j - 1);
        if (ps != kNegInf) {
          if (type2 != 0) temp = ps + lds.small[SL::kStack + type * 7 + type2];
          flag = true;
        }
        if (pe != kNegInf) {
          temp = flag ? ra_lse(lds, temp, pe) : pe;
          flag = true;
        }
        stem = flag ? temp : kNegInf;
      }
      EM(a_stem, i, j) = stem;
      if (use_masks && stem != kNegInf) rowmask_set(rm, i, d);
      double temp = 0;
      bool flag = false;
      if (type != 0 && stem != kNegInf) {
        const double dng = dangle_energy(lds, v, type, i, j);
        temp = stem + MLintern + dng;
        flag = true;
        const double x = stem + dng; // (:235-236)
        reg_set<NP>(to_reg, pass, x + ao[i]);
      }
      const double prev = EM(a_multi2, i, j - 1);
      double m2;
      if (prev != kNegInf) {
        m2 = prev + MLbase;
        if (flag) m2 = ra_lse(lds, temp, m2);
      } else {
        m2 = flag ? temp : kNegInf;
      }
      EM(a_multi2, i, j) = m2;
    }
    wave_sync();
    RA_PROF(1);
    } // role == 0
    if constexpr (kF) __syncthreads(); // phase 1 (Alpha_stem, the row masks) before the helpers read them

    if (role == 0) {
    // phase 2: Alpha_multibif (:131-143) then Alpha_multi1 (:164-175)
    int pass = 0;
    for (int dtop = dmax; dtop >= kTurn; dtop -= kWave, pass++) {
      const int d = dtop - lane;
      const bool cell = d >= kTurn;
      const int i = cell ? j - d : j - kTurn;
      double temp = 0;
      bool flag = false;
      // (operands of eight terms fetched together, then folded in order: k = i + t, t = 1 .. d - 1)
      for (int t0 = 1; t0 < dtop; t0 += kRaAhead) {
        double vs[kRaAhead];
#pragma unroll
        for (int b = 0; b < kRaAhead; b++) {
          const bool in = cell && t0 + b < d;
          const int t = in ? t0 + b : 1; // (a lane without a term reads one of its own)
          const double m1 = EM(a_multi1, i, i + t), m2 = EM(a_multi2, i + t, j);
          vs[b] = (in && m1 != kNegInf && m2 != kNegInf) ? m1 + m2 : kNegInf;
        }
#pragma unroll
        for (int b = 0; b < kRaAhead; b++)
          if (vs[b] != kNegInf) {
            temp = flag ? ra_lse(lds, temp, vs[b]) : vs[b];
            flag = true;
          }
      }
      if (!cell) continue;
      const double mb = flag ? temp : kNegInf;
      reg_set<NP>(mb_reg, pass, mb);
      EM(a_multibif, i, j) = mb;
      const double m2 = EM(a_multi2, i, j);
      double m1;
      if (m2 != kNegInf && mb != kNegInf) m1 = ra_lse(lds, m2, mb);
      else if (m2 == kNegInf) m1 = mb;
      else m1 = m2;
      EM(a_multi1, i, j) = m1;
      SM(a_multi1t, i, j) = m1;
    }
    wave_sync();
    RA_PROF(2);

    // phase 3, two serial chains in ONE instruction stream on lanes 0 and 1: Alpha_multi (:177-191), i descending
    // (d ascending), and Alpha_outer[j] (:230-241), p ascending (d descending).  A step's inputs come from the
    // registers of the lanes that computed them (v_readlane), not through memory, so a step is one logsumexp.
    {
      const bool l0 = lane == 0;
      double acc = l0 ? kNegInf : ao[j - 1]; // lane 0: Alpha_multi of the previous cell (none before d = 3); lane 1: the running sum
      for (int k = 0; k + kTurn <= dmax; k++) {
        const int d0 = kTurn + k, d1 = dmax - k;
        const double mb = cell_value_desc<NP>(mb_reg, dmax, d0), to = cell_value_desc<NP>(to_reg, dmax, d1);
        if (lane < 2) {
          const double term = l0 ? mb : to;
          const double base = l0 ? acc + MLbase : acc;
          const double r = ra_lse(lds, base, term);
          if (l0) {
            const double m = acc != kNegInf ? (mb != kNegInf ? r : base) : mb;
            EM(a_multi, j - d0, j) = m;
            acc = m;
          } else if (to != kNegInf) {
            acc = r;
          }
        }
      }
      if (lane == 1) ao[j] = acc;
    }
    wave_sync();
    RA_PROF(3);
    } // role == 0

    // phase 4: Alpha_stemend (:193-226).  The enclosed stems (p = i + u1, q = j - u2) are folded in the
    // reference's order - p ascending, q ascending - by the lane that owns the cell; a lane walks only the
    // terms that exist (set bits of the rows of Alpha_stem, spans max(5, d - 30) .. d - u1), eight at a time:
    // their band entries and sequence codes are fetched together, then folded one by one.
    // (The pieces - InsideCell, InsideTerms, inside_values, fold_batch, inside_close - are in raccess_fold.hpp; the forms
    // below differ in who runs which of them and in how a batch gets from one wavefront to another.)
    if constexpr (kF) {
      if (role != 0 && j != L) {
        int pass = 0;
        for (int dtop = dmax; dtop >= kTurn; dtop -= kWave, pass++) {
          const InsideCell ce = inside_cell(lds, s, j, dtop, lane);
          double temp = ce.start;
          InsideTerms it(ce);
          bool pend = __ballot(it.more) != 0; // (the same in every wavefront: from the cells themselves)
          while (pend) {
            const ToLds xb{xbuf[seq & 1], lane};
            if (role == 3) { // the fold
              if (!fold_wait(fsync, fsync.prod[0], seq + 1, b.watchdog) || !fold_wait(fsync, fsync.prod[1], seq + 1, b.watchdog)) return;
              fold_batch<kHB>(lds, temp, xb);
              pend = xflag[seq & 1] != 0;
              fold_post(fsync.cons, seq + 1, lane);
            } else { // a helper: which terms (both, identically), the values of its half of the batch
              if (!fold_wait(fsync, fsync.cons, seq - 1, b.watchdog)) return; // (the batch that was in this buffer is folded)
              int su1[kHB], sspan[kHB];
              it.next(rm, ce, su1, sspan);
              if (role == 1) inside_values<0, kHB / 2>(lds, c.big, a_stem, s, S, j, ce, su1, sspan, xb);
              else inside_values<kHB / 2, kHB>(lds, c.big, a_stem, s, S, j, ce, su1, sspan, xb);
              pend = __ballot(it.more) != 0;
              if (role == 1 && lane == 0) xflag[seq & 1] = pend ? 1 : 0;
              fold_post(fsync.prod[role - 1], seq + 1, lane);
            }
            seq++;
          }
          if (role == 3) fold_out[pass][lane] = temp;
        }
      }
      __syncthreads(); // the folds, and phases 2 - 3 (Alpha_multi) beside them
      if (role == 0 && j != L) { // the last term of phase 4
        int pass = 0;
        for (int dtop = dmax; dtop >= kTurn; dtop -= kWave, pass++) {
          const InsideCell ce = inside_cell(lds, s, j, dtop, lane);
          if (ce.cell) EM(a_stemend, ce.i, j) = inside_close(lds, a_multi, S, j, ce, fold_out[pass][lane]);
        }
      }
    } else if constexpr (kH > 0) {
      __syncthreads(); // the owner's phases 1 - 3 (Alpha_stem, the row masks) before the helpers read them
      if (j != L) {
        for (int dtop = dmax; dtop >= kTurn; dtop -= kWave) {
          const InsideCell ce = inside_cell(lds, s, j, dtop, lane);
          double temp = ce.start;
          InsideTerms it(ce);
          // (is there another batch?  Before the first: every wavefront sees it from the cells themselves; from then on
          // the first helper says so - the owner does not walk the masks at all, its rounds are the fold alone)
          bool pend = __ballot(it.more) != 0;
          for (int r = 0;; r++) {
            if (pend && role != 0) { // a helper: the next batch into xbuf[r & 1]
              const ToLds xb{xbuf[r & 1], lane};
              int su1[kHB], sspan[kHB];
              it.next(rm, ce, su1, sspan);
              if (kH == 1) inside_values<0, kHB>(lds, c.big, a_stem, s, S, j, ce, su1, sspan, xb);
              else if (role == 1) inside_values<0, kHB / 2>(lds, c.big, a_stem, s, S, j, ce, su1, sspan, xb);
              else inside_values<kHB / 2, kHB>(lds, c.big, a_stem, s, S, j, ce, su1, sspan, xb);
              const bool nxt = __ballot(it.more) != 0; // (every lane of the helper takes part)
              if (role == 1 && lane == 0) xflag[(r + 1) & 1] = nxt ? 1 : 0;
            }
            if (role == 0 && r >= 1) fold_batch<kHB>(lds, temp, ToLds{xbuf[(r - 1) & 1], lane}); // the fold, one batch behind
            __syncthreads();
            if (!pend) break;
            pend = xflag[(r + 1) & 1] != 0;
          }
          if (role == 0 && ce.cell) EM(a_stemend, ce.i, j) = inside_close(lds, a_multi, S, j, ce, temp);
        }
      }
    }
    // (kH = 0 keeps its own copy of the pieces, as they were: built from the shared ones, the throughput form needs
    // more registers than three wavefronts per SIMD leave and spills)
    if (kH == 0 && j != L && use_masks) {
      const int bj = s[j]; // = s[j'-1] for the closing pair (i, j' = j+1)
      for (int dtop = dmax; dtop >= kTurn; dtop -= kWave) {
        const int d = dtop - lane;
        const bool cell = d >= kTurn;
        const int i = cell ? j - d : 0;
        const int type = cell ? ra_bp(lds, s[i], s[j + 1]) : 0;
        const int bi1 = cell ? s[i + 1] : 0;
        double temp = type != 0 ? ra_hairpin_energy(lds, type, d, bi1, bj) : 0.0;
        // this lane's terms: rows u1 = 0 .. m, p <= j - 5
        const int m = type != 0 ? imin(kMaxLoop, d - (kTurn + 2)) : -1;
        const int span_lo = imax(kTurn + 2, d - kMaxLoop);
        int u1 = -1;
        uint32_t wbits = 0; // the terms left in row u1: bit b = span span_lo + b
        bool more = m >= 0;
        // One batch = the next eight terms of this lane, as values: (1) which terms - integer work and the row masks in
        // LDS, without a branch: a step that finds its row used up moves on ONE row and may come back empty-handed;
        // (2) their band entries and sequence codes, all fetched together (a lane without a term reads its own cell);
        // (3) their values - the table look-ups are independent of each other.
        auto next_batch = [&](double (&xs)[kRaAhead]) {
          int su1[kRaAhead], sspan[kRaAhead];
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const bool adv = more && wbits == 0 && u1 < m;
            u1 += adv ? 1 : 0;
            const uint32_t wnew = rowmask_window(rm, i + (u1 < 0 ? 0 : u1), span_lo, d - u1 - (u1 == 0 ? 1 : 0)); // (p, q) == (i, j) is excluded (:207)
            wbits = adv ? wnew : wbits;
            const bool has = more && wbits != 0;
            sspan[t] = span_lo + __builtin_ctz(wbits | 0x80000000u);
            su1[t] = has ? u1 : -1;
            wbits = has ? (wbits & (wbits - 1)) : wbits;
            more = more && (wbits != 0 || u1 < m);
          }
          double sts[kRaAhead];
          int su2[kRaAhead], sq[kRaAhead], sq1[kRaAhead], sp0[kRaAhead], sp1[kRaAhead];
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const bool ok = su1[t] >= 0;
            const int p = ok ? i + su1[t] : i, q = ok ? p + sspan[t] : j;
            su2[t] = j - q;
            sts[t] = EM(a_stem, p, q);
            sq[t] = s[q];
            sq1[t] = s[q + 1];
            sp0[t] = s[p];
            sp1[t] = s[p + 1];
          }
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const int type2 = ra_rtype(ra_bp(lds, sp1[t], sq[t])); // (not 0 where the stem exists)
            const double z = ra_loop_energy_bf(lds, c.big, type, type2, su1[t] < 0 ? 0 : su1[t], su2[t], bi1, bj, sp0[t], sq1[t]);
            xs[t] = (su1[t] >= 0 && sts[t] != kNegInf && type2 != 0) ? sts[t] + z : kNegInf;
          }
        };
        // The fold - a chain of dependent logsumexp, what a column costs - runs one batch behind: the next batch is
        // prepared in the same stretch of straight-line code, so its loads and look-ups fill the chain's stalls.
        double xs[kRaAhead];
        bool pending = __ballot(more) != 0;
        if (pending) next_batch(xs);
        while (pending) {
          double xn[kRaAhead];
          const bool again = __ballot(more) != 0;
          if (again) next_batch(xn);
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const double r = ra_lse(lds, temp, xs[t]);
            temp = xs[t] != kNegInf ? r : temp;
          }
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) xs[t] = xn[t];
          pending = again;
        }
        if (cell) {
          double out = kNegInf;
          if (type != 0) {
            const int tt = ra_rtype(type);
            out = ra_lse(lds, temp,
                         EM(a_multi, i, j) + MLclosing + MLintern + lds.small[SL::kDangle3 + tt * 5 + bi1] +
                             lds.small[SL::kDangle5 + tt * 5 + bj]);
          }
          EM(a_stemend, i, j) = out;
        }
      }
    }
    if (kH == 0 && j != L && !use_masks) {
      // (spans beyond the row masks: every (u1, u2) term of the window is enumerated wave-uniformly)
      const int bj = s[j]; // = s[j'-1] for the closing pair (i, j' = j+1)
      for (int dtop = dmax; dtop >= kTurn; dtop -= kWave) {
        const int d = dtop - lane;
        const bool cell = d >= kTurn;
        const int i = cell ? j - d : 0;
        const int type = cell ? ra_bp(lds, s[i], s[j + 1]) : 0;
        const int bi1 = cell ? s[i + 1] : 0;
        double temp = type != 0 ? ra_hairpin_energy(lds, type, d, bi1, bj) : 0.0;
        // p <= j-5 and q >= p+5  <=>  u1 + u2 <= d - 5; the pass bound uses dtop
        const int m = imin(kMaxLoop, dtop - (kTurn + 2));
        // (terms in blocks of kRaAhead: the band entries and sequence codes of a block are fetched
        // together, so their HBM / L2 latency is paid once per block, not once per term; the fold
        // itself stays in the reference's order)
        for (int u1 = 0; u1 <= m; u1++) {
          const int p = i + u1;
          const int bp1 = type != 0 ? s[p + 1] : 0, bp0 = type != 0 ? s[p] : 0;
          for (int u2hi = imin(kMaxLoop - u1, dtop - (kTurn + 2) - u1); u2hi >= 0; u2hi -= kRaAhead) {
            double sts[kRaAhead];
            int sq[kRaAhead], sq1[kRaAhead];
#pragma unroll
            for (int b = 0; b < kRaAhead; b++) {
              const int u2 = u2hi - b;
              // the (p,q) == (i,j) term is excluded (:207)
              const bool ok = u2 >= 0 && !(u1 == 0 && u2 == 0) && type != 0 && u1 + u2 <= d - (kTurn + 2);
              const int q = j - u2;
              sts[b] = ok ? EM(a_stem, p, q) : kNegInf;
              sq[b] = ok ? s[q] : 0;
              sq1[b] = ok ? s[q + 1] : 0;
            }
#pragma unroll
            for (int b = 0; b < kRaAhead; b++) {
              const double st = sts[b];
              if (st != kNegInf) {
                int type2 = ra_bp(lds, bp1, sq[b]);
                if (type2 != 0) {
                  type2 = ra_rtype(type2);
                  const double z = ra_loop_energy(lds, c.big, type, type2, u1, u2hi - b, bi1, bj, bp0, sq1[b]);
                  temp = ra_lse(lds, temp, st + z);
                }
              }
            }
          }
        }
        if (cell) {
          double out = kNegInf;
          if (type != 0) {
            const int tt = ra_rtype(type);
            out = ra_lse(lds, temp,
                         EM(a_multi, i, j) + MLclosing + MLintern + lds.small[SL::kDangle3 + tt * 5 + bi1] +
                             lds.small[SL::kDangle5 + tt * 5 + bj]);
          }
          EM(a_stemend, i, j) = out;
        }
      }
    }
    wave_sync();
    RA_PROF(4);
  }
}

} // namespace

void ra_launch_inside(const RaBatch &b, const RaConst &c, hipStream_t stream) {
  const RaForm f = ra_form(b);
  if (f.np == 4) ra_launch_form(k_inside<4, 0>, 0, b, c, stream);
  else if (f.helpers == 3) ra_launch_form(k_inside<2, 3>, 3, b, c, stream);
  else if (f.helpers == 2) ra_launch_form(k_inside<2, 2>, 2, b, c, stream);
  else if (f.helpers == 1) ra_launch_form(k_inside<2, 1>, 1, b, c, stream);
  else ra_launch_form(k_inside<2, 0>, 0, b, c, stream);
}
#ifdef PRB_GAP_PROFILE
int ra_inside_profile(unsigned long long *out, int reset) { return ra_profile_add(out, reset); }
#endif

} // namespace prb
