// Raccess, the outside pass: k_outside <-> Raccess::CalcOutsideVariable, raccess.cpp:258-412 (mapping: raccess_common.hpp).
#include "raccess_fold.hpp"

namespace prb {

namespace {

// ----------------------------------------------------------------------------- outside
// (kH: helper wavefronts for the big fold, see k_inside)
// kH = 3: phase A, a barrier, then the big fold of phase E (helpers -> folding wavefront) beside phases B - D on the
// sequence's own wavefront, a barrier, the last two terms of phase E (they need Beta_multi2 of phase D) - see k_inside.
template <int NP, int kH>
__global__ __launch_bounds__(kH ? kWave * (1 + kH) : kBlock, kH ? 1 : PRB_RA_WPS) void k_outside(RaBatch b, RaConst c) {
  constexpr bool kF = kH == 3;
  __shared__ RaLds lds;
  __shared__ RowMasks rowmasks[kH ? 1 : kWavesPerBlock];
  __shared__ double xbuf[kH ? 2 : 1][kHB][kH ? kWave : 1];
  __shared__ int xflag[2];
  __shared__ FoldSync fsync;
  __shared__ double fold_out[kF ? NP : 1][kF ? kWave : 1];
  if (kF && threadIdx.x == 0) fsync.prod[0] = fsync.prod[1] = fsync.cons = fsync.abort = 0;
  int seq = 0;
  ra_load_lds(lds, c);
  const int lane = threadIdx.x & 63;
  const int role = kH ? (int)(threadIdx.x >> 6) : 0;
  const int idx = kH ? (int)blockIdx.x : (int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (idx >= b.nseq) return;
  RA_PROF_DECL;
  RowMasks &rm = rowmasks[kH ? 0 : (threadIdx.x >> 6)]; // rows of Beta_stemend
  const bool use_masks = b.W + 2 + kMaxLoop <= 128;
  if (role == 0)
    for (int t = lane; t < 128; t += kWave) rowmask_clear(rm, t);
  using SL = RaSmallLayout;
  const SeqView v = make_view(b, idx);
  const int L = v.L, W = v.W, S = v.S;
  const unsigned char *s = v.s;
  const double *a_stem = v.tab(A_STEM), *a_multi2 = v.tab(A_MULTI2), *a_multi1t = v.tab(A_MULTI1_T);
  double *b_stem = v.tab(B_STEM), *b_stemend = v.tab(B_STEMEND), *b_multi = v.tab(B_MULTI);
  double *b_multibif = v.tab(B_MULTIBIF), *b_multi1 = v.tab(B_MULTI1), *b_multi2 = v.tab(B_MULTI2);
  const double *ao = v.v(V_AO);
  double *bo = v.v(V_BO);
  const double MLbase = lds.small[SL::kMLbase], MLintern = lds.small[SL::kMLintern], MLclosing = lds.small[SL::kMLclosing];

  // Beta_outer[i] (raccess.cpp:260-271) is a serial chain over i descending that only reads
  // Alpha_stem; it runs on lane 1 one position ahead of the column loop.
  auto beta_outer_at = [&](int i) {
    double temp = bo[i + 1];
    for (int p = i + 1; p <= imin(i + W + 1, L); p++) {
      const double st = EM(a_stem, i, p);
      if (st != kNegInf) {
        const int type = ra_bp(lds, s[i + 1], s[p]);
        const double x = st + dangle_energy(lds, v, type, i, p);
        temp = ra_lse(lds, temp, x + bo[p]);
      }
    }
    bo[i] = temp;
  };

  for (int q = L; q >= kTurn + 1; q--) {
    // cells of column q: p = max(0,q-W-1) .. q-3 ascending <=> d = q - p descending from dmax.
    // lane mapping: d = dbot + lane, dbot = 3, 67, ... (the last pass holds the large
    // spans, which are the cheap ones in every outside phase)
    const int dmax = imin(q, W + 1);
    double xb_reg[NP], tob_reg[NP];
    const int pend_o = imin(q + W, L); // Beta_outer[q - 1] sums p' = q .. pend_o

    if (role == 0) { // ---- phases A - D: the sequence's own wavefront ----
    // phase A: Beta_stemend (:278-279), copy from column q+1
    if (use_masks && lane == 0) rowmask_clear(rm, q - W); // the row whose first cell comes in column q - 1 (spans >= W never exist)
    // Also, in registers for the chains of phase B: per cell the term it contributes to Beta_multi (:296-300), and
    // - one per lane, p' = q + lane (+ 64) - the terms of Beta_outer[q - 1] (:262-269).
#pragma unroll
    for (int k = 0; k < NP; k++) xb_reg[k] = tob_reg[k] = kNegInf;
    {
      int pass = 0;
      for (int dbot = kTurn; dbot <= dmax; dbot += kWave, pass++) {
        const int d = dbot + lane;
        if (q == L || d > dmax) continue;
        const int p = q - d;
        if (p != 0) {
          const double se = d >= W ? kNegInf : EM(b_stem, p - 1, q + 1);
          EM(b_stemend, p, q) = se;
          if (use_masks && se != kNegInf) rowmask_set(rm, p, d);
          if (se != kNegInf) {
            const int tt = ra_rtype(ra_bp(lds, s[p], s[q + 1]));
            const double x = se + MLclosing + MLintern + lds.small[SL::kDangle3 + tt * 5 + s[p + 1]] +
                             lds.small[SL::kDangle5 + tt * 5 + s[q]];
            reg_set<NP>(xb_reg, pass, x);
          }
        }
      }
      for (pass = 0; pass < NP; pass++) {
        const int pp = q + lane + 64 * pass;
        if (pp > pend_o) continue;
        const int i = q - 1;
        const double st = EM(a_stem, i, pp);
        if (st != kNegInf) {
          const int type = ra_bp(lds, s[i + 1], s[pp]);
          const double x = st + dangle_energy(lds, v, type, i, pp);
          reg_set<NP>(tob_reg, pass, x + bo[pp]);
        }
      }
    }
    wave_sync();
    RA_PROF(8);
    } // role == 0
    if constexpr (kF) __syncthreads(); // phase A (Beta_stemend, the row masks) before the helpers read them

    if (role == 0) {
    // phase B, two serial chains in one instruction stream (see k_inside's phase 3): Beta_multi (:281-308), p
    // ascending (d descending), on lane 0; Beta_outer[q - 1] (:260-271), p' ascending, on lane 1; inputs by v_readlane.
    {
      const bool l0 = lane == 0;
      const int k0n = q != L ? dmax - kTurn + 1 : 0, k1n = pend_o - q + 1;
      double acc = l0 ? kNegInf : bo[q]; // lane 0: Beta_multi of the previous cell; lane 1: the running sum
      for (int k = 0; k < imax(k0n, k1n); k++) {
        const int d0 = dmax - k;
        const double xb = k < k0n ? lane_value_asc<NP>(xb_reg, d0 - kTurn) : kNegInf;
        const double to = k < k1n ? lane_value_asc<NP>(tob_reg, k) : kNegInf;
        if (lane < 2) {
          const double term = l0 ? xb : to;
          const double base = l0 ? acc + MLbase : acc;
          const double r = ra_lse(lds, base, term);
          if (l0) {
            const int p = q - d0;
            if (k < k0n && p != 0) {
              const bool flag = d0 + 1 <= W + 1 && acc != kNegInf; // (Beta_multi[p - 1][q - p + 1] exists)
              const double temp = xb != kNegInf ? (flag ? r : xb) : (flag ? base : kNegInf);
              EM(b_multi, p, q) = temp;
              acc = temp;
            }
          } else if (to != kNegInf) {
            acc = r;
          }
        }
      }
      if (lane == 1) bo[q - 1] = acc;
    }
    wave_sync();
    RA_PROF(9);

    if (q != L) {
      // phase C: Beta_multi1 (:310-324) then Beta_multibif (:354-364)
      for (int dbot = kTurn; dbot <= dmax; dbot += kWave) {
        const int d = dbot + lane;
        if (d > dmax) continue;
        const int p = q - d;
        if (p == 0) continue;
        double temp = 0;
        bool flag = false;
        const int kend = imin(L, p + W);
        // (operands of eight terms fetched together, then folded in order)
        for (int k0 = q + 1; k0 <= kend; k0 += kRaAhead) {
          double vs[kRaAhead];
#pragma unroll
          for (int b = 0; b < kRaAhead; b++) {
            const bool in = k0 + b <= kend;
            const int k = in ? k0 + b : q + 1;
            const double bb = EM(b_multibif, p, k), m2 = EM(a_multi2, q, k);
            vs[b] = (in && bb != kNegInf && m2 != kNegInf) ? bb + m2 : kNegInf;
          }
#pragma unroll
          for (int b = 0; b < kRaAhead; b++)
            if (vs[b] != kNegInf) {
              temp = flag ? ra_lse(lds, temp, vs[b]) : vs[b];
              flag = true;
            }
        }
        const double m1 = flag ? temp : kNegInf;
        EM(b_multi1, p, q) = m1;
        const double mm = EM(b_multi, p, q);
        double mb;
        if (m1 != kNegInf && mm != kNegInf) mb = ra_lse(lds, m1, mm);
        else if (mm == kNegInf) mb = m1;
        else mb = mm;
        EM(b_multibif, p, q) = mb;
      }
      wave_sync();
      RA_PROF(10);

      // phase D: Beta_multi2 (:326-352)
      for (int dbot = kTurn; dbot <= dmax; dbot += kWave) {
        const int d = dbot + lane;
        if (d > dmax) continue;
        const int p = q - d;
        if (p == 0) continue;
        double temp = 0;
        bool flag = false;
        const double m1 = EM(b_multi1, p, q);
        if (m1 != kNegInf) {
          temp = m1;
          flag = true;
        }
        if (d <= W) {
          const double nx = EM(b_multi2, p, q + 1);
          if (nx != kNegInf) {
            temp = flag ? ra_lse(lds, temp, nx + MLbase) : nx + MLbase;
            flag = true;
          }
        }
        for (int k0 = imax(0, q - W); k0 < p; k0 += kRaAhead) { // (eight terms' operands together, as in phase C)
          double vs[kRaAhead];
#pragma unroll
          for (int b = 0; b < kRaAhead; b++) {
            const bool in = k0 + b < p;
            const int k = in ? k0 + b : p - 1; // (p >= 1 here)
            const double bb = EM(b_multibif, k, q), a1 = SM(a_multi1t, k, p);
            vs[b] = (in && bb != kNegInf && a1 != kNegInf) ? bb + a1 : kNegInf;
          }
#pragma unroll
          for (int b = 0; b < kRaAhead; b++)
            if (vs[b] != kNegInf) {
              temp = flag ? ra_lse(lds, temp, vs[b]) : vs[b];
              flag = true;
            }
        }
        EM(b_multi2, p, q) = flag ? temp : kNegInf;
      }
      wave_sync();
      RA_PROF(11);
    }

    } // role == 0
    // phase E: Beta_stem (:367-409).  Enclosing pairs (i = p - u1, j+1 = q + u2 + 1) in the reference's
    // order: i ascending, j ascending.  As in k_inside's phase 4, a lane walks only the terms whose
    // Beta_stemend entry exists (set bits of a window of the row masks), eight at a time: fetch, evaluate, fold.
    // (The pieces - OutsideCell, OutsideTerms, outside_values, fold_batch, outside_close - are in raccess_fold.hpp; the
    // forms below differ in who runs which of them and in how a batch gets from one wavefront to another.)
    if constexpr (kF) {
      if (role != 0) {
        int pass = 0;
        for (int dbot = kTurn; dbot <= dmax; dbot += kWave, pass++) {
          const OutsideCell ce = outside_cell(lds, s, q, dbot, dmax, W, lane);
          double temp = role == 3 ? outside_start(lds, v, q, ce) : 0.0;
          OutsideTerms it(ce);
          bool pend = __ballot(it.more) != 0;
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
              it.next(rm, ce, q, L, W, su1, sspan);
              if (role == 1) outside_values<0, kHB / 2>(lds, c.big, b_stemend, s, S, q, ce, su1, sspan, xb);
              else outside_values<kHB / 2, kHB>(lds, c.big, b_stemend, s, S, q, ce, su1, sspan, xb);
              pend = __ballot(it.more) != 0;
              if (role == 1 && lane == 0) xflag[seq & 1] = pend ? 1 : 0;
              fold_post(fsync.prod[role - 1], seq + 1, lane);
            }
            seq++;
          }
          if (role == 3) fold_out[pass][lane] = temp;
        }
      }
      __syncthreads(); // the folds, and phases B - D (Beta_multi2) beside them
      if (role == 0) { // the last terms of phase E
        int pass = 0;
        for (int dbot = kTurn; dbot <= dmax; dbot += kWave, pass++) {
          const OutsideCell ce = outside_cell(lds, s, q, dbot, dmax, W, lane);
          if (ce.cell) EM(b_stem, ce.p, q) = outside_close(lds, v, q, ce, fold_out[pass][lane]);
        }
      }
    } else {
    if constexpr (kH > 0) {
      __syncthreads(); // the owner's phases A - D (Beta_stemend, the row masks) before the helpers read them
      for (int dbot = kTurn; dbot <= dmax; dbot += kWave) { // (helpers: the host made sure that the row masks apply)
        const OutsideCell ce = outside_cell(lds, s, q, dbot, dmax, W, lane);
        double temp = outside_start(lds, v, q, ce);
        OutsideTerms it(ce);
        // (is there another batch?  Before the first: every wavefront sees it from the cells themselves; from then on
        // the first helper says so - the owner does not walk the masks at all, its rounds are the fold alone)
        bool pend = __ballot(it.more) != 0;
        for (int r = 0;; r++) {
          if (pend && role != 0) { // a helper: the next batch into xbuf[r & 1]
            const ToLds xb{xbuf[r & 1], lane};
            int su1[kHB], sspan[kHB];
            it.next(rm, ce, q, L, W, su1, sspan);
            if (kH == 1) outside_values<0, kHB>(lds, c.big, b_stemend, s, S, q, ce, su1, sspan, xb);
            else if (role == 1) outside_values<0, kHB / 2>(lds, c.big, b_stemend, s, S, q, ce, su1, sspan, xb);
            else outside_values<kHB / 2, kHB>(lds, c.big, b_stemend, s, S, q, ce, su1, sspan, xb);
            const bool nxt = __ballot(it.more) != 0; // (every lane of the helper takes part)
            if (role == 1 && lane == 0) xflag[(r + 1) & 1] = nxt ? 1 : 0;
          }
          if (role == 0 && r >= 1) fold_batch<kHB>(lds, temp, ToLds{xbuf[(r - 1) & 1], lane}); // the fold, one batch behind
          __syncthreads();
          if (!pend) break;
          pend = xflag[(r + 1) & 1] != 0;
        }
        if (role == 0 && ce.cell) EM(b_stem, ce.p, q) = outside_close(lds, v, q, ce, temp);
      }
    } else {
    // (kH = 0 keeps its own copy of the pieces, as they were: built from the shared ones, the throughput form spills more)
    for (int dbot = kTurn; dbot <= dmax; dbot += kWave) {
      const int d = dbot + lane;
      const bool cell = d <= dmax;
      const int p = cell ? q - d : 1;
      const int t2raw = cell ? ra_bp(lds, s[p + 1], s[q]) : 0;
      const int type2 = ra_rtype(t2raw);
      const int bp0 = cell ? s[p] : 0, bq1 = cell ? s[q + 1] : 0;
      double temp = 0;
      if (t2raw != 0) temp = ao[p] + bo[q] + dangle_energy(lds, v, t2raw, p, q);
      if (use_masks) {
        // rows u1 = u1max .. 0 (i = p - u1 >= 1), spans d + u1 .. d + u1 + u2max with j <= L - 1 and j - i <= W + 1
        int u1 = t2raw != 0 ? imin(imin(kMaxLoop, p - 1), W + 1 - d) + 1 : 0; // (one above the first row)
        uint32_t wbits = 0;
        int span0 = 0; // span of bit 0 of wbits
        bool more = t2raw != 0 && u1 > 0;
        // (as in k_inside's phase 4: which terms, without a branch; fetch; values - then the fold one batch behind)
        auto next_batch = [&](double (&xs)[kRaAhead]) {
          int su1[kRaAhead], sspan[kRaAhead];
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const bool adv = more && wbits == 0 && u1 > 0;
            u1 -= adv ? 1 : 0;
            const int u2max = imin(imin(kMaxLoop - u1, L - 1 - q), W + 1 - d - u1);
            const int s0 = d + u1 + (u1 == 0 ? 1 : 0); // (i, j) == (p, q) is excluded (:377)
            const uint32_t wnew = rowmask_window(rm, p - u1, s0, d + u1 + u2max);
            wbits = adv ? wnew : wbits;
            span0 = adv ? s0 : span0;
            const bool has = more && wbits != 0;
            sspan[t] = span0 + __builtin_ctz(wbits | 0x80000000u);
            su1[t] = has ? u1 : -1;
            wbits = has ? (wbits & (wbits - 1)) : wbits;
            more = more && (wbits != 0 || u1 > 0);
          }
          double ses[kRaAhead];
          int su2[kRaAhead], sj[kRaAhead], sj1[kRaAhead], si0[kRaAhead], si1[kRaAhead];
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const bool ok = su1[t] >= 0;
            const int i = ok ? p - su1[t] : p, j = ok ? i + sspan[t] : q; // (a lane without a term reads its own cell)
            su2[t] = j - q;
            ses[t] = EM(b_stemend, i, j);
            sj[t] = s[j];
            sj1[t] = s[j + 1];
            si0[t] = s[i];
            si1[t] = s[i + 1];
          }
#pragma unroll
          for (int t = 0; t < kRaAhead; t++) {
            const int type = ra_bp(lds, si0[t], sj1[t]);
            const double z = ra_loop_energy_bf(lds, c.big, type, type2, su1[t] < 0 ? 0 : su1[t], su2[t], si1[t], sj[t], bp0, bq1);
            xs[t] = (su1[t] >= 0 && ses[t] != kNegInf && type != 0) ? ses[t] + z : kNegInf;
          }
        };
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
      } else {
        // (spans beyond the row masks: every (u1, u2) term of the window is enumerated wave-uniformly)
        // j - i = d + u1 + u2 <= W + 1; the pass bound uses dbot
        const int m = imin(kMaxLoop, W + 1 - dbot);
        const int u1top = imin(m, q - dbot - 1); // i >= 1 for the smallest span of the pass
        for (int u1 = u1top; u1 >= 0; u1--) {
          const int u2top = imin(imin(kMaxLoop - u1, L - 1 - q), W + 1 - dbot - u1);
          const bool row = t2raw != 0 && u1 <= p - 1;
          const int i = p - u1;
          const int bi0 = row ? s[i] : 0, bi1 = row ? s[i + 1] : 0;
          for (int u2lo = 0; u2lo <= u2top; u2lo += kRaAhead) { // blocks of terms, see k_inside
            double ses[kRaAhead];
            int sj[kRaAhead], sj1[kRaAhead];
#pragma unroll
            for (int b = 0; b < kRaAhead; b++) {
              const int u2 = u2lo + b;
              // (i,j) == (p,q) is excluded (:377)
              const bool ok = row && u2 <= u2top && !(u1 == 0 && u2 == 0) && d + u1 + u2 <= W + 1;
              const int j = q + u2;
              ses[b] = ok ? EM(b_stemend, i, j) : kNegInf;
              sj[b] = ok ? s[j] : 0;
              sj1[b] = ok ? s[j + 1] : 0;
            }
#pragma unroll
            for (int b = 0; b < kRaAhead; b++) {
              const double se = ses[b];
              if (se != kNegInf) {
                const int type = ra_bp(lds, bi0, sj1[b]);
                if (type != 0) {
                  const double z = ra_loop_energy(lds, c.big, type, type2, u1, u2lo + b, bi1, sj[b], bp0, bq1);
                  temp = ra_lse(lds, temp, se + z);
                }
              }
            }
          }
        }
      }
      if (cell) {
        double out = kNegInf;
        if (t2raw != 0) {
          if (p != 0 && q != L) {
            const int type = ra_bp(lds, bp0, bq1);
            if (type != 0 && d + 2 <= W + 1) {
              const double ps = EM(b_stem, p - 1, q + 1);
              if (ps != kNegInf) temp = ra_lse(lds, temp, ps + lds.small[SL::kStack + type * 7 + type2]);
            }
          }
          out = temp;
          const double m2 = EM(b_multi2, p, q);
          if (m2 != kNegInf) {
            const double x = m2 + MLintern + dangle_energy(lds, v, t2raw, p, q);
            out = ra_lse(lds, x, out);
          }
        }
        if (role == 0) EM(b_stem, p, q) = out;
      }
    }
    }
    } // !kF
    wave_sync();
    RA_PROF(12);
  }
  // remaining Beta_outer positions (columns stop at q = 4)
  if (role == 0 && lane == 1)
    for (int i = (L >= kTurn + 1 ? kTurn - 1 : L - 1); i >= 0; i--) beta_outer_at(i);
}

} // namespace

void ra_launch_outside(const RaBatch &b, const RaConst &c, hipStream_t stream) {
  const RaForm f = ra_form(b);
  if (f.np == 4) ra_launch_form(k_outside<4, 0>, 0, b, c, stream);
  else if (f.helpers == 3) ra_launch_form(k_outside<2, 3>, 3, b, c, stream);
  else if (f.helpers == 2) ra_launch_form(k_outside<2, 2>, 2, b, c, stream);
  else if (f.helpers == 1) ra_launch_form(k_outside<2, 1>, 1, b, c, stream);
  else ra_launch_form(k_outside<2, 0>, 0, b, c, stream);
}
#ifdef PRB_GAP_PROFILE
int ra_outside_profile(unsigned long long *out, int reset) { return ra_profile_add(out, reset); }
#endif

} // namespace prb
