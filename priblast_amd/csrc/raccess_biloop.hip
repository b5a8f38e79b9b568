// Raccess, the bulge / interior-loop sums per position: k_biloop, k_biloop_win <-> CalcBulgeAndInternalProbability /
// CalcLogSumBulgeAndInternalProbability, raccess.cpp:614-771 (mapping: raccess_common.hpp).
#include "raccess_common.hpp"

namespace prb {

namespace {

// ------------------------------------------------------------- bulge / interior loops
// Ordered scatter of every interior-loop term into the positions it makes accessible
// (raccess.cpp:626-665 / :695-752).  The sums per position k are sequential in the
// reference, so tuples are applied one at a time in (i, j, p, q) order; the lanes own the
// positions (k mod 64, NS slots for windows up to 64 * NS positions), so one tuple updates all its
// positions in one predicated instruction.
template <int NS>
__device__ __forceinline__ double slot_get(const double (&a)[NS], int sl) {
  double r = a[0];
#pragma unroll
  for (int t = 1; t < NS; t++)
    if (sl == t) r = a[t];
  return r;
}
template <int NS>
__device__ __forceinline__ void slot_put(double (&a)[NS], int sl, double v) {
#pragma unroll
  for (int t = 0; t < NS; t++)
    if (sl == t) a[t] = v;
}

template <bool kLogSum, int NS>
__device__ void biloop_run(const RaLds &lds, const RaConst &c, const SeqView &v, int delta, int lane) {
  const int L = v.L, W = v.W, S = v.S;
  const unsigned char *s = v.s;
  const double *a_stem = v.tab(A_STEM), *b_stemend = v.tab(B_STEMEND);
  double *bp = v.v(V_BP), *cbp = v.v(V_CBP), *bfl = v.v(V_BFLAG), *cfl = v.v(V_CFLAG);
  // accumulators of position k live on lane k & 63, slot (k >> 6) & (NS - 1); "has a term" flags: one bit per slot
  double accb[NS], accc[NS];
#pragma unroll
  for (int t = 0; t < NS; t++) accb[t] = accc[t] = 0;
  unsigned fb = 0, fc = 0;

  for (int i = 1; i < L - kTurn - 2; i++) {
    const int kb = i + 1; // smallest position this and later i can touch
    const int jend = imin(i + W, L);
    for (int j = i + kTurn + 3; j <= jend; j++) {
      const int type = ra_bp(lds, s[i], s[j]);
      if (type == 0) continue;
      const double bs = EM(b_stemend, i, j - 1);
      if (bs == kNegInf) continue;
      const int D = j - i;
      const int m = imin(kMaxLoop, D - 6); // u1 + u2 <= m
      const int bi1 = s[i + 1], bj1 = s[j - 1];
      for (int u1 = 0; u1 <= m; u1++) {
        // lanes take the q of this p in the reference's order: q ascending <=> u2 descending
        const int p = i + 1 + u1;
        const int u2 = (m - u1) - lane;
        bool valid = u2 >= 0 && !(u1 == 0 && u2 == 0);
        double val = 0;
        int q = 0;
        if (valid) {
          q = j - 1 - u2;
          int type2 = ra_bp(lds, s[p], s[q]);
          const double as = EM(a_stem, p - 1, q);
          valid = type2 != 0 && as != kNegInf;
          if (valid) {
            type2 = ra_rtype(type2);
            const double e = bs + ra_loop_energy_bf(lds, c.big, type, type2, u1, u2, bi1, bj1, s[p - 1], s[q + 1]) + as;
            val = kLogSum ? e : ra_expd(lds, e);
          }
        }
        unsigned long long mask = __ballot(valid);
        const int kl1 = p - delta; // left range [i+1, p-delta]
        while (mask) {
          const int src = __builtin_ctzll(mask);
          mask &= mask - 1;
          const double tv = __shfl(val, src);
          const int tq = __shfl(q, src);
          const int kr0 = tq + 1, kr1 = j - delta; // right range [q+1, j-delta]
#pragma unroll
          for (int h = 0; h < NS; h++) {
            const int k = kb + ((lane - kb) & 63) + 64 * h;
            const bool inl = k <= kl1; // k >= kb = i+1 always
            const bool inr = k >= kr0 && k <= kr1;
            if (inl || inr) {
              const bool last = inl ? k == kl1 : k == kr1;
              const int sl = (k >> 6) & (NS - 1);
              if (!kLogSum) {
                if (last) slot_put<NS>(accb, sl, slot_get<NS>(accb, sl) + tv);
                else slot_put<NS>(accc, sl, slot_get<NS>(accc, sl) + tv);
              } else {
                if (last) {
                  const double cur = slot_get<NS>(accb, sl);
                  const double nv = ((fb >> sl) & 1) ? ra_lse(lds, cur, tv) : tv;
                  slot_put<NS>(accb, sl, nv);
                  fb |= 1u << sl;
                } else {
                  const double cur = slot_get<NS>(accc, sl);
                  const double nv = ((fc >> sl) & 1) ? ra_lse(lds, cur, tv) : tv;
                  slot_put<NS>(accc, sl, nv);
                  fc |= 1u << sl;
                }
              }
            }
          }
        }
      }
    }
    // position k = i+1 receives nothing from later i: store it and recycle the slot
    if ((kb & 63) == lane) {
      const int sl = (kb >> 6) & (NS - 1);
      bp[kb - 1] = slot_get<NS>(accb, sl);
      cbp[kb - 1] = slot_get<NS>(accc, sl);
      bfl[kb - 1] = ((fb >> sl) & 1) ? 1.0 : 0.0;
      cfl[kb - 1] = ((fc >> sl) & 1) ? 1.0 : 0.0;
      slot_put<NS>(accb, sl, 0.0);
      slot_put<NS>(accc, sl, 0.0);
      fb &= ~(1u << sl);
      fc &= ~(1u << sl);
    }
  }
  // positions beyond the last i keep their zero-initialised value: every position that
  // can receive a term (k <= L - delta, k >= 2) has been flushed when i passed k - 1,
  // except those with k - 1 >= L - 5; flush what the last windows left behind.
  for (int k = imax(2, L - kTurn - 2 + 1); k <= L; k++) {
    if ((k & 63) == lane) {
      const int sl = (k >> 6) & (NS - 1);
      bp[k - 1] = slot_get<NS>(accb, sl);
      cbp[k - 1] = slot_get<NS>(accc, sl);
      bfl[k - 1] = ((fb >> sl) & 1) ? 1.0 : 0.0;
      cfl[k - 1] = ((fc >> sl) & 1) ? 1.0 : 0.0;
      slot_put<NS>(accb, sl, 0.0);
      slot_put<NS>(accc, sl, 0.0);
      fb &= ~(1u << sl);
      fc &= ~(1u << sl);
    }
  }
}

// Linear branch, float-overflow regime: the un-normalised sums are only ever used as
// `(float)sum` under a log, and fmath::log(+inf) is the constant 88.722839.  A position whose sum
// contains ONE term expd(e) with e >= 89 (> FLT_MAX by a third) therefore has the same final value
// whatever the other terms and their order are, and a position without any non-zero term
// (e <= -708.39.. for all of them) stays exactly 0.  This pass only classifies: per position and
// per sum (bulge/interior "b", conditional "c") two bits - some term is that large / some term is
// non-zero - as order-independent ORs over the same (i, j, p, q) enumeration, without the
// tuple-by-tuple scatter.  It stores +inf / 0 where that decides the result (k_access's
// finalisation then takes the same branches as with the true sums) and returns false when some
// position needs its true sum, in which case the caller runs the ordered pass.  For random RNA
// of 1 kb (log Z ~ 270) every position is decided here.
template <int NS>
__device__ bool biloop_classify(const RaLds &lds, const RaConst &c, const SeqView &v, int delta, int lane) {
  const int L = v.L, W = v.W, S = v.S;
  const unsigned char *s = v.s;
  const double *a_stem = v.tab(A_STEM), *b_stemend = v.tab(B_STEMEND);
  double *bp = v.v(V_BP), *cbp = v.v(V_CBP);
  // flags of position k live on lane k & 63, in nibble (k >> 6) & (NS - 1) of one word: bit 0 b-big, 1 b-nonzero,
  // 2 c-big, 3 c-nonzero
  unsigned fl = 0;
  bool undecided = false;
  auto flush = [&](int k) {
    if ((k & 63) == lane) {
      const int sl = (k >> 6) & (NS - 1);
      const unsigned f = (fl >> (4 * sl)) & 15u;
      const bool bbig = f & 1, bnz = f & 2, cbig = f & 4, cnz = f & 8;
      if (!((cbig || !cnz) && (cbig || bbig || !bnz))) undecided = true;
      bp[k - 1] = bnz ? __builtin_huge_val() : 0.0;
      cbp[k - 1] = cnz ? __builtin_huge_val() : 0.0;
      fl &= ~(15u << (4 * sl));
    }
  };
  for (int i = 1; i < L - kTurn - 2; i++) {
    const int kb = i + 1; // smallest position this and later i can touch
    const int jend = imin(i + W, L);
    // the closing pairs (i, j) of this i that exist, found for all j at once: lane t looks at j = jb + t
    for (int jb = i + kTurn + 3; jb <= jend; jb += kWave) {
      const int jl = jb + lane;
      const int typ_l = jl <= jend ? ra_bp(lds, s[i], s[jl]) : 0;
      const double bs_l = typ_l != 0 ? EM(b_stemend, i, jl - 1) : kNegInf;
      unsigned long long jmask = __ballot(typ_l != 0 && bs_l != kNegInf);
      while (jmask) {
        const int jt = __builtin_ctzll(jmask);
        jmask &= jmask - 1;
        const int j = jb + jt;
        const int type = __builtin_amdgcn_readlane(typ_l, jt);
        const double bs = readlane_f64(bs_l, jt);
        const int D = j - i;
        const int m = imin(kMaxLoop, D - 6); // u1 + u2 <= m
        const int bi1 = s[i + 1], bj1 = s[j - 1];
        const int kr1 = j - delta;
        // The tuples (u1, u2), u2 = 0 .. m - u1, of row u1 make m - u1 + 1 lanes; rows a and m + 1 - a together make
        // m + 1 <= 31, so half a wavefront takes two rows and a pass four (row 0 and - m odd - the middle row go alone).
        // The flags are ORs, so only two things matter about a pass: which rows have a non-zero / a big term (the left
        // ranges [i + 1, p - delta] depend on the row only) and which columns q have one (the right ranges [q + 1,
        // j - delta] on the column only).  Both are collected from the ballots with scalar instructions; the positions
        // are updated once per (i, j), not once per row.
        unsigned long long col_nz = 0, col_big = 0; // bit = q - (j - 1 - m)
        unsigned row_nz = 0, row_big = 0;           // bit = u1
        const int nslots = 1 + (m + 1) / 2;         // (0), (1, m), (2, m - 1), ...
        for (int s0 = 0; s0 < nslots; s0 += 2) {
          const int half = lane >> 5, l5 = lane & 31;
          const int slot = s0 + half;
          const int ra_ = slot, rb_ = slot == 0 ? -1 : m + 1 - slot; // the slot's rows (rb_ <= ra_: none / the same row)
          const int na = slot < nslots ? m - ra_ + 1 : 0, nb = (slot < nslots && rb_ > ra_) ? m - rb_ + 1 : 0;
          const bool in_a = l5 < na, in_b = !in_a && l5 < na + nb;
          const int u1 = in_a ? ra_ : rb_, t5 = in_a ? l5 : l5 - na;
          const int u2 = (m - u1) - t5; // lane t of a row holds q = q0 + t, q0 = j - 1 - (m - u1)
          const bool in = (in_a || in_b) && !(u1 == 0 && u2 == 0);
          const int pp = in ? i + 1 + u1 : i + 1, q = in ? j - 1 - u2 : j - 1; // (a lane without a tuple reads inside the window)
          const int type2raw = ra_bp(lds, s[pp], s[q]);
          const double as = EM(a_stem, pp - 1, q);
          const double z = ra_loop_energy_bf(lds, c.big, type, ra_rtype(type2raw), in ? u1 : 0, in ? u2 : 0, bi1, bj1, s[pp - 1], s[q + 1]);
          const double e = bs + z + as;
          const bool ok = in && type2raw != 0 && as != kNegInf;
          const bool nz = ok && e > -708.39641853226408; // ra_expd(e) != 0
          const bool big = ok && e >= 89.0;
          const unsigned long long nzall = __ballot(nz);
          if (nzall == 0) continue;
          const unsigned long long bigall = __ballot(big);
#pragma unroll
          for (int h = 0; h < 2; h++) { // (wave-uniform: scalar instructions)
            const int sl = s0 + h;
            if (sl >= nslots) continue;
            const int a_ = sl, b_ = sl == 0 ? -1 : m + 1 - sl;
            const int n_a = m - a_ + 1, n_b = b_ > a_ ? m - b_ + 1 : 0;
            const unsigned hn = (unsigned)(nzall >> (32 * h)), hb = (unsigned)(bigall >> (32 * h));
            const unsigned an = hn & ((n_a >= 32 ? 0u : (1u << n_a)) - 1u), ab = hb & ((n_a >= 32 ? 0u : (1u << n_a)) - 1u);
            col_nz |= (unsigned long long)an << a_;
            col_big |= (unsigned long long)ab << a_;
            row_nz |= (an != 0 ? 1u : 0u) << a_;
            row_big |= (ab != 0 ? 1u : 0u) << a_;
            if (n_b > 0) {
              const unsigned bn = (hn >> n_a) & ((1u << n_b) - 1u), bb = (hb >> n_a) & ((1u << n_b) - 1u);
              col_nz |= (unsigned long long)bn << b_;
              col_big |= (unsigned long long)bb << b_;
              row_nz |= (bn != 0 ? 1u : 0u) << b_;
              row_big |= (bb != 0 ? 1u : 0u) << b_;
            }
          }
        }
        if (row_nz == 0) continue;
        // the positions: left ranges end at p - delta = i + 1 + u1 - delta, right ranges at j - delta
        const int qbase = j - 1 - m;
#pragma unroll
        for (int h = 0; h < NS; h++) {
          const int k = kb + ((lane - kb) & 63) + 64 * h;
          unsigned add = 0;
          const int ustar = k - (i + 1 - delta); // the row whose left range ends at k
          if (ustar >= 0 && ustar <= m) {
            if ((row_nz >> ustar) & 1) add |= 2u | (((row_big >> ustar) & 1) ? 1u : 0u);
          }
          if (ustar < m) { // rows above: k lies inside their left ranges
            const int sh = ustar < 0 ? 0 : ustar + 1;
            if (row_nz >> sh) add |= 8u | ((row_big >> sh) ? 4u : 0u);
          }
          if (k <= kr1) { // right ranges [q + 1, j - delta]: the tuples with q <= k - 1
            const int nl = k - qbase;
            if (nl > 0) {
              const unsigned long long below = nl >= 64 ? ~0ull : ((1ull << nl) - 1);
              if (col_nz & below) add |= (k == kr1 ? 2u : 8u) | ((col_big & below) ? (k == kr1 ? 1u : 4u) : 0u);
            }
          }
          fl |= add << (4 * ((k >> 6) & (NS - 1)));
        }
      }
    }
    flush(kb); // position i+1 receives nothing from later i
  }
  for (int k = imax(2, L - kTurn - 2 + 1); k <= L; k++) flush(k);
  return __ballot(undecided) == 0;
}

// The LOGSUM branch (|log Z| > 690, raccess.cpp:683-771) for a WINDOW of 64 positions: one logsumexp per (tuple,
// position) in the reference's (i, j, p, q) order makes the ordered pass above a chain of ~5,600 tuples per nucleotide
// on its one wavefront (2.35 ms per nucleotide: 47 s for a lone 20 kb sequence).  The sums of different positions do
// not depend on each other, only the order WITHIN a position matters: a wavefront owns positions k0 .. k0 + 63 (one per
// lane), walks the tuples of every i that can reach them (k - W + delta <= i <= k - 1) in the same order - the lanes
// evaluating the tuples of one (i, j, u1) side by side, as above -, and a lane folds a tuple in only if its position lies
// in one of the tuple's two ranges.  Every window costs what ~(W + 64) values of i cost, all windows of all sequences
// run at once: the time of a sequence no longer grows with its length.
// (kLogSum false: the linear branch, the same walk with plain sums of expd(e) - for the windows the classification below
// cannot decide, and for sequences with log Z < 120)
template <bool kLogSum>
__device__ void biloop_window(const RaLds &lds, const RaConst &c, const SeqView &v, int delta, int lane, int k0) {
  const int L = v.L, W = v.W, S = v.S;
  const int k = k0 + lane; // this lane's position
  const unsigned char *s = v.s;
  const double *a_stem = v.tab(A_STEM), *b_stemend = v.tab(B_STEMEND);
  double accb = 0, accc = 0;
  bool fb = false, fc = false;
  const int i_lo = imax(1, k0 - W + delta), i_hi = imin(L - kTurn - 3, k0 + kWave - 2); // i < L - kTurn - 2, i <= k - 1
  for (int i = i_lo; i <= i_hi; i++) {
    const int jend = imin(i + W, L);
    // (closing pairs whose right range ends before the window and whose left ranges cannot reach it either are skipped:
    // left ranges end at p - delta <= i + 1 + 30 - delta, right ranges at j - delta)
    for (int j = i + kTurn + 3; j <= jend; j++) {
      if (j - delta < k0 && i + 1 + kMaxLoop - delta < k0) continue;
      const int type = ra_bp(lds, s[i], s[j]);
      if (type == 0) continue;
      const double bs = EM(b_stemend, i, j - 1);
      if (bs == kNegInf) continue;
      const int D = j - i;
      const int m = imin(kMaxLoop, D - 6); // u1 + u2 <= m
      const int bi1 = s[i + 1], bj1 = s[j - 1];
      for (int u1 = 0; u1 <= m; u1++) {
        // lanes take the q of this p in the reference's order: q ascending <=> u2 descending
        const int p = i + 1 + u1;
        const int u2 = (m - u1) - lane;
        bool valid = u2 >= 0 && !(u1 == 0 && u2 == 0);
        double val = 0;
        int q = 0;
        if (valid) {
          q = j - 1 - u2;
          int type2 = ra_bp(lds, s[p], s[q]);
          const double as = EM(a_stem, p - 1, q);
          valid = type2 != 0 && as != kNegInf;
          if (valid) {
            type2 = ra_rtype(type2);
            const double e = bs + ra_loop_energy_bf(lds, c.big, type, type2, u1, u2, bi1, bj1, s[p - 1], s[q + 1]) + as;
            val = kLogSum ? e : ra_expd(lds, e);
          }
        }
        unsigned long long mask = __ballot(valid);
        const int kl1 = p - delta; // left range [i+1, p-delta]
        const bool inl = k >= i + 1 && k <= kl1;
        while (mask) {
          const int src = __builtin_ctzll(mask);
          mask &= mask - 1;
          const double tv = __shfl(val, src);
          const int tq = __shfl(q, src);
          const int kr0 = tq + 1, kr1 = j - delta; // right range [q+1, j-delta]
          const bool inr = k >= kr0 && k <= kr1;
          if (inl || inr) {
            const bool last = inl ? k == kl1 : k == kr1;
            if (!kLogSum) {
              if (last) accb += tv;
              else accc += tv;
            } else if (last) {
              accb = fb ? ra_lse(lds, accb, tv) : tv;
              fb = true;
            } else {
              accc = fc ? ra_lse(lds, accc, tv) : tv;
              fc = true;
            }
          }
        }
      }
    }
  }
  if (k <= L) {
    v.v(V_BP)[k - 1] = accb;
    v.v(V_CBP)[k - 1] = accc;
    v.v(V_BFLAG)[k - 1] = fb ? 1.0 : 0.0;
    v.v(V_CFLAG)[k - 1] = fc ? 1.0 : 0.0;
  }
}

// biloop_classify for a window of 64 positions (one per lane): the flags are order-independent ORs, so a window only
// has to look at the closing pairs whose ranges can reach it.  Stores +inf / 0 where that decides a position's sums and
// returns false when some position of the window needs its true sums.
__device__ bool biloop_classify_window(const RaLds &lds, const RaConst &c, const SeqView &v, int delta, int lane, int k0) {
  const int L = v.L, W = v.W, S = v.S;
  const int k = k0 + lane;
  const unsigned char *s = v.s;
  const double *a_stem = v.tab(A_STEM), *b_stemend = v.tab(B_STEMEND);
  unsigned fl = 0; // bit 0 b-big, 1 b-nonzero, 2 c-big, 3 c-nonzero
  const int i_lo = imax(1, k0 - W + delta), i_hi = imin(L - kTurn - 3, k0 + kWave - 2);
  for (int i = i_lo; i <= i_hi; i++) {
    const int jend = imin(i + W, L);
    for (int jb = i + kTurn + 3; jb <= jend; jb += kWave) {
      const int jl = jb + lane;
      const int typ_l = jl <= jend ? ra_bp(lds, s[i], s[jl]) : 0;
      const double bs_l = typ_l != 0 ? EM(b_stemend, i, jl - 1) : kNegInf;
      // (pairs that cannot reach the window: right ranges end at j - delta, left ranges at i + 1 + 30 - delta at the latest)
      unsigned long long jmask = __ballot(typ_l != 0 && bs_l != kNegInf && !(jl - delta < k0 && i + 1 + kMaxLoop - delta < k0));
      while (jmask) {
        const int jt = __builtin_ctzll(jmask);
        jmask &= jmask - 1;
        const int j = jb + jt;
        const int type = __builtin_amdgcn_readlane(typ_l, jt);
        const double bs = readlane_f64(bs_l, jt);
        const int D = j - i;
        const int m = imin(kMaxLoop, D - 6); // u1 + u2 <= m
        const int bi1 = s[i + 1], bj1 = s[j - 1];
        const int kr1 = j - delta;
        unsigned long long col_nz = 0, col_big = 0; // bit = q - (j - 1 - m)
        unsigned row_nz = 0, row_big = 0;           // bit = u1
        const int nslots = 1 + (m + 1) / 2;         // (0), (1, m), (2, m - 1), ... (see biloop_classify)
        for (int s0 = 0; s0 < nslots; s0 += 2) {
          const int half = lane >> 5, l5 = lane & 31;
          const int slot = s0 + half;
          const int ra_ = slot, rb_ = slot == 0 ? -1 : m + 1 - slot;
          const int na = slot < nslots ? m - ra_ + 1 : 0, nb = (slot < nslots && rb_ > ra_) ? m - rb_ + 1 : 0;
          const bool in_a = l5 < na, in_b = !in_a && l5 < na + nb;
          const int u1 = in_a ? ra_ : rb_, t5 = in_a ? l5 : l5 - na;
          const int u2 = (m - u1) - t5;
          const bool in = (in_a || in_b) && !(u1 == 0 && u2 == 0);
          const int pp = in ? i + 1 + u1 : i + 1, q = in ? j - 1 - u2 : j - 1;
          const int type2raw = ra_bp(lds, s[pp], s[q]);
          const double as = EM(a_stem, pp - 1, q);
          const double z = ra_loop_energy_bf(lds, c.big, type, ra_rtype(type2raw), in ? u1 : 0, in ? u2 : 0, bi1, bj1, s[pp - 1], s[q + 1]);
          const double e = bs + z + as;
          const bool ok = in && type2raw != 0 && as != kNegInf;
          const bool nz = ok && e > -708.39641853226408; // ra_expd(e) != 0
          const bool big = ok && e >= 89.0;
          const unsigned long long nzall = __ballot(nz);
          if (nzall == 0) continue;
          const unsigned long long bigall = __ballot(big);
#pragma unroll
          for (int h = 0; h < 2; h++) { // (wave-uniform: scalar instructions)
            const int sl = s0 + h;
            if (sl >= nslots) continue;
            const int a_ = sl, b_ = sl == 0 ? -1 : m + 1 - sl;
            const int n_a = m - a_ + 1, n_b = b_ > a_ ? m - b_ + 1 : 0;
            const unsigned hn = (unsigned)(nzall >> (32 * h)), hb = (unsigned)(bigall >> (32 * h));
            const unsigned an = hn & ((n_a >= 32 ? 0u : (1u << n_a)) - 1u), ab = hb & ((n_a >= 32 ? 0u : (1u << n_a)) - 1u);
            col_nz |= (unsigned long long)an << a_;
            col_big |= (unsigned long long)ab << a_;
            row_nz |= (an != 0 ? 1u : 0u) << a_;
            row_big |= (ab != 0 ? 1u : 0u) << a_;
            if (n_b > 0) {
              const unsigned bn = (hn >> n_a) & ((1u << n_b) - 1u), bb = (hb >> n_a) & ((1u << n_b) - 1u);
              col_nz |= (unsigned long long)bn << b_;
              col_big |= (unsigned long long)bb << b_;
              row_nz |= (bn != 0 ? 1u : 0u) << b_;
              row_big |= (bb != 0 ? 1u : 0u) << b_;
            }
          }
        }
        if (row_nz == 0) continue;
        // this lane's position: left ranges [i + 1, i + 1 + u1 - delta], right ranges [q + 1, j - delta]
        const int qbase = j - 1 - m;
        unsigned add = 0;
        if (k >= i + 1) {
          const int ustar = k - (i + 1 - delta); // the row whose left range ends at k
          if (ustar >= 0 && ustar <= m) {
            if ((row_nz >> ustar) & 1) add |= 2u | (((row_big >> ustar) & 1) ? 1u : 0u);
          }
          if (ustar < m) { // rows above: k lies inside their left ranges
            const int sh = ustar < 0 ? 0 : ustar + 1;
            if (row_nz >> sh) add |= 8u | ((row_big >> sh) ? 4u : 0u);
          }
        }
        if (k <= kr1) { // right ranges: the tuples with q <= k - 1
          const int nl = k - qbase;
          if (nl > 0) {
            const unsigned long long below = nl >= 64 ? ~0ull : ((1ull << nl) - 1);
            if (col_nz & below) add |= (k == kr1 ? 2u : 8u) | ((col_big & below) ? (k == kr1 ? 1u : 4u) : 0u);
          }
        }
        fl |= add;
      }
    }
  }
  const bool bbig = fl & 1, bnz = fl & 2, cbig = fl & 4, cnz = fl & 8;
  const bool undecided = k <= L && !((cbig || !cnz) && (cbig || bbig || !bnz));
  if (__ballot(undecided) != 0) return false;
  if (k <= L) {
    v.v(V_BP)[k - 1] = bnz ? __builtin_huge_val() : 0.0;
    v.v(V_CBP)[k - 1] = cnz ? __builtin_huge_val() : 0.0;
  }
  return true;
}

// The bulge / interior-loop sums by windows of 64 positions, a wavefront each.  RaBatch::windows_all: every sequence (a launch
// with few sequences: k_biloop is not launched at all); else only the sequences in the LOGSUM regime.
__global__ __launch_bounds__(kBlock) void k_biloop_win(RaBatch b, RaConst c) {
  __shared__ RaLds lds;
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.y;
  const SeqView v = make_view(b, idx);
  const int L = v.L;
  const double pf = v.v(V_AO)[L];
  const bool linear = pf >= -690 && pf <= 690; // raccess.cpp:500-507
  // (both tests are the same for every thread of the workgroup: nobody is left waiting at the barrier of the table load)
  if (linear && !b.windows_all) return; // the linear branch of this launch: k_biloop
  if (1 + kWave * (int)(blockIdx.x * kWavesPerBlock) > L) return;
  ra_load_lds(lds, c);
  const int k0 = 1 + kWave * (blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (k0 > L) return;
  if (!linear) {
    biloop_window<true>(lds, c, v, b.delta, lane, k0);
  } else if (pf < 120.0 || !biloop_classify_window(lds, c, v, b.delta, lane, k0)) {
    biloop_window<false>(lds, c, v, b.delta, lane, k0);
  }
}

template <int NS>
__global__ __launch_bounds__(kBlock) void k_biloop(RaBatch b, RaConst c) {
  __shared__ RaLds lds;
  ra_load_lds(lds, c);
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (idx >= b.nseq) return;
  const SeqView v = make_view(b, idx);
  const double pf = v.v(V_AO)[v.L];
  if (pf >= -690 && pf <= 690) { // raccess.cpp:500-507
    // large log Z: nearly always decided by the classification alone
    if (pf < 120.0 || !biloop_classify<NS>(lds, c, v, b.delta, lane)) biloop_run<false, NS>(lds, c, v, b.delta, lane);
  } else if (b.logsum_windows == 0) { // (else: k_biloop_logsum, a wavefront per window of 64 positions)
    biloop_run<true, NS>(lds, c, v, b.delta, lane);
  }
}

} // namespace

// k_biloop, a wavefront per sequence (not when the windows take every sequence), then k_biloop_win, a wavefront per window
void ra_launch_biloop(const RaBatch &b, const RaConst &c, hipStream_t stream) {
  const int blocks = (b.nseq + kWavesPerBlock - 1) / kWavesPerBlock;
  if (!(b.windows_all && b.logsum_windows > 0)) {
    if (ra_form(b).np == 4) hipLaunchKernelGGL(k_biloop<4>, dim3(blocks), dim3(kBlock), 0, stream, b, c);
    else hipLaunchKernelGGL(k_biloop<2>, dim3(blocks), dim3(kBlock), 0, stream, b, c);
  }
  if (b.logsum_windows > 0) {
    const int wblocks = (b.logsum_windows + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(k_biloop_win, dim3(wblocks, b.nseq), dim3(kBlock), 0, stream, b, c);
  }
}

} // namespace prb
