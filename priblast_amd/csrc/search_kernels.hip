// Interaction search on gfx950: seed expansion, ungapped extension, sort keys, the
// order-exact redundancy filter, gapped extension and traceback.
//
//   k_seed_count/emit <-> SeedSearch::CalcInteractionEnergy, GetSeqIdAndStart  seed_search.cpp:47-151
//   k_ungapped        <-> UngappedExtension::Run / LoopEnergy                   ungapped_extension.cpp:30-186
//   k_filter_*        <-> CheckRedundancy                                       rna_interaction_search.cpp:387-424
//   (gapped extension: gapped_lds.hip)
//
// All of this is HBM/L2-bound gather work on small integer tables; there is no dense
// contraction in it.  Energies are doubles built from exact multiples of 0.01 and
// float-derived accessibilities, summed in the reference's order (-ffp-contract=off).
#include "search_kernels.hpp"

#include <cstdlib>

#include "../../include/priblast_hip.h"

#include "search_device.hpp"

namespace prb {

namespace {

constexpr int kBlock = 256;

// id with start_pos[id] <= sp < start_pos[id+1]  (GetSeqIdAndStart, seed_search.cpp:101-141)
__device__ __forceinline__ int seq_of(const PageDev &pg, int sp) {
  int lo = 0, hi = pg.nseq - 1;
  while (lo < hi) {
    int m = (lo + hi + 1) >> 1;
    if (pg.start_pos[m] <= sp) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// SeedSearch::CalcAccessibility, seed_search.cpp:143-151
__device__ __forceinline__ double window_acc(const float *acc, const float *cond, int64_t sp, int length, int delta) {
  double t = acc[sp];
  for (int i = delta; i < length; i++) t += cond[sp + i];
  return t;
}

__device__ __forceinline__ int find_cand(const CandDev *c, int n, int64_t row) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    int m = (lo + hi + 1) >> 1;
    if (c[m].row0 <= row) lo = m;
    else hi = m - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_sa_seq(PageDev pg, int32_t *sa_seq) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < pg.nchars) sa_seq[k] = seq_of(pg, pg.sa[k]);
}

// Query-side window sums (SeedSearch::CalcAccessibility): one per (candidate, query SA entry),
// shared by all the database entries of the candidate.
__global__ __launch_bounds__(kBlock) void k_seed_qacc(const CandDev *__restrict__ cands, int ncand, int64_t n, QBatchDev qb, int delta,
                                                      double *__restrict__ qacc) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  int lo = 0, hi = ncand - 1; // candidate with qoff <= e
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (cands[m].qoff <= e) lo = m;
    else hi = m - 1;
  }
  const CandDev c = cands[lo];
  const int64_t qo = qb.off[c.query];
  const int q_sp = qb.sa[qo + c.sp_q + (int)(e - c.qoff)];
  qacc[e] = window_acc(qb.acc + qo, qb.cond + qo, q_sp, c.length, delta);
}

// One row = one (candidate, db SA entry); the query interval is walked inside the row.  The
// count pass finds the row's candidate - a workgroup's 256 rows span at most 256 candidates,
// whose first rows are put in LDS - and leaves it for the emit pass.
// With `row_perm` the threads take the rows in that order (rows sorted by query and database position, see
// k_row_key): thread t works on row row_perm[t], whose candidate k_row_key has left in row_cand; counts and offsets
// are indexed by t.
template <bool kEmit>
__global__ __launch_bounds__(kBlock) void k_seed(const CandDev *__restrict__ cands, int ncand, int64_t nrows, QBatchDev qb,
                                                 PageDev pg, int delta, const double *__restrict__ qacc,
                                                 int32_t *__restrict__ row_count, int32_t *__restrict__ row_cand,
                                                 const int64_t *__restrict__ row_off, HitSoA hits,
                                                 const uint32_t *__restrict__ row_perm) {
  __shared__ int64_t s_row0[kBlock + 1];
  __shared__ int s_c0;
  const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x; // index of the row's count / offset
  int64_t row = slot;
  int ci;
  if (kEmit || row_perm) {
    if (slot >= nrows) return;
    if (row_perm) row = row_perm[slot];
    ci = row_cand[row];
  } else {
    if (threadIdx.x == 0) s_c0 = find_cand(cands, ncand, (int64_t)blockIdx.x * kBlock);
    __syncthreads();
    const int c0 = s_c0;
    for (int t = threadIdx.x; t <= kBlock; t += kBlock) s_row0[t] = c0 + t < ncand ? cands[c0 + t].row0 : INT64_MAX;
    __syncthreads();
    if (row >= nrows) return;
    int lo = 0, hi = kBlock; // last t with s_row0[t] <= row
    while (lo < hi) {
      const int m = (lo + hi + 1) >> 1;
      if (s_row0[m] <= row) lo = m;
      else hi = m - 1;
    }
    ci = c0 + lo;
    row_cand[row] = ci;
  }
  const CandDev c = cands[ci];
  const int k = c.sp_db + (int)(row - c.row0);
  const int db_sp = pg.sa[k];
  const int id = pg.sa_seq[k];
  const int st = pg.seq_length[id] - (db_sp - pg.start_pos[id]) - c.length;
  const int64_t base = (int64_t)pg.start_pos[id] - id;
  const double dba = window_acc(pg.acc + base, pg.cond + base, st, c.length, delta);
  const int32_t *qsa = qb.sa + qb.off[c.query];
  const double *qa_c = qacc + c.qoff - c.sp_q;
  int cnt = 0;
  int64_t w = kEmit ? row_off[slot] : 0;
  for (int j = c.sp_q; j <= c.ep_q; j++) {
    const double qa = qa_c[j];
    const double ie = qa + dba + c.score;
    if (ie < 0) {
      if (kEmit) {
        hits.q_sp[w] = qsa[j];
        hits.db_sp[w] = db_sp;
        hits.q_len[w] = c.length;
        hits.db_len[w] = c.length;
        hits.db_id[w] = id;
        hits.db_id_start[w] = st;
        hits.query[w] = c.query;
        const double ea = qa + dba;
        hits.e_acc[w] = ea;
        hits.e_hyb[w] = c.score;
        hits.e_tot[w] = ea + c.score;
        w++;
      }
      cnt++;
    }
  }
  if (!kEmit) row_count[slot] = cnt;
}

// Sort key of a row = (query, position in the page text): the rows of a candidate are consecutive entries of the
// suffix array, i.e. RANDOM positions of the database, and a seed's extension reads ~5 cache lines around its
// position - at the configs[2] database (0.9 GB of text + accessibilities) every one of them from HBM (measured:
// 377 B fetched per seed in k_ungapped, 105 B in each k_seed pass).  Emitting the seeds of a query in the order of
// their database positions makes neighbouring threads read neighbouring lines.  The low `shift` bits of the position
// are left out of the key (fewer radix passes): rows of one 2^shift window stay in suffix-array order, which is all
// the same to the caches.  The order of the seeds is free: the list is sorted by coordinates afterwards and the ties of
// that sort are broken by the hits' own fields (k_fix_ties).
template <class Key>
__global__ __launch_bounds__(kBlock) void k_row_key(const CandDev *__restrict__ cands, int ncand, int64_t nrows, PageDev pg, int qmin,
                                                    int shift, int dbits, int32_t *__restrict__ row_cand, Key *__restrict__ key,
                                                    uint32_t *__restrict__ val) {
  __shared__ int64_t s_row0[kBlock + 1];
  __shared__ int s_c0;
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (threadIdx.x == 0) s_c0 = find_cand(cands, ncand, (int64_t)blockIdx.x * kBlock);
  __syncthreads();
  const int c0 = s_c0;
  for (int t = threadIdx.x; t <= kBlock; t += kBlock) s_row0[t] = c0 + t < ncand ? cands[c0 + t].row0 : INT64_MAX;
  __syncthreads();
  if (row >= nrows) return;
  int lo = 0, hi = kBlock; // last t with s_row0[t] <= row
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (s_row0[m] <= row) lo = m;
    else hi = m - 1;
  }
  const int ci = c0 + lo;
  row_cand[row] = ci;
  const CandDev c = cands[ci];
  const int k = c.sp_db + (int)(row - c.row0);
  key[row] = ((Key)(uint32_t)(c.query - qmin) << dbits) | (Key)((uint32_t)pg.sa[k] >> shift);
  val[row] = (uint32_t)row;
}

// ---------------------------------------------------------------------------- ungapped
// symmetric interior loops only: stack / 1x1 / 2x2 / generic without asymmetry term
// (UngappedExtension::LoopEnergy, ungapped_extension.cpp:157-186)
__device__ __forceinline__ double loop_energy_ungapped(const SearchConst &sc, int type, int type2, int i, int j, int p,
                                                       int q, const uint8_t *qs, const uint8_t *ds) {
  const int u1 = p - i - 1, u2 = q - j - 1;
  int z;
  if (u1 == 0 && u2 == 0) {
    z = sc.stack37[type * 7 + type2];
  } else {
    const int a = base_of(qs[i + 1]), b = base_of(ds[j + 1]), c = base_of(qs[p - 1]), d = base_of(ds[q - 1]);
    if (u1 + u2 == 2) z = sc.int11[((type * 8 + type2) * 5 + a) * 5 + b];
    else if (u1 == 1 && u2 == 2) z = sc.int21[(((type * 8 + type2) * 5 + a) * 5 + d) * 5 + b];
    else if (u1 == 2 && u2 == 1) z = sc.int21[(((type2 * 8 + type) * 5 + d) * 5 + a) * 5 + c];
    else if (u1 == 2 && u2 == 2) z = sc.int22[((((type * 8 + type2) * 5 + a) * 5 + c) * 5 + d) * 5 + b];
    else z = sc.internal37[u1 + u2] + sc.mismatchI37[(type * 5 + a) * 5 + b] + sc.mismatchI37[(type2 * 5 + d) * 5 + c];
  }
  return div100(sc, z);
}

// The tables UngappedExtension::LoopEnergy reads: all but the 2x2 table (160 KB, one pair in ten)
// are staged in LDS by the workgroup.
struct UngappedTabs {
  const int32_t *stack37, *internal37, *mismatchI37, *int11; // LDS
  const int32_t *int22;                                        // HBM / L2
};
constexpr int kUtStack = 0, kUtInternal = 49, kUtMismatch = 49 + 31, kUtInt11 = 49 + 31 + 175, kUtTotal = 49 + 31 + 175 + 1600;

// UngappedExtension::LoopEnergy (ungapped_extension.cpp:157-186) on values the walk already holds:
// the loop between the pairs (type, type2) is symmetric, u unpaired bases per strand; a, b = the
// bases next to the first pair (query, db), c, d = next to the second one.
__device__ __forceinline__ double loop_energy_ungapped_abcd(const SearchConst &sc, const UngappedTabs &t, int type, int type2,
                                                           int u, int a, int b, int c, int d) {
  int z;
  if (u == 0) z = t.stack37[type * 7 + type2];
  else if (u == 1) z = t.int11[((type * 8 + type2) * 5 + a) * 5 + b];
  else if (u == 2) z = t.int22[((((type * 8 + type2) * 5 + a) * 5 + c) * 5 + d) * 5 + b];
  else z = t.internal37[2 * u] + t.mismatchI37[(type * 5 + a) * 5 + b] + t.mismatchI37[(type2 * 5 + d) * 5 + c];
  return div100(sc, z);
}

// The query side of a walk: in HBM, or staged in LDS by the workgroup.
struct QueryGlobal {
  const uint8_t *qs;
  const float *qacc, *qcond;
  __device__ __forceinline__ unsigned enc(int i) const { return qs[i]; }
  __device__ __forceinline__ float acc(int i) const { return qacc[i]; }
  __device__ __forceinline__ float cond(int i) const { return qcond[i]; }
};
struct QueryLds {
  const uint8_t *qs; // derived from the kernel's __shared__ block
  const float *qacc, *qcond;
  __device__ __forceinline__ unsigned enc(int i) const { return qs[i]; }
  __device__ __forceinline__ float acc(int i) const { return qacc[i]; }
  __device__ __forceinline__ float cond(int i) const { return qcond[i]; }
};

// One seed hit (UngappedExtension::Run, ungapped_extension.cpp:30-155).  A walk is a chain of
// data-dependent steps, and what it costs is memory latency, not arithmetic (PMC: VALU 16 % busy,
// ~400 ns per load, all exposed).  So: the query side and the small energy tables come from LDS;
// the database side of the next kUngappedAhead positions is fetched at once, speculatively
// (clamped to the arrays; a walk that stops earlier just drops the values); and everything a step
// needs again later is carried in registers - the accessibility of the previous position, the
// bases of the previous position and of the position next to the last pair, the type of the
// last pair (the reference re-reads all of them).
// a hit in registers: the seed on the way in, the extended hit on the way out
struct WalkHit {
  int q_sp, db_sp, len, id, id_start;
  double e_acc, e_hyb, e_tot;
};
template <int kUngappedAhead, class Q>
__device__ __forceinline__ void ungapped_walk_reg(const Q &qv, const UngappedTabs &tabs, WalkHit &w, const PageDev &pg,
                                              const SearchConst &sc, const ExtOpts &o) {
  const uint8_t *ds = pg.seqs;
  const int id = w.id;
  const int64_t base = (int64_t)pg.start_pos[id] - id;
  const int64_t nacc = (int64_t)pg.nchars - pg.nseq; // floats in pg.acc / pg.cond
  const int delta = o.delta, drop = o.drop_wo_gap;
  const int q_sp0 = w.q_sp, db_sp0 = w.db_sp, len0 = w.len;

  double min_e = w.e_tot, e = min_e, min_a = w.e_acc, a = min_a, min_h = w.e_hyb, hy = min_h;
  int i = q_sp0, p = q_sp0, j = db_sp0, min_p = p, min_q = db_sp0;
  int id_start = w.id_start, id_end = id_start + len0 - 1, min_id_start = id_start;
  {
    // walk left (:55-94).  (bq, bd) = bases at (i+1, j+1); (cq, cd) = bases at (p-1, q-1), the
    // position next to the last pair; tp = rtype of the pair at (p, q)
    int bq = base_of(qv.enc(i)), bd = base_of(ds[j]);
    int tp = rtype_of(bp_type(sc, bq, bd));
    int cq = 0, cd = 0;
    float acc_next = qv.acc(i); // qacc[i + 1] of the step to come
    bool done = false;
    while (!done) {
      unsigned dcs[kUngappedAhead];
      float dcn[kUngappedAhead];
#pragma unroll
      for (int s = 0; s < kUngappedAhead; s++) {
        const int jj = j - 1 - s;
        dcs[s] = jj >= 0 ? ds[jj] : 0u;
        int64_t ci = base + id_end + 1 + s;
        ci = ci < nacc ? ci : nacc - 1;
        dcn[s] = pg.cond[ci];
      }
#pragma unroll
      for (int s = 0; s < kUngappedAhead; s++) {
        if (done) continue;
        i--;
        j--;
        id_end++;
        if (i < 0 || j < 0) {
          done = true;
          continue;
        }
        const unsigned qc = qv.enc(i), dc = dcs[s];
        if (qc < 2 || dc < 2) {
          done = true;
          continue;
        }
        const float acc_i = qv.acc(i);
        const double ta = acc_i - acc_next + qv.cond(i + delta) + dcn[s]; // float arithmetic, as the reference
        acc_next = acc_i;
        e += ta;
        a += ta;
        const int nq = base_of(qc), nd = base_of(dc);
        if (i == p - 1) {
          cq = nq;
          cd = nd;
        }
        const int type = bp_type(sc, nq, nd);
        if (type != 0) {
          const double le = loop_energy_ungapped_abcd(sc, tabs, type, tp, p - i - 1, bq, bd, cq, cd);
          e += le;
          hy += le;
          if (e < min_e) {
            min_e = e;
            min_a = a;
            min_h = hy;
            min_p = i;
            min_q = j;
          }
          p = i;
          tp = rtype_of(type);
        }
        bq = nq;
        bd = nd;
        if (min_p - i >= drop) done = true;
      }
    }
  }
  e = min_e;
  a = min_a;
  hy = min_h;
  int k = q_sp0 + len0 - 1, r = k, l = db_sp0 + len0 - 1, min_r = r;
  {
    // walk right (:96-145).  (bq, bd) = bases at (k-1, l-1); (cq, cd) = bases at (r+1, s+1); tr = type
    // of the pair at (r, s)
    int bq = base_of(qv.enc(k)), bd = base_of(ds[l]);
    int tr = bp_type(sc, bq, bd);
    int cq = 0, cd = 0;
    float acc_prev = pg.acc[base + id_start]; // dacc[id_start + 1] of the step to come
    bool done = false;
    while (!done) {
      unsigned dcs[kUngappedAhead];
      float dan[kUngappedAhead], dcn[kUngappedAhead];
#pragma unroll
      for (int s = 0; s < kUngappedAhead; s++) {
        const int ll = l + 1 + s;
        dcs[s] = ll < pg.nchars ? ds[ll] : 0u;
        int64_t ai = base + id_start - 1 - s;
        ai = ai > 0 ? ai : 0;
        int64_t ci = ai + delta;
        ci = ci < nacc ? ci : nacc - 1;
        dan[s] = pg.acc[ai];
        dcn[s] = pg.cond[ci];
      }
#pragma unroll
      for (int s = 0; s < kUngappedAhead; s++) {
        if (done) continue;
        k++;
        l++;
        id_start--;
        const unsigned qc = qv.enc(k), dc = dcs[s];
        if (qc < 2 || dc < 2) {
          done = true;
          continue;
        }
        const float acc_i = dan[s];
        const double ta = qv.cond(k) + acc_i - acc_prev + dcn[s];
        acc_prev = acc_i;
        e += ta;
        a += ta;
        const int nq = base_of(qc), nd = base_of(dc);
        if (k == r + 1) {
          cq = nq;
          cd = nd;
        }
        const int type2 = rtype_of(bp_type(sc, nq, nd));
        if (type2 != 0) {
          // loop between (r, s) and (k, l): a, b next to the first pair, c, d next to the second
          const double le = loop_energy_ungapped_abcd(sc, tabs, tr, type2, k - r - 1, cq, cd, bq, bd);
          e += le;
          hy += le;
          if (e < min_e) {
            min_e = e;
            min_a = a;
            min_h = hy;
            min_r = k;
            min_id_start = id_start;
          }
          r = k;
          tr = rtype_of(type2);
        }
        bq = nq;
        bd = nd;
        if (k - min_r >= drop) done = true;
      }
    }
  }
  w.id_start = min_id_start;
  w.q_sp = min_p;
  w.db_sp = min_q;
  w.len = min_r - min_p + 1;
  w.e_tot = min_e;
  w.e_acc = min_a;
  w.e_hyb = min_h;
}
// the same on a hit of a list
template <class Q>
__device__ __forceinline__ void ungapped_walk(const Q &qv, const UngappedTabs &tabs, HitSoA &h, int64_t x, const PageDev &pg,
                                              const SearchConst &sc, const ExtOpts &o) {
  WalkHit w{h.q_sp[x], h.db_sp[x], h.q_len[x], h.db_id[x], h.db_id_start[x], h.e_acc[x], h.e_hyb[x], h.e_tot[x]};
  ungapped_walk_reg<8>(qv, tabs, w, pg, sc, o);
  h.db_id_start[x] = w.id_start;
  h.q_sp[x] = w.q_sp;
  h.db_sp[x] = w.db_sp;
  h.q_len[x] = w.len;
  h.db_len[x] = w.len;
  h.e_tot[x] = w.e_tot;
  h.e_acc[x] = w.e_acc;
  h.e_hyb[x] = w.e_hyb;
}

// A workgroup takes kUngappedPer x kBlock consecutive seed hits.  Seed hits are emitted query
// by query, and the 64 lanes of a wave sit at 64 unrelated positions of that query (its suffix-array
// interval) but at one position of the database.  When all hits of the workgroup belong to one
// query (all but the few workgroups at query boundaries), the query's codes and accessibilities
// (9 B per nucleotide) are staged in LDS; queries longer than the launch's LDS capacity take the
// HBM path.
constexpr int kUngappedPer = 8;
__global__ __launch_bounds__(kBlock) void k_ungapped(HitSoA h, int64_t n, QBatchDev qb, PageDev pg, SearchConst sc, ExtOpts o,
                                                     int qcap) {
  extern __shared__ __align__(16) uint8_t ungapped_smem[];
  __shared__ int32_t s_tab[kUtTotal];
  const int64_t b0 = (int64_t)blockIdx.x * (kBlock * kUngappedPer);
  if (b0 >= n) return;
  const int64_t b1 = (b0 + kBlock * kUngappedPer < n ? b0 + kBlock * kUngappedPer : n) - 1;
  for (int t = threadIdx.x; t < kUtTotal; t += kBlock)
    s_tab[t] = t < kUtInternal   ? sc.stack37[t]
               : t < kUtMismatch ? sc.internal37[t - kUtInternal]
               : t < kUtInt11    ? sc.mismatchI37[t - kUtMismatch]
                                 : sc.int11[t - kUtInt11];
  const UngappedTabs tabs{s_tab + kUtStack, s_tab + kUtInternal, s_tab + kUtMismatch, s_tab + kUtInt11, sc.int22};
  const int q0 = h.query[b0];
  const int nslots = qb.len[q0] + 1;
  const bool staged = q0 == h.query[b1] && nslots <= qcap; // uniform over the workgroup
  if (staged) {
    float *s_acc = reinterpret_cast<float *>(ungapped_smem), *s_cond = s_acc + qcap;
    uint8_t *s_enc = reinterpret_cast<uint8_t *>(s_cond + qcap);
    const int64_t qo = qb.off[q0];
    for (int t = threadIdx.x; t < nslots; t += kBlock) {
      s_acc[t] = qb.acc[qo + t];
      s_cond[t] = qb.cond[qo + t];
      s_enc[t] = qb.enc[qo + t];
    }
    __syncthreads();
    const QueryLds qv{s_enc, s_acc, s_cond};
    for (int64_t x = b0 + threadIdx.x; x <= b1; x += kBlock) ungapped_walk(qv, tabs, h, x, pg, sc, o);
  } else {
    __syncthreads();
    for (int64_t x = b0 + threadIdx.x; x <= b1; x += kBlock) {
      const int64_t qo = qb.off[h.query[x]];
      const QueryGlobal qv{qb.enc + qo, qb.acc + qo, qb.cond + qo};
      ungapped_walk(qv, tabs, h, x, pg, sc, o);
    }
  }
}

// ---------------------------------------------------------------------------- seeds -> extended hits in one pass
// Every (query SA entry, database SA entry) PAIR of a chunk of candidates is one unit of work:
//   k_pair_key    pair p -> sort key (query, database position >> shift) and a 64-bit value
//                 {database position : 32, candidate : 20, query entry within the candidate : 12}
//   (radix sort of the pairs by key)
//   k_seed_extend pair -> SeedSearch::CalcInteractionEnergy's test (seed_search.cpp:47-99); a seed is walked at once
//                 (UngappedExtension::Run) and, if it is not above the -f threshold, kept (see SliceRec)
//   k_collect_slices  what the workgroups kept -> the list of 64-byte records
// Against k_seed (count) / scan / k_seed (emit) / k_ungapped / threshold compaction this never writes the seeds
// (3.3e9 x 48 B per configs[2] step, written once, read and written by the walk, read by the compaction), and
// neighbouring threads work at neighbouring database positions.  The list comes out in no particular order; the sort
// behind it is total on the hits' own fields (k_fix_ties), so the result is the same.
constexpr int kPairCandBits = 20, kPairEntBits = 12;
static_assert(kMaxFusedCands == (1 << kPairCandBits) && kMaxFusedEntries == (1 << kPairEntBits) && kPairCandBits + kPairEntBits == 32,
              "the value of a pair");
constexpr int kSeqBlkShift = 5; // PageDev::blk_seq: one entry per 32 characters of the page text

__global__ __launch_bounds__(kBlock) void k_blk_seq(PageDev pg, int32_t *blk_seq, int64_t nblk) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b < nblk) blk_seq[b] = seq_of(pg, (int)(b << kSeqBlkShift));
}

template <class Key>
__global__ __launch_bounds__(kBlock) void k_pair_key(const CandDev *__restrict__ cands, const int64_t *__restrict__ pair0, int ncand,
                                                     int64_t npairs, PageDev pg, int qmin, int shift, int dbits,
                                                     Key *__restrict__ key, uint64_t *__restrict__ val) {
  __shared__ int64_t s_p0[kBlock + 1];
  __shared__ int s_c0;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (threadIdx.x == 0) { // candidate of the workgroup's first pair
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    int lo = 0, hi = ncand - 1;
    while (lo < hi) {
      const int m = (lo + hi + 1) >> 1;
      if (pair0[m] <= first) lo = m;
      else hi = m - 1;
    }
    s_c0 = lo;
  }
  __syncthreads();
  const int c0 = s_c0;
  for (int t = threadIdx.x; t <= kBlock; t += kBlock) s_p0[t] = c0 + t < ncand ? pair0[c0 + t] : INT64_MAX;
  __syncthreads();
  if (p >= npairs) return;
  int lo = 0, hi = kBlock; // last t with s_p0[t] <= p
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (s_p0[m] <= p) lo = m;
    else hi = m - 1;
  }
  const int ci = c0 + lo;
  const CandDev c = cands[ci];
  const uint32_t pl = (uint32_t)(p - s_p0[lo]), qw = (uint32_t)(c.ep_q - c.sp_q + 1);
  const uint32_t rowl = pl / qw, jrel = pl - rowl * qw;
  const uint32_t db_sp = (uint32_t)pg.sa[c.sp_db + (int)rowl];
  key[p] = ((Key)(uint32_t)(c.query - qmin) << dbits) | (Key)(db_sp >> shift);
  val[p] = (uint64_t)db_sp | ((uint64_t)(uint32_t)ci << 32) | ((uint64_t)jrel << (32 + kPairCandBits));
}

// What a workgroup keeps goes to ITS slice of a sparse list (kFusePairs records, one per pair it takes: no bound to
// check), the position from a counter in LDS; k_collect_slices then packs the used part of every slice into the list
// proper.  (One global counter for all wavefronts - an atomic add with return per 64 pairs - serialised the whole
// kernel: 844 ms per configs[2] step instead of 300, ~14 ns per atomic on one address.)
struct alignas(16) SliceRec {
  int32_t q_sp, db_sp, len, db_id, db_id_start, query;
  double e_acc, e_hyb, e_tot;
};
static_assert(sizeof(SliceRec) == kSliceRecBytes, "three 16-byte stores");

struct FuseArgs {
  const CandDev *cands;
  const uint64_t *vals;
  int64_t npairs;
  const double *qacc;
  double thr;
  SliceRec *slices;        // kFusePairs per workgroup
  int32_t *slice_count;    // records in each slice
  unsigned long long *nseed; // [0] += seeds, [1] = max(., length of the longest hit kept)
  int qcap;
};

__device__ __forceinline__ int pair_cand(uint64_t v) { return (int)((v >> 32) & ((1u << kPairCandBits) - 1)); }

constexpr int kFusePer = kFusePairs / kBlock;
static_assert(kFusePer * kBlock == kFusePairs, "pairs per workgroup");
template <int kAhead>
__global__ __launch_bounds__(kBlock) void k_seed_extend(FuseArgs f, QBatchDev qb, PageDev pg, SearchConst sc, ExtOpts o) {
  extern __shared__ __align__(16) uint8_t ungapped_smem[];
  __shared__ int32_t s_tab[kUtTotal];
  __shared__ unsigned s_kept, s_seeds, s_maxlen;
  const int64_t b0 = (int64_t)blockIdx.x * kFusePairs;
  if (b0 >= f.npairs) return;
  const int64_t b1 = (b0 + kFusePairs < f.npairs ? b0 + kFusePairs : f.npairs) - 1;
  if (threadIdx.x == 0) {
    s_kept = 0;
    s_seeds = 0;
    s_maxlen = 0;
  }
  for (int t = threadIdx.x; t < kUtTotal; t += kBlock)
    s_tab[t] = t < kUtInternal   ? sc.stack37[t]
               : t < kUtMismatch ? sc.internal37[t - kUtInternal]
               : t < kUtInt11    ? sc.mismatchI37[t - kUtMismatch]
                                 : sc.int11[t - kUtInt11];
  const UngappedTabs tabs{s_tab + kUtStack, s_tab + kUtInternal, s_tab + kUtMismatch, s_tab + kUtInt11, sc.int22};
  // the pairs are sorted by query first: one query for the whole workgroup unless it sits on a boundary
  const int q0 = f.cands[pair_cand(f.vals[b0])].query;
  const int nslots = qb.len[q0] + 1;
  const bool staged = q0 == f.cands[pair_cand(f.vals[b1])].query && nslots <= f.qcap; // uniform over the workgroup
  float *s_acc = reinterpret_cast<float *>(ungapped_smem), *s_cond = s_acc + f.qcap;
  uint8_t *s_enc = reinterpret_cast<uint8_t *>(s_cond + f.qcap);
  if (staged) {
    const int64_t qo = qb.off[q0];
    for (int t = threadIdx.x; t < nslots; t += kBlock) {
      s_acc[t] = qb.acc[qo + t];
      s_cond[t] = qb.cond[qo + t];
      s_enc[t] = qb.enc[qo + t];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  SliceRec *slice = f.slices + b0;
  unsigned nseed = 0, maxlen = 0; // (the longest hit kept: the sort behind this packs the lengths into as many bits)
  for (int it = 0; it < kFusePer; it++) {
    const int64_t x = b0 + (int64_t)it * kBlock + threadIdx.x;
    bool keep = false;
    WalkHit w{};
    int query = 0;
    if (x <= b1) {
      const uint64_t v = f.vals[x];
      const int db_sp = (int)(uint32_t)v, jrel = (int)(v >> (32 + kPairCandBits));
      const CandDev c = f.cands[pair_cand(v)];
      int id = pg.blk_seq[db_sp >> kSeqBlkShift];
      while (id + 1 < pg.nseq && pg.start_pos[id + 1] <= db_sp) id++;
      const int sp0 = pg.start_pos[id];
      const int st = pg.seq_length[id] - (db_sp - sp0) - c.length;
      const int64_t base = (int64_t)sp0 - id;
      const double dba = window_acc(pg.acc + base, pg.cond + base, st, c.length, o.delta);
      const double qa = f.qacc[c.qoff + jrel];
      const double ie = qa + dba + c.score;
      if (ie < 0) {
        nseed++;
        const int64_t qo = qb.off[c.query];
        const double ea = qa + dba;
        w = WalkHit{qb.sa[qo + c.sp_q + jrel], db_sp, c.length, id, st, ea, c.score, ea + c.score};
        query = c.query;
        if (staged) {
          const QueryLds qv{s_enc, s_acc, s_cond};
          ungapped_walk_reg<kAhead>(qv, tabs, w, pg, sc, o);
        } else {
          const QueryGlobal qv{qb.enc + qo, qb.acc + qo, qb.cond + qo};
          ungapped_walk_reg<kAhead>(qv, tabs, w, pg, sc, o);
        }
        keep = !(w.e_tot > f.thr);
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (mask) {
      const int leader = __ffsll((long long)mask) - 1;
      unsigned basepos = 0;
      if (lane == leader) basepos = atomicAdd(&s_kept, (unsigned)__popcll(mask));
      basepos = (unsigned)__shfl((int)basepos, leader);
      if (keep) {
        SliceRec r;
        r.q_sp = w.q_sp;
        r.db_sp = w.db_sp;
        r.len = w.len;
        r.db_id = w.id;
        r.db_id_start = w.id_start;
        r.query = query;
        r.e_acc = w.e_acc;
        r.e_hyb = w.e_hyb;
        r.e_tot = w.e_tot;
        slice[basepos + (unsigned)__popcll(mask & ((1ull << lane) - 1))] = r;
        maxlen = (unsigned)w.len > maxlen ? (unsigned)w.len : maxlen;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    nseed += (unsigned)__shfl_down((int)nseed, d);
    const unsigned o = (unsigned)__shfl_down((int)maxlen, d);
    maxlen = o > maxlen ? o : maxlen;
  }
  if (lane == 0 && nseed) atomicAdd(&s_seeds, nseed);
  if (lane == 0 && maxlen) atomicMax(&s_maxlen, maxlen);
  __syncthreads();
  if (threadIdx.x == 0) {
    f.slice_count[blockIdx.x] = (int32_t)s_kept;
    if (s_seeds) atomicAdd(f.nseed, (unsigned long long)s_seeds);
    if (s_maxlen) atomicMax(f.nseed + 1, (unsigned long long)s_maxlen);
  }
}

// slice b's records to out[off[b] ...]
__global__ __launch_bounds__(kBlock) void k_collect_slices(const SliceRec *__restrict__ slices, const int32_t *__restrict__ count,
                                                           const int64_t *__restrict__ off, HitRec *__restrict__ out) {
  const int n = count[blockIdx.x];
  const SliceRec *src = slices + (int64_t)blockIdx.x * kFusePairs;
  HitRec *dst = out + off[blockIdx.x];
  for (int t = threadIdx.x; t < n; t += kBlock) {
    const SliceRec a = src[t];
    HitRec r;
    r.q_sp = a.q_sp;
    r.db_sp = a.db_sp;
    r.q_len = a.len;
    r.db_len = a.len;
    r.db_id = a.db_id;
    r.db_id_start = a.db_id_start;
    r.query = a.query;
    r.pad0 = 0;
    r.e_acc = a.e_acc;
    r.e_hyb = a.e_hyb;
    r.e_tot = a.e_tot;
    r.pad1 = 0;
    dst[t] = r;
  }
}

// ------------------------------------------------------------------- sort keys / gather

__global__ __launch_bounds__(kBlock) void k_make_keys(HitSoA h, int64_t n, uint64_t *k_energy, uint32_t *k_len,
                                                      uint32_t *k_qsp, uint64_t *k_pos, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  // compare(): db_sp asc, q_sp asc, db_len desc, q_len desc (rna_interaction_search.cpp:45-55);
  // ties are then broken by energy asc, its two parts and input order (DESIGN.md "total order")
  const uint64_t eb = (uint64_t)__double_as_longlong(h.e_tot[i]);
  k_energy[i] = (eb >> 63) ? ~eb : (eb | 0x8000000000000000ull);
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
  const uint64_t eb = (uint64_t)__double_as_longlong(h.e_tot[i]);
  k_energy[i] = (eb >> 63) ? ~eb : (eb | 0x8000000000000000ull);
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
  const uint64_t eb = (uint64_t)__double_as_longlong(r.e_tot);
  k_energy[i] = (eb >> 63) ? ~eb : (eb | 0x8000000000000000ull);
  uint64_t k = (uint64_t)(uint32_t)(r.query - f.qmin);
  k = (k << f.bd) | (uint32_t)r.db_sp;
  k = (k << f.bq) | (uint32_t)r.q_sp;
  k = (k << f.bl) | (uint32_t)(f.lmax - US(r.db_len));
  if (!f.one_len) k = (k << f.bl) | (uint32_t)(f.lmax - US(r.q_len)); // (one_len: q_len = db_len in every hit of the list)
  key[i] = k;
  idx[i] = (uint32_t)i;
}

constexpr int kMaxTieRun = 4096;
// monotone map of a double onto unsigned integers
__device__ __forceinline__ uint64_t order_bits(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
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

// ---- per-pair summaries ----
// The final list is sorted by query, then db_sp, and a database sequence is one contiguous range of the page text
// (db_id = seq_of(db_sp)), so the hits of a (query, db_id) pair are one run of the list.
__global__ __launch_bounds__(kBlock) void k_pair_heads(const int32_t *__restrict__ query, const int32_t *__restrict__ db_id,
                                                       int64_t n, uint8_t *head) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  head[i] = i == 0 || query[i] != query[i - 1] || db_id[i] != db_id[i - 1];
}

// A lane walks its pair's run in list order: strict `<` keeps the first minimum, the sum is the left-to-right one.
// (A lane per pair: the skew of the run lengths is in DESIGN.md §4.)
__global__ __launch_bounds__(kBlock) void k_pair_fold(HitSoA h, int64_t n, const uint32_t *__restrict__ start, int64_t npairs,
                                                      const int32_t *__restrict__ ends, prb_pair_summary *out) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= npairs) return;
  const int64_t a = start[k], b = k + 1 < npairs ? (int64_t)start[k + 1] : n;
  double sum = 0.0, mn = h.e_tot[a];
  int64_t best = a;
  for (int64_t i = a; i < b; i++) {
    const double e = h.e_tot[i];
    sum += e;
    if (e < mn) {
      mn = e;
      best = i;
    }
  }
  prb_pair_summary r;
  r.query = h.query[a];
  r.db_id = h.db_id[a];
  r.hits = b - a;
  r.e_min = mn;
  r.e_sum = sum;
  r.e_acc = h.e_acc[best];
  r.e_hyb = h.e_hyb[best];
  r.bp_first[0] = ends[4 * best];
  r.bp_first[1] = ends[4 * best + 1];
  r.bp_last[0] = ends[4 * best + 2];
  r.bp_last[1] = ends[4 * best + 3];
  out[k] = r;
}

// ---- distinct interaction sites (prb_ris_opts::distinct_sites, `ris -u`) ----
// Greedy non-maximum suppression inside every (query, db_id) run of the final list (the rule: include/priblast_hip.h),
// in its fix-point form: a hit is kept once every intersecting hit before it in the order (e_tot, place) is dropped, and
// dropped once one of them is kept.  The first undecided hit of the order has only decided hits before it, so every
// round decides it at least: a run of L hits is done after at most L rounds, and every loop below has that bound.
// Decisions are final and never wrong whenever they are taken, so a round may read states that the same round writes.
__device__ __forceinline__ int4 site_rect(const HitSoA &h, int64_t i) { // inclusive ends: (q0, q1, db0, db1)
  const int q = h.q_sp[i], d = h.db_sp[i];
  return make_int4(q, q + h.q_len[i] - 1, d, d + h.db_len[i] - 1);
}
__device__ __forceinline__ bool site_intersect(const int4 &a, const int4 &b) {
  return a.x <= b.y && b.x <= a.y && a.z <= b.w && b.z <= a.w;
}
// hit j comes before hit i: e_tot ascending, compared as doubles (-0.0 == +0.0), then the place in the list
__device__ __forceinline__ bool site_before(double ej, int j, double ei, int i) { return ej < ei || (ej == ei && j < i); }

// Runs of up to 64 hits (fourteen on average, most of them one to thirty), several per wavefront: a wavefront (= a
// workgroup) owns the runs that start in its slice of 64 hits and lays 64 consecutive hits from the first of them over
// its lanes; a run that does not end inside that window opens a second one (two windows always reach the end of the
// slice's runs: whatever the second one leaves open starts behind the slice).  Per window: the run of each lane from
// the ballot of the head flags; if all runs are singletons nothing else happens; else rectangles and energies go
// through 1.5 KB of LDS once, every lane collects the mask of the lanes before it in the order that intersect it, and
// the rounds are three ballots and a few mask operations each.  Runs longer than short_max (<= 64) are appended to
// long_list for k_site_select_long.
__global__ __launch_bounds__(64) void k_site_select_packed(HitSoA h, int64_t n, const uint8_t *__restrict__ head, int short_max,
                                                           uint8_t *__restrict__ keep, uint32_t *__restrict__ long_list, uint32_t *nlong) {
  __shared__ int4 rect_s[64];
  __shared__ double key_s[64];
  const int lane = threadIdx.x;
  const int64_t slice0 = (int64_t)blockIdx.x * 64, slice1 = min(n, slice0 + 64);
  const uint64_t starts = __ballot(slice0 + lane < n && head[min(slice0 + lane, n - 1)] != 0);
  if (starts == 0) return; // (the slice lies inside a run that began before it)
  int64_t base = slice0 + __builtin_ctzll(starts);
  for (int pass = 0; pass < 2 && base < slice1; pass++) {
    const int wlen = (int)min((int64_t)64, n - base);
    const bool valid = lane < wlen;
    const int64_t i = valid ? base + lane : base;
    const uint64_t heads = __ballot(valid && head[i] != 0); // (bit 0 is set)
    const bool closed = base + 64 >= n || head[base + 64] != 0; // the window's last run ends with the window
    // the run of this lane, as lanes [ls, le)
    const int ls = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
    const uint64_t above = lane < 63 ? heads >> (lane + 1) : 0;
    const int le = above ? lane + 1 + __builtin_ctzll(above) : wlen;
    const int len = le - ls;
    const bool whole = le < wlen || closed;
    const bool mine = valid && base + ls < slice1;
    // the run that does not end inside the window (only the last one can): from lane 0 on it is longer than a wavefront,
    // else the next window starts with it
    const uint64_t open = __ballot(mine && !whole && lane == ls);
    const bool packed = mine && whole && len <= short_max;
    if (mine && lane == ls && (whole ? len > short_max : ls == 0)) long_list[atomicAdd(nlong, 1u)] = (uint32_t)(base + ls);
    uint8_t st = 1; // a singleton is kept
    if (__ballot(packed && len > 1) != 0) {
      if (valid) {
        rect_s[lane] = site_rect(h, i);
        key_s[lane] = h.e_tot[i];
      }
      __syncthreads();
      int maxlen = packed ? len : 0;
      for (int o = 32; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
      const int4 r = rect_s[valid ? lane : 0];
      const double e = key_s[valid ? lane : 0];
      uint64_t before = 0; // the lanes of the run that intersect this one and come before it in the order
      for (int k = 0; k < maxlen; k++) {
        const int j = ls + k;
        if (packed && k < len && j != lane && site_intersect(r, rect_s[j]) && site_before(key_s[j], j, e, lane)) before |= 1ull << j;
      }
      uint64_t kept = 0, dropped = 0;
      st = 0;
      for (int round = 0; round < maxlen; round++) {
        if (packed && st == 0) {
          if (before & kept) st = 2;
          else if ((before & ~dropped) == 0) st = 1;
        }
        kept = __ballot(packed && st == 1);
        dropped = __ballot(packed && st == 2);
        if (__ballot(packed && st == 0) == 0) break;
      }
      __syncthreads(); // (the next window writes the same LDS)
    }
    if (packed) keep[i] = st == 1;
    if (open == 0 || (open & 1)) break; // nothing open, or the long run: whatever follows starts behind the slice
    base += __builtin_ctzll(open);
  }
}

// A run's rectangles, energies and state, indexed from the run's first hit: in the workgroup's LDS ...
struct SiteLds {
  int4 *rect;
  double *key;
  int32_t *lo;
  uint16_t *hi;
  volatile uint8_t *st;
  __device__ __forceinline__ int4 r(int k) const { return rect[k]; }
  __device__ __forceinline__ double e(int k) const { return key[k]; }
  __device__ __forceinline__ int d0(int k) const { return rect[k].z; }
  __device__ __forceinline__ int get_hi(int k) const { return hi[k]; }
  __device__ __forceinline__ void set_hi(int k, int v) const { hi[k] = (uint16_t)v; }
};
// ... or, for a run beyond the LDS capacity, read from the list itself with the state in HBM scratch (through the L2:
// a workgroup's run is a few hundred KB)
struct SiteHbm {
  HitSoA h; // from the run's first hit on
  int32_t *lo, *hi;
  volatile uint8_t *st;
  __device__ __forceinline__ int4 r(int k) const { return site_rect(h, k); }
  __device__ __forceinline__ double e(int k) const { return h.e_tot[k]; }
  __device__ __forceinline__ int d0(int k) const { return h.db_sp[k]; }
  __device__ __forceinline__ int get_hi(int k) const { return hi[k]; }
  __device__ __forceinline__ void set_hi(int k, int v) const { hi[k] = v; }
};

constexpr int kSiteBlock = 256;

// One run of L hits by one workgroup, the hits dealt round-robin to its threads.  The search's list is sorted by db_sp,
// so hit k can intersect only a window [lo, hi) of its run: hi = the first hit behind k that starts behind k's target
// interval, lo = the first hit whose own window reaches k (an atomicMin from every such hit while it looks for its
// hi).  A caller's list (prb_distinct_sites) need not be sorted: then the window is the run.  state: 0 undecided,
// 1 kept, 2 dropped.
template <class S> __device__ void site_select_run(const S &s, int L, uint8_t *__restrict__ keep) {
  const int tid = threadIdx.x;
  int unsorted = 0;
  for (int k = tid; k < L; k += kSiteBlock) {
    if (k + 1 < L) unsorted |= s.d0(k + 1) < s.d0(k);
    s.lo[k] = k;
    s.st[k] = 0;
  }
  unsorted = __syncthreads_or(unsorted);
  for (int k = tid; k < L; k += kSiteBlock) {
    int j = L;
    if (unsorted) {
      s.lo[k] = 0;
    } else {
      const int d1 = s.r(k).w;
      for (j = k + 1; j < L; j++) {
        if (s.d0(j) > d1) break;
        atomicMin(&s.lo[j], k);
      }
    }
    s.set_hi(k, j);
  }
  __syncthreads();
  for (int round = 0; round < L; round++) {
    int undecided = 0;
    for (int k = tid; k < L; k += kSiteBlock) {
      if (s.st[k] != 0) continue;
      const int4 r = s.r(k);
      const double e = s.e(k);
      const int hi = s.get_hi(k);
      bool waits = false, drop = false;
      for (int j = s.lo[k]; j < hi; j++) {
        if (j == k) continue;
        const uint8_t sj = s.st[j];
        if (sj == 2 || !site_intersect(r, s.r(j)) || !site_before(s.e(j), j, e, k)) continue;
        if (sj == 1) {
          drop = true;
          break;
        }
        waits = true;
      }
      if (drop) s.st[k] = 2;
      else if (!waits) s.st[k] = 1;
      else undecided = 1;
    }
    if (__syncthreads_or(undecided) == 0) break;
  }
  for (int k = tid; k < L; k += kSiteBlock) keep[k] = s.st[k] == 1;
}

// The runs of long_list, one workgroup each (the workgroups take them in turns): up to lds_hits hits with everything in
// LDS (62 KB for kSiteLdsHits: two workgroups per CU), longer ones through SiteHbm with lo / hi / state = scratch of
// one entry per hit of the list.
__global__ __launch_bounds__(kSiteBlock) void k_site_select_long(HitSoA h, int64_t n, const uint8_t *__restrict__ head,
                                                                 const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ nlong,
                                                                 int lds_hits, int32_t *lo, int32_t *hi, uint8_t *state, uint8_t *keep) {
  __shared__ int4 rect_s[kSiteLdsHits];
  __shared__ double key_s[kSiteLdsHits];
  __shared__ int32_t lo_s[kSiteLdsHits];
  __shared__ uint16_t hi_s[kSiteLdsHits];
  __shared__ uint8_t st_s[kSiteLdsHits];
  __shared__ unsigned end_s;
  const int tid = threadIdx.x;
  const uint32_t nl = *nlong;
  for (uint32_t run = blockIdx.x; run < nl; run += gridDim.x) {
    const int64_t s0 = long_list[run];
    // the run ends at the next head flag (or with the list)
    if (tid == 0) end_s = 0xFFFFFFFFu;
    __syncthreads();
    for (int64_t c0 = s0 + 1; c0 < n + kSiteBlock; c0 += kSiteBlock) {
      const int64_t pos = c0 + tid;
      const int ends = pos >= n || head[pos] != 0;
      if (ends) atomicMin(&end_s, (unsigned)min(pos, n));
      if (__syncthreads_or(ends)) break;
    }
    const int L = (int)((int64_t)end_s - s0);
    if (L <= lds_hits) {
      for (int k = tid; k < L; k += kSiteBlock) {
        rect_s[k] = site_rect(h, s0 + k);
        key_s[k] = h.e_tot[s0 + k];
      }
      __syncthreads();
      site_select_run(SiteLds{rect_s, key_s, lo_s, hi_s, st_s}, L, keep + s0);
    } else {
      const HitSoA hr{h.q_sp + s0, h.db_sp + s0, h.q_len + s0, h.db_len + s0, h.db_id + s0, h.db_id_start + s0, h.query + s0,
                      h.e_acc + s0, h.e_hyb + s0, h.e_tot + s0};
      site_select_run(SiteHbm{hr, lo + s0, hi + s0, state + s0}, L, keep + s0);
    }
    __syncthreads(); // (the next run takes the same LDS)
  }
}

// ---- top-N tables (prb_search_page_top, prb_search_page_tophits) ----
// What k_top_merge ranks: the per-pair summaries by e_min into prb_top_pair slots, or the final hits by e_tot into
// prb_top_hit slots.  Either record is 64 bytes with `query` in it, and either slot is the record, `page`, `rank`.
struct TopPairs {
  using Rec = prb_pair_summary;
  using Slot = prb_top_pair;
  static __device__ __forceinline__ double energy(const Rec &r) { return r.e_min; }
  static __device__ __forceinline__ Rec &body(Slot &s) { return s.s; }
  static __device__ __forceinline__ const Rec &body(const Slot &s) { return s.s; }
};
struct TopHits {
  using Rec = prb_hit;
  using Slot = prb_top_hit;
  static __device__ __forceinline__ double energy(const Rec &r) { return r.e_tot; }
  static __device__ __forceinline__ Rec &body(Slot &s) { return s.h; }
  static __device__ __forceinline__ const Rec &body(const Slot &s) { return s.h; }
};
static_assert(sizeof(prb_pair_summary) == 64 && sizeof(prb_hit) == 64 && sizeof(prb_top_pair) == 72 && sizeof(prb_top_hit) == 72,
              "k_top_merge moves a record as 8 x 8 bytes");
// A record's rank key is (energy key, tie key), compared as two u64 with the smaller one first.  The energy key maps
// the energy to an unsigned integer of the same order (-0.0 becomes +0.0 first, so the two compare equal); the tie key is
// (page << 32) | ordinal, the pair's position among its query's records of that page: the `-t` output order.  Within
// one table no two pairs share a tie key (a page is merged once), so every merge below is one of distinct keys.
constexpr int kTopBlock = 256;
constexpr int kTopLoads = 4;                        // records per lane per step of the stream (loads in flight)
constexpr int kTopTile = kTopBlock * kTopLoads;     // records per step
constexpr int kTopCap = 2 * kTopMaxN;               // candidate buffer: room for at least one step beyond kTopMaxN
constexpr int kTopPer = kTopMaxN / kTopBlock;       // set entries per lane in a merge
constexpr int kTopCandPer = kTopCap / kTopBlock;    // candidate entries per lane in a merge
static_assert(kTopPer * kTopBlock == kTopMaxN && kTopTile <= kTopCap - kTopMaxN, "top-N entries per lane");

__device__ __forceinline__ uint64_t energy_key(double e) {
  const uint64_t b = (uint64_t)__double_as_longlong(e + 0.0);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ bool key_less(uint64_t a1, uint64_t a2, uint64_t b1, uint64_t b2) {
  return a1 < b1 || (a1 == b1 && a2 < b2);
}
// entries of the sorted keys (k1, k2)[0, n) below (x1, x2)
__device__ __forceinline__ int count_below(const uint64_t *k1, const uint64_t *k2, int n, uint64_t x1, uint64_t x2) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key_less(k1[m], k2[m], x1, x2)) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// One workgroup per query q = q0 + blockIdx.x of a sub-batch.  rec[0, nrec) are the sub-batch's pair records against
// `page`, ascending by query, so q's records are one run [a, b).  The table keeps q's best pairs in slots
// tab[q * n, q * n + fill[q]), in rank order; on the device a slot's `rank` holds its ordinal.
// LDS (dynamic): the current set's keys and sources (n entries) and a candidate buffer of cap = kTopCap entries.  The
// run streams through in steps of kTopTile records, kTopLoads per lane (one wavefront ballot per load): a record whose
// key beats the set's n-th key (any key while the set is not full) is appended to the buffer, placed by the ballots
// and the waves' counts.  When the next step might not fit, the buffer is bitonic-sorted and merged into the set (each entry's new place = its index + the entries of the
// other list below it), the set is cut to n and the threshold drops.  At the end the set's records are gathered -
// new ones from rec, kept ones from their old slots - and written in rank order.
template <class R>
__global__ __launch_bounds__(kTopBlock) void k_top_merge(const typename R::Rec *__restrict__ rec, int64_t nrec, int32_t q0,
                                                         int32_t page, int32_t n, int32_t cap, typename R::Slot *__restrict__ tab,
                                                         int32_t *__restrict__ fill) {
  using Rec = typename R::Rec;
  using Slot = typename R::Slot;
  extern __shared__ uint64_t top_lds[];
  uint64_t *sk1 = top_lds, *sk2 = sk1 + n, *ck1 = sk2 + n, *ck2 = ck1 + cap;
  uint32_t *ssrc = reinterpret_cast<uint32_t *>(ck2 + cap); // < 2^31: the old slot; else 2^31 | ordinal of a new record
  __shared__ int64_t s_run[2];
  __shared__ int s_wave[kTopBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t q = q0 + (int32_t)blockIdx.x;
  if (tid < 2) { // lower bound of q (tid 0) and of q + 1 (tid 1) in rec
    const int32_t want = q + tid;
    int64_t lo = 0, hi = nrec;
    while (lo < hi) {
      const int64_t m = (lo + hi) >> 1;
      if (rec[m].query < want) lo = m + 1;
      else hi = m;
    }
    s_run[tid] = lo;
  }
  __syncthreads();
  const int64_t a = s_run[0], b = s_run[1];
  if (a >= b) return; // (uniform: no record of q against this page)
  Slot *const slots = tab + (int64_t)q * n;
  int cnt = fill[q];
  for (int i = tid; i < cnt; i += kTopBlock) {
    const Slot &t = slots[i];
    sk1[i] = energy_key(R::energy(R::body(t)));
    sk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
    ssrc[i] = (uint32_t)i;
  }
  __syncthreads();
  uint64_t thr1 = ~0ull, thr2 = ~0ull;
  if (cnt == n) {
    thr1 = sk1[n - 1];
    thr2 = sk2[n - 1];
  }
  int bcnt = 0;
  bool changed = false;
  auto flush = [&]() { // (uniform) sort the buffer, merge it into the set, cut to n
    int P = 1;
    while (P < bcnt) P <<= 1;
    for (int i = bcnt + tid; i < P; i += kTopBlock) ck1[i] = ck2[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P; i += kTopBlock) {
          const int o = i ^ j;
          if (o > i) {
            const uint64_t x1 = ck1[i], x2 = ck2[i], y1 = ck1[o], y2 = ck2[o];
            if (key_less(y1, y2, x1, x2) == ((i & k) == 0)) {
              ck1[i] = y1;
              ck2[i] = y2;
              ck1[o] = x1;
              ck2[o] = x2;
            }
          }
        }
        __syncthreads();
      }
    }
    constexpr int kE = kTopPer + kTopCandPer;
    uint64_t e1[kE], e2[kE];
    uint32_t src[kE];
    int pos[kE];
#pragma unroll
    for (int r = 0; r < kTopPer; r++) {
      const int i = tid + r * kTopBlock;
      pos[r] = n; // (not written)
      if (i < cnt) {
        e1[r] = sk1[i];
        e2[r] = sk2[i];
        src[r] = ssrc[i];
        pos[r] = i + count_below(ck1, ck2, bcnt, e1[r], e2[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kTopCandPer; r++) {
      const int i = tid + r * kTopBlock;
      pos[kTopPer + r] = n;
      if (i < bcnt) {
        e1[kTopPer + r] = ck1[i];
        e2[kTopPer + r] = ck2[i];
        src[kTopPer + r] = 0x80000000u | (uint32_t)ck2[i];
        pos[kTopPer + r] = i + count_below(sk1, sk2, cnt, ck1[i], ck2[i]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kE; r++) {
      if (pos[r] < n) {
        sk1[pos[r]] = e1[r];
        sk2[pos[r]] = e2[r];
        ssrc[pos[r]] = src[r];
      }
    }
    __syncthreads();
    cnt = min(n, cnt + bcnt);
    bcnt = 0;
    changed = true;
    if (cnt == n) {
      thr1 = sk1[n - 1];
      thr2 = sk2[n - 1];
    }
  };
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t base = a; base < b; base += kTopTile) {
    if (bcnt + kTopTile > cap) flush();
    double e[kTopLoads];
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) { // (all loads issued before the first is used)
      const int64_t i = base + u * kTopBlock + tid;
      e[u] = i < b ? R::energy(rec[i]) : 0.0;
    }
    uint64_t k1[kTopLoads], mask[kTopLoads];
    bool take[kTopLoads];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) {
      const int64_t i = base + u * kTopBlock + tid;
      k1[u] = energy_key(e[u]);
      take[u] = i < b && key_less(k1[u], ((uint64_t)(uint32_t)page << 32) | (uint32_t)(i - a), thr1, thr2);
      mask[u] = __ballot(take[u]);
      mine += __popcll(mask[u]);
    }
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    int off = bcnt, total = 0;
#pragma unroll
    for (int w = 0; w < kTopBlock / 64; w++) {
      const int c = s_wave[w];
      off += w < wave ? c : 0;
      total += c;
    }
#pragma unroll
    for (int u = 0; u < kTopLoads; u++) {
      if (take[u]) {
        const int64_t i = base + u * kTopBlock + tid;
        const int at = off + __popcll(mask[u] & below);
        ck1[at] = k1[u];
        ck2[at] = ((uint64_t)(uint32_t)page << 32) | (uint32_t)(i - a);
      }
      off += __popcll(mask[u]);
    }
    bcnt += total;
    __syncthreads(); // (the buffer is complete, s_wave free for the next step)
  }
  if (bcnt > 0) flush();
  if (!changed) return;
  // Write-back in rank order.  A kept pair moves from slot s to a place j >= s, so rounds of 256 places from the top
  // down never read a slot an earlier round wrote; within a round every lane reads before any lane writes.
  for (int r0 = ((cnt - 1) / kTopBlock) * kTopBlock; r0 >= 0; r0 -= kTopBlock) {
    const int j = r0 + tid;
    const Rec *from = nullptr; // (the record, moved as 8 x 8 bytes: 8-byte aligned in both places)
    int32_t pg = 0, rk = 0;
    if (j < cnt) {
      const uint32_t s = ssrc[j];
      if (s & 0x80000000u) {
        rk = (int32_t)(s & 0x7FFFFFFFu);
        from = rec + a + rk;
        pg = page;
      } else if ((int)s != j) {
        from = &R::body(slots[s]);
        pg = slots[s].page;
        rk = slots[s].rank;
      }
    }
    uint2 v[8];
    if (from) {
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint2 *>(from)[k];
    }
    __syncthreads();
    if (from) {
      uint2 *to = reinterpret_cast<uint2 *>(&R::body(slots[j]));
#pragma unroll
      for (int k = 0; k < 8; k++) to[k] = v[k];
      slots[j].page = pg;
      slots[j].rank = rk;
    }
  }
  if (tid == 0) fill[q] = cnt;
}

// ---- two tables of one kind into one (prb_topset_merge, prb_tophits_merge) ----
// One workgroup per query.  The query's slots in use are two ranked lists - tab's and src's - over disjoint page sets, so
// no two of their (energy key, tie key) pairs are equal, and an entry's place in the union is its index plus the entries
// of the other list below it (binary-search rank: no re-sort).  LDS (dynamic): the two lists' keys (n entries each) and
// the sources of the n places kept - < 2^31: tab's slot, else 2^31 | src's slot.  A record from src keeps its page and
// ordinal; shift = what is added to its bp_offset (the top-N hit table: its list lies behind tab's pool, see
// k_tophits_gather).  The write-back is k_top_merge's: in rank order, from the top down.
template <class R> struct TopRebase;
template <> struct TopRebase<TopPairs> {
  static __device__ __forceinline__ void apply(prb_top_pair &, int64_t) {}
};
template <> struct TopRebase<TopHits> {
  static __device__ __forceinline__ void apply(prb_top_hit &s, int64_t shift) { s.h.bp_offset += shift; }
};
template <class R>
__global__ __launch_bounds__(kTopBlock) void k_table_merge(typename R::Slot *__restrict__ tab, int32_t *__restrict__ fill,
                                                           const typename R::Slot *__restrict__ src, const int32_t *__restrict__ src_fill,
                                                           int32_t n, int64_t shift) {
  using Slot = typename R::Slot;
  extern __shared__ uint64_t top_lds[];
  uint64_t *dk1 = top_lds, *dk2 = dk1 + n, *sk1 = dk2 + n, *sk2 = sk1 + n;
  uint32_t *from = reinterpret_cast<uint32_t *>(sk2 + n);
  const int tid = threadIdx.x;
  const int32_t q = (int32_t)blockIdx.x;
  const int cs = min(max(src_fill[q], 0), n);
  if (cs == 0) return; // (uniform: src has nothing of q)
  const int cd = min(max(fill[q], 0), n);
  Slot *const slots = tab + (int64_t)q * n;
  const Slot *const other = src + (int64_t)q * n;
  for (int i = tid; i < cd; i += kTopBlock) {
    const Slot &t = slots[i];
    dk1[i] = energy_key(R::energy(R::body(t)));
    dk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
  }
  for (int i = tid; i < cs; i += kTopBlock) {
    const Slot &t = other[i];
    sk1[i] = energy_key(R::energy(R::body(t)));
    sk2[i] = ((uint64_t)(uint32_t)t.page << 32) | (uint32_t)t.rank;
  }
  for (int i = tid; i < n; i += kTopBlock) from[i] = (uint32_t)i; // (every place has a source inside the table, whatever the keys)
  __syncthreads();
  for (int i = tid; i < cd; i += kTopBlock) {
    const int pos = i + count_below(sk1, sk2, cs, dk1[i], dk2[i]);
    if (pos < n) from[pos] = (uint32_t)i;
  }
  for (int i = tid; i < cs; i += kTopBlock) {
    const int pos = i + count_below(dk1, dk2, cd, sk1[i], sk2[i]);
    if (pos < n) from[pos] = 0x80000000u | (uint32_t)i;
  }
  __syncthreads();
  const int cnt = min(n, cd + cs);
  // A kept record of tab moves from slot s to a place j >= s, so rounds of 256 places from the top down never read a
  // slot an earlier round wrote; within a round every lane reads before any lane writes.
  for (int r0 = ((cnt - 1) / kTopBlock) * kTopBlock; r0 >= 0; r0 -= kTopBlock) {
    const int j = r0 + tid;
    bool move = false;
    Slot v;
    if (j < cnt) {
      const uint32_t s = from[j];
      if (s & 0x80000000u) {
        v = other[s & 0x7FFFFFFFu];
        TopRebase<R>::apply(v, shift);
        move = true;
      } else if ((int)s != j) {
        v = slots[s];
        move = true;
      }
    }
    __syncthreads();
    if (move) slots[j] = v;
  }
  if (tid == 0) fill[q] = cnt;
}

// ---- base pairs of the top-N hit table ----
// The kept hits' lists lie in a pool in table order without gaps.  After a merge: the counts of the slots in use, their
// exclusive scan (rocPRIM, on the host side), then every list gathered into a second pool at its scanned place.
__global__ __launch_bounds__(kBlock) void k_tophits_counts(const prb_top_hit *__restrict__ tab, const int32_t *__restrict__ fill,
                                                           int32_t n, int64_t nslots, int32_t *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > nslots) return;
  int32_t c = 0;
  if (i < nslots && (int32_t)(i % n) < fill[i / n]) c = max(tab[i].h.bp_count, 0);
  cnt[i] = c;
}
// kTopHitLanes lanes per slot, a pair (8 bytes) per lane and step.  A hit that came with this merge has an offset at
// or beyond `split`, the old pool's size in pairs - its list lies in `fresh` at that offset less `split` -, every other
// one lies in the old pool.  (The lanes of a slot have its old offset in a register before they copy, the first of them
// replaces it behind the copy.)
constexpr int kTopHitLanes = 16;
static_assert(kBlock % kTopHitLanes == 0, "whole slots per workgroup");
__global__ __launch_bounds__(kBlock) void k_tophits_gather(prb_top_hit *__restrict__ tab, const int32_t *__restrict__ fill, int32_t n,
                                                           int64_t nslots, const int64_t *__restrict__ off, int64_t split,
                                                           const int2 *__restrict__ old_pool, const int2 *__restrict__ fresh,
                                                           int2 *__restrict__ pool) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = t / kTopHitLanes;
  const int sub = (int)(t % kTopHitLanes);
  if (i >= nslots) return;
  const int32_t q = (int32_t)(i / n);
  if ((int32_t)(i % n) >= fill[q]) return;
  prb_top_hit &slot = tab[i];
  const int32_t c = max(slot.h.bp_count, 0);
  const int64_t from = slot.h.bp_offset, to = off[i];
  const int2 *src = from >= split ? fresh + (from - split) : old_pool + from;
  for (int32_t j = sub; j < c; j += kTopHitLanes) pool[to + j] = src[j];
  if (sub == 0) slot.h.bp_offset = to;
}

// ---- per-position profile (prb_search_page_profile) ----
// Every column is an integer count, a minimum or a lexicographic minimum, built with integer atomics only, so the table
// does not depend on the order in which hits, sub-batches or pages arrive.  A hit's span is [min(q0, qN), max(q0, qN)]
// of its `-s 0` end pairs (q0 <= qN except for the unsorted first hit of a list).  The kernels run a lane
// per hit over the whole grid (a query's hits spread over many workgroups); a lane walks its span, which is short (tens
// of positions), and the atomics of the minima are skipped wherever the value already there is not larger.
__device__ __forceinline__ void prof_span(const int32_t *ends, int64_t h, int32_t &lo, int32_t &hi) {
  const int32_t a = ends[4 * h], b = ends[4 * h + 2];
  lo = min(a, b);
  hi = max(a, b);
}
// the slots of hit h's span: first slot, or -1 (and `bad` raised) when the span lies outside its query
__device__ __forceinline__ int64_t prof_base(const ProfTab &t, int32_t q, int32_t lo, int32_t hi) {
  if (q < 0 || q >= t.nq || lo < 0 || (int64_t)hi >= t.off[q + 1] - t.off[q] - 1) {
    atomicOr(t.bad, 1u);
    return -1;
  }
  return t.off[q];
}
__device__ __forceinline__ unsigned long long prof_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t prof_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_prof_keys(int64_t n, const uint32_t *__restrict__ start, int64_t npairs,
                                                      const int32_t *__restrict__ ends, uint64_t *key, uint32_t *val) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int64_t lo = 0, hi = npairs; // the last pair that starts at or before i
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if ((int64_t)start[m] <= i) lo = m;
    else hi = m;
  }
  int32_t a, b;
  prof_span(ends, i, a, b);
  key[i] = ((uint64_t)lo << 32) | (uint32_t)a;
  val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_prof_span(int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                      const int32_t *__restrict__ ends, uint64_t *v) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int32_t a, b;
  prof_span(ends, val[i], a, b);
  v[i] = (key[i] & 0xFFFFFFFF00000000ull) | (uint32_t)max(b + 1, 0);
}

// Hits sorted by (pair, first position): m[i - 1] of the same pair holds 1 + the furthest position that the pair's
// earlier hits reach, so [max(lo, that), hi] is what hit i adds to the union of the pair's spans (nothing if empty).
__global__ __launch_bounds__(kBlock) void k_prof_add(HitSoA h, int64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                     const uint64_t *__restrict__ m, const int32_t *__restrict__ ends, ProfTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = val[i];
  int32_t lo, hi;
  prof_span(ends, x, lo, hi);
  const int64_t base = prof_base(t, h.query[x], lo, hi);
  if (base < 0) return;
  atomicAdd(&t.hdiff[base + lo], 1ull);
  atomicAdd(&t.hdiff[base + hi + 1], ~0ull);
  int32_t from = lo;
  if (i > 0 && (m[i - 1] >> 32) == (key[i] >> 32)) from = max(lo, (int32_t)(uint32_t)m[i - 1]);
  if (from <= hi) {
    atomicAdd(&t.tdiff[base + from], 1);
    atomicAdd(&t.tdiff[base + hi + 1], -1);
  }
}

// pass 0: skey = min energy key; pass 1 (after pass 0 has finished): stie = min place among the hits at that key
template <int kPass>
__global__ __launch_bounds__(kBlock) void k_prof_min(HitSoA h, int64_t n, const uint32_t *__restrict__ val, const int32_t *__restrict__ ends,
                                                     ProfTab t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = val[i]; // (in span order: neighbouring lanes walk neighbouring positions)
  int32_t lo, hi;
  prof_span(ends, x, lo, hi);
  const int64_t base = prof_base(t, h.query[x], lo, hi);
  if (base < 0) return;
  const unsigned long long ek = energy_key(h.e_tot[x]);
  for (int64_t p = base + lo; p <= base + hi; p++) {
    if (kPass == 0) {
      if (ek < prof_load(&t.skey[p])) atomicMin(&t.skey[p], ek); // (the value only falls: a skipped atomic would not have won)
    } else if (t.skey[p] == ek && x < prof_load(&t.stie[p])) {
      atomicMin(&t.stie[p], x);
    }
  }
}

// A slot the sub-batch covers takes the sub-batch's best hit if (key, page << 32 | place) is below the table's.  The
// sub-batch's list is gone once the page is done, so the hit's fields are copied now.
__global__ __launch_bounds__(kBlock) void k_prof_merge(HitSoA h, const int32_t *__restrict__ ends, ProfTab t, int64_t p0, int64_t p1,
                                                       int32_t page) {
  const int64_t p = p0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= p1) return;
  const unsigned long long sk = t.skey[p];
  if (sk == ~0ull) return; // (not covered in this sub-batch: the scratch is untouched)
  const uint32_t x = t.stie[p];
  const unsigned long long tie = ((unsigned long long)(uint32_t)page << 32) | x;
  const unsigned long long k = t.key[p];
  if (sk < k || (sk == k && tie < t.tie[p])) {
    t.key[p] = sk;
    t.tie[p] = tie;
    t.e_min[p] = h.e_tot[x];
    t.db_id[p] = h.db_id[x];
#pragma unroll
    for (int c = 0; c < 4; c++) t.bp[4 * p + c] = ends[4 * x + c];
  }
  t.skey[p] = ~0ull;
  t.stie[p] = ~0u;
}

// prb_profset_merge: the table s, over other pages of the same batch, into t, a lane per slot.  The difference arrays
// add (no page is in both, so no (page, db_id) is counted twice among the targets); the best hit is the lower of the two
// (key, tie) pairs.
__global__ __launch_bounds__(kBlock) void k_prof_join(ProfTab t, ProfTab s, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p == 0 && *s.bad) *t.bad = 1u;
  if (p >= P) return;
  t.hdiff[p] += s.hdiff[p];
  t.tdiff[p] += s.tdiff[p];
  const unsigned long long sk = s.key[p], st = s.tie[p], k = t.key[p];
  if (sk < k || (sk == k && st < t.tie[p])) {
    t.key[p] = sk;
    t.tie[p] = st;
    t.e_min[p] = s.e_min[p];
    t.db_id[p] = s.db_id[p];
#pragma unroll
    for (int c = 0; c < 4; c++) t.bp[4 * p + c] = s.bp[4 * p + c];
  }
}

__global__ __launch_bounds__(kBlock) void k_prof_rows(ProfTab t, const uint32_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ hits,
                                                      const int32_t *__restrict__ targets, prb_profile_pos *rows) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int64_t p = idx[j];
  int32_t lo = 0, hi = t.nq; // the query whose slots hold p
  while (hi - lo > 1) {
    const int32_t m = (lo + hi) >> 1;
    if (t.off[m] <= p) lo = m;
    else hi = m;
  }
  prb_profile_pos r;
  r.query = lo;
  r.pos = (int32_t)(p - t.off[lo]);
  r.hits = hits[p];
  r.targets = targets[p];
  r.page = (int32_t)(t.tie[p] >> 32);
  r.db_id = t.db_id[p];
  r.reserved = 0;
  r.e_min = t.e_min[p];
  r.bp_first[0] = t.bp[4 * p];
  r.bp_first[1] = t.bp[4 * p + 1];
  r.bp_last[0] = t.bp[4 * p + 2];
  r.bp_last[1] = t.bp[4 * p + 3];
  rows[j] = r;
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

// ------------------------------------------------------------------- redundancy filter
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

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

} // namespace

hipError_t launch_sa_seq(const PageDev &pg, int32_t *sa_seq, hipStream_t s) {
  if (pg.nchars <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sa_seq, grid_for(pg.nchars), dim3(kBlock), 0, s, pg, sa_seq);
  return hipGetLastError();
}
hipError_t launch_seed_qacc(const CandDev *cands, int32_t ncand, int64_t nq_entries, const QBatchDev &qb, int delta, double *qacc,
                            hipStream_t s) {
  if (nq_entries <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_seed_qacc, grid_for(nq_entries), dim3(kBlock), 0, s, cands, ncand, nq_entries, qb, delta, qacc);
  return hipGetLastError();
}
hipError_t launch_row_keys(const CandDev *cands, int32_t ncand, int64_t nrows, const PageDev &pg, int qmin, int shift, int dbits,
                           bool wide, int32_t *row_cand, void *key, uint32_t *val, hipStream_t s) {
  if (nrows <= 0) return hipSuccess;
  if (wide)
    hipLaunchKernelGGL(k_row_key<uint64_t>, grid_for(nrows), dim3(kBlock), 0, s, cands, ncand, nrows, pg, qmin, shift, dbits, row_cand,
                       (uint64_t *)key, val);
  else
    hipLaunchKernelGGL(k_row_key<uint32_t>, grid_for(nrows), dim3(kBlock), 0, s, cands, ncand, nrows, pg, qmin, shift, dbits, row_cand,
                       (uint32_t *)key, val);
  return hipGetLastError();
}
hipError_t launch_seed_count(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                             int delta, const double *qacc, int32_t *row_count, int32_t *row_cand, const uint32_t *row_perm,
                             hipStream_t s) {
  if (nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_seed<false>, grid_for(nrows), dim3(kBlock), 0, s, cands, ncand, nrows, qb, pg, delta, qacc, row_count,
                     row_cand, (const int64_t *)nullptr, HitSoA{}, row_perm);
  return hipGetLastError();
}
hipError_t launch_seed_emit(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                            int delta, const double *qacc, const int32_t *row_cand, const int64_t *row_off, HitSoA hits,
                            const uint32_t *row_perm, hipStream_t s) {
  if (nrows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_seed<true>, grid_for(nrows), dim3(kBlock), 0, s, cands, ncand, nrows, qb, pg, delta, qacc,
                     (int32_t *)nullptr, const_cast<int32_t *>(row_cand), row_off, hits, row_perm);
  return hipGetLastError();
}
hipError_t launch_blk_seq(const PageDev &pg, int32_t *blk_seq, hipStream_t s) {
  const int64_t nblk = blk_seq_entries(pg.nchars);
  hipLaunchKernelGGL(k_blk_seq, grid_for(nblk), dim3(kBlock), 0, s, pg, blk_seq, nblk);
  return hipGetLastError();
}
hipError_t launch_pair_keys(const CandDev *cands, const int64_t *pair0, int32_t ncand, int64_t npairs, const PageDev &pg, int qmin,
                            int shift, int dbits, bool wide, void *key, uint64_t *val, hipStream_t s) {
  if (npairs <= 0) return hipSuccess;
  if (wide)
    hipLaunchKernelGGL(k_pair_key<uint64_t>, grid_for(npairs), dim3(kBlock), 0, s, cands, pair0, ncand, npairs, pg, qmin, shift, dbits,
                       (uint64_t *)key, val);
  else
    hipLaunchKernelGGL(k_pair_key<uint32_t>, grid_for(npairs), dim3(kBlock), 0, s, cands, pair0, ncand, npairs, pg, qmin, shift, dbits,
                       (uint32_t *)key, val);
  return hipGetLastError();
}
hipError_t launch_seed_extend(const CandDev *cands, const uint64_t *vals, int64_t npairs, const QBatchDev &qb, const PageDev &pg,
                              const SearchConst &sc, ExtOpts o, const double *qacc, double thr, int max_query_len, void *slices,
                              int32_t *slice_count, uint64_t *nseed, hipStream_t s) {
  if (npairs <= 0) return hipSuccess;
  int qcap = (max_query_len + 1 + 3) & ~3; // as launch_ungapped
  if (qcap > 7168) qcap = 7168;
  FuseArgs f{cands, vals, npairs, qacc, thr, static_cast<SliceRec *>(slices), slice_count, reinterpret_cast<unsigned long long *>(nseed),
             qcap};
  // (4, 5 or 6 positions fetched ahead instead of 8: the same 273-290 ms per configs[2] step)
  hipLaunchKernelGGL(k_seed_extend<8>, dim3((unsigned)fused_slices(npairs)), dim3(kBlock), (size_t)qcap * 9, s, f, qb, pg, sc, o);
  return hipGetLastError();
}
hipError_t launch_collect_slices(const void *slices, const int32_t *slice_count, const int64_t *slice_off, int64_t nslices, HitRec *out,
                                 hipStream_t s) {
  if (nslices <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_collect_slices, dim3((unsigned)nslices), dim3(kBlock), 0, s, static_cast<const SliceRec *>(slices), slice_count,
                     slice_off, out);
  return hipGetLastError();
}
hipError_t launch_ungapped(HitSoA hits, int64_t n, const QBatchDev &qb, const PageDev &pg, const SearchConst &sc, ExtOpts o,
                           int max_query_len, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  // LDS slots per query array: the longest query of the batch, at most 7168 (63 KB per workgroup)
  int qcap = (max_query_len + 1 + 3) & ~3;
  if (qcap > 7168) qcap = 7168;
  const int64_t per_block = (int64_t)kBlock * kUngappedPer;
  hipLaunchKernelGGL(k_ungapped, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBlock), (size_t)qcap * 9, s, hits, n,
                     qb, pg, sc, o, qcap);
  return hipGetLastError();
}
hipError_t launch_make_keys(const HitSoA &hits, int64_t n, uint64_t *k_energy, uint32_t *k_len, uint32_t *k_qsp,
                            uint64_t *k_pos, uint32_t *idx, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_make_keys, grid_for(n), dim3(kBlock), 0, s, hits, n, k_energy, k_len, k_qsp, k_pos, idx);
  return hipGetLastError();
}
hipError_t launch_make_packed_keys(const HitSoA &hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                   uint32_t *idx, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_make_packed_keys, grid_for(n), dim3(kBlock), 0, s, hits, n, f, key, k_energy, idx);
  return hipGetLastError();
}
hipError_t launch_fix_ties(const uint64_t *key_sorted, const uint64_t *e_sorted, const uint32_t *perm, int64_t n, const HitRec *recs,
                           uint32_t *perm_out, int32_t *too_long, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fix_ties, grid_for(n), dim3(kBlock), 0, s, key_sorted, e_sorted, perm, n, recs, perm_out, too_long);
  return hipGetLastError();
}
hipError_t launch_order_keys(const double *v, int64_t n, uint64_t *key, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_order_keys, grid_for(n), dim3(kBlock), 0, s, v, n, key);
  return hipGetLastError();
}
hipError_t launch_gather_u64(const uint64_t *src, const uint32_t *idx, uint64_t *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather<uint64_t>, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
hipError_t launch_gather_u32(const uint32_t *src, const uint32_t *idx, uint32_t *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather<uint32_t>, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
namespace {
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
} // namespace
namespace {
__global__ __launch_bounds__(256) void k_flag_marked(const uint8_t *__restrict__ marks, const uint32_t *__restrict__ list, int64_t n, uint8_t mask,
                                                     uint8_t *flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = (marks[list[i]] & mask) ? 1 : 0;
}
} // namespace
hipError_t launch_flag_marked(const uint8_t *marks, const uint32_t *list, int64_t n, uint8_t mask, uint8_t *flags, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_flag_marked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, marks, list, n, mask, flags);
  return hipGetLastError();
}
hipError_t launch_iota_u32(uint32_t *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_iota_u32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, n);
  return hipGetLastError();
}
hipError_t launch_gather_rows(const void *src, const uint32_t *idx, void *dst, int64_t n, int row_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (row_bytes % 16 != 0) return hipErrorInvalidValue;
  const int words = row_bytes / 16;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n * words + 255) / 256)), dim3(256), 0, s, static_cast<const uint4 *>(src), idx,
                     static_cast<uint4 *>(dst), n, words);
  return hipGetLastError();
}
hipError_t launch_gather_u8(const uint8_t *src, const uint32_t *idx, uint8_t *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather<uint8_t>, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
hipError_t launch_gather_hits(const HitSoA &src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather_hits, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
hipError_t launch_gather_hits_to_recs(const HitSoA &src, const uint32_t *idx, HitRec *dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather_hits_to_recs, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
hipError_t launch_gather_recs_to_hits(const HitRec *src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather_recs_to_hits, grid_for(n), dim3(kBlock), 0, s, src, idx, dst, n);
  return hipGetLastError();
}
hipError_t launch_make_packed_keys_recs(const HitRec *hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                        uint32_t *idx, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_make_packed_keys_recs, grid_for(n), dim3(kBlock), 0, s, hits, n, f, key, k_energy, idx);
  return hipGetLastError();
}
hipError_t launch_pack_hits(const HitSoA &src, int64_t n, const int32_t *bp_count, const int64_t *bp_off, int64_t bp_base,
                            void *out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_hits, grid_for(n), dim3(kBlock), 0, s, src, n, bp_count, bp_off, bp_base, static_cast<prb_hit *>(out));
  return hipGetLastError();
}
hipError_t launch_pair_heads(const int32_t *query, const int32_t *db_id, int64_t n, uint8_t *head, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_heads, grid_for(n), dim3(kBlock), 0, s, query, db_id, n, head);
  return hipGetLastError();
}
hipError_t launch_site_select(const HitSoA &h, int64_t n, const uint8_t *head, int lds_hits, const SiteScratch &w, uint8_t *keep,
                              hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > INT32_MAX) return hipErrorInvalidValue;
  lds_hits = std::min(std::max(lds_hits, 1), kSiteLdsHits);
  if (hipError_t e = hipMemsetAsync(w.nlong, 0, sizeof(uint32_t), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_site_select_packed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, h, n, head, std::min(lds_hits, 64), keep,
                     w.long_list, w.nlong);
  // (how many runs the first kernel left is known on the device only: the workgroups read the count)
  hipLaunchKernelGGL(k_site_select_long, dim3((unsigned)std::min<int64_t>(kSiteLongGrid, site_long_runs_max(n))), dim3(kSiteBlock), 0, s, h,
                     n, head, w.long_list, w.nlong, lds_hits, w.lo, w.hi, w.state, keep);
  return hipGetLastError();
}
hipError_t launch_pair_fold(const HitSoA &h, int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, void *out,
                            hipStream_t s) {
  if (npairs <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_fold, grid_for(npairs), dim3(kBlock), 0, s, h, n, start, npairs, ends, static_cast<prb_pair_summary *>(out));
  return hipGetLastError();
}
template <class R>
static hipError_t launch_top_merge_of(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab,
                                      int32_t *fill, hipStream_t s) {
  if (nrec <= 0 || q1 <= q0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const int cap = kTopCap;
  const size_t lds = (size_t)n * (8 + 8 + 4) + (size_t)cap * 16; // at most 52 KB (n = 1024)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_top_merge<R>), dim3((unsigned)(q1 - q0)), dim3(kTopBlock), lds, s,
                     static_cast<const typename R::Rec *>(rec), nrec, q0, page, n, cap, static_cast<typename R::Slot *>(tab), fill);
  return hipGetLastError();
}
hipError_t launch_top_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                            hipStream_t s) {
  return launch_top_merge_of<TopPairs>(rec, nrec, q0, q1, page, n, tab, fill, s);
}
hipError_t launch_tophits_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                                hipStream_t s) {
  return launch_top_merge_of<TopHits>(rec, nrec, q0, q1, page, n, tab, fill, s);
}
hipError_t launch_tophits_counts(const void *tab, const int32_t *fill, int32_t n, int64_t nslots, int32_t *cnt, hipStream_t s) {
  if (nslots < 0 || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tophits_counts, grid_for(nslots + 1), dim3(kBlock), 0, s, static_cast<const prb_top_hit *>(tab), fill, n, nslots, cnt);
  return hipGetLastError();
}
hipError_t launch_tophits_gather(void *tab, const int32_t *fill, int32_t n, int64_t nslots, const int64_t *off, int64_t split,
                                 const int32_t *old_pool, const int32_t *fresh, int32_t *pool, hipStream_t s) {
  if (nslots <= 0) return hipSuccess;
  if (n < 1 || split < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tophits_gather, grid_for(nslots * kTopHitLanes), dim3(kBlock), 0, s, static_cast<prb_top_hit *>(tab), fill, n, nslots,
                     off, split, reinterpret_cast<const int2 *>(old_pool), reinterpret_cast<const int2 *>(fresh),
                     reinterpret_cast<int2 *>(pool));
  return hipGetLastError();
}
template <class R>
static hipError_t launch_table_merge_of(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n,
                                        int64_t shift, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (n < 1 || n > kTopMaxN) return hipErrorInvalidValue;
  const size_t lds = (size_t)n * (4 * 8 + 4); // at most 36 KB (n = 1024)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_table_merge<R>), dim3((unsigned)nq), dim3(kTopBlock), lds, s, static_cast<typename R::Slot *>(tab),
                     fill, static_cast<const typename R::Slot *>(src), src_fill, n, shift);
  return hipGetLastError();
}
hipError_t launch_top_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, hipStream_t s) {
  return launch_table_merge_of<TopPairs>(tab, fill, src, src_fill, nq, n, 0, s);
}
hipError_t launch_tophits_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, int64_t shift,
                               hipStream_t s) {
  return launch_table_merge_of<TopHits>(tab, fill, src, src_fill, nq, n, shift, s);
}
hipError_t launch_prof_join(const ProfTab &t, const ProfTab &src, int64_t P, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_join, grid_for(P), dim3(kBlock), 0, s, t, src, P);
  return hipGetLastError();
}
hipError_t launch_prof_keys(int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, uint64_t *key, uint32_t *val,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_keys, grid_for(n), dim3(kBlock), 0, s, n, start, npairs, ends, key, val);
  return hipGetLastError();
}
hipError_t launch_prof_span(int64_t n, const uint64_t *key, const uint32_t *val, const int32_t *ends, uint64_t *v, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_span, grid_for(n), dim3(kBlock), 0, s, n, key, val, ends, v);
  return hipGetLastError();
}
hipError_t launch_prof_add(const HitSoA &h, int64_t n, const uint64_t *key, const uint32_t *val, const uint64_t *m, const int32_t *ends,
                           const ProfTab &t, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_add, grid_for(n), dim3(kBlock), 0, s, h, n, key, val, m, ends, t);
  return hipGetLastError();
}
hipError_t launch_prof_min(const HitSoA &h, int64_t n, const uint32_t *val, const int32_t *ends, const ProfTab &t, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_min<0>, grid_for(n), dim3(kBlock), 0, s, h, n, val, ends, t);
  hipLaunchKernelGGL(k_prof_min<1>, grid_for(n), dim3(kBlock), 0, s, h, n, val, ends, t);
  return hipGetLastError();
}
hipError_t launch_prof_merge(const HitSoA &h, const int32_t *ends, const ProfTab &t, int64_t p0, int64_t p1, int32_t page,
                             hipStream_t s) {
  if (p1 <= p0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_merge, grid_for(p1 - p0), dim3(kBlock), 0, s, h, ends, t, p0, p1, page);
  return hipGetLastError();
}
hipError_t launch_prof_rows(const ProfTab &t, const uint32_t *idx, int64_t n, const int64_t *hits, const int32_t *targets, void *rows,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prof_rows, grid_for(n), dim3(kBlock), 0, s, t, idx, n, hits, targets, static_cast<prb_profile_pos *>(rows));
  return hipGetLastError();
}
hipError_t launch_flag_not_above(const double *e_tot, int64_t n, double thr, uint8_t *keep, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_flag_not_above, grid_for(n), dim3(kBlock), 0, s, e_tot, n, thr, keep);
  return hipGetLastError();
}
hipError_t launch_mark_first(const int32_t *query, int64_t n, uint8_t *first, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mark_first, grid_for(n), dim3(kBlock), 0, s, query, n, first);
  return hipGetLastError();
}
hipError_t launch_filter_init(const HitSoA &h, int64_t n, double thr, int64_t *end_key, uint8_t *state, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_filter_init, grid_for(n), dim3(kBlock), 0, s, h, n, thr, end_key, state);
  return hipGetLastError();
}
hipError_t launch_filter_round(const HitSoA &h, int64_t n, const int64_t *pmax, uint8_t *state, int32_t *pending,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const bool tiles = !(getenv("PRB_FILTER_TILES") && atoi(getenv("PRB_FILTER_TILES")) == 0);
  if (tiles) hipLaunchKernelGGL(k_filter_round_tile, grid_for(n), dim3(kBlock), 0, s, h, n, pmax, state, pending);
  else hipLaunchKernelGGL(k_filter_round, grid_for(n), dim3(kBlock), 0, s, h, n, pmax, state, pending);
  return hipGetLastError();
}
hipError_t launch_filter_final(const HitSoA &h, int64_t n, const int64_t *pmax, const uint8_t *state, uint8_t *keep,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const bool tiles = !(getenv("PRB_FILTER_TILES") && atoi(getenv("PRB_FILTER_TILES")) == 0);
  if (tiles) hipLaunchKernelGGL(k_filter_final_tile, grid_for(n), dim3(kBlock), 0, s, h, n, pmax, state, keep);
  else hipLaunchKernelGGL(k_filter_final, grid_for(n), dim3(kBlock), 0, s, h, n, pmax, state, keep);
  return hipGetLastError();
}
} // namespace prb
