// Ungapped extension on gfx950: the walk along a seed's diagonal, on a list of seed hits (k_ungapped) or fused with
// the seed test over the sorted (query SA entry, database SA entry) pairs of a chunk (k_pair_key, k_seed_extend,
// k_collect_slices: "seeds -> extended hits in one pass" below).
//
//   ungapped_walk_reg, k_ungapped <-> UngappedExtension::Run / LoopEnergy          ungapped_extension.cpp:30-186
//   k_seed_extend's seed test     <-> SeedSearch::CalcInteractionEnergy            seed_search.cpp:47-99
//
// HBM/L2-bound gather work on small integer tables; there is no dense contraction in it.  Energies are doubles built
// from exact multiples of 0.01 and float-derived accessibilities, summed in the reference's order (-ffp-contract=off).
#include <algorithm>

#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

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
//   k_pair_key    pair p -> a sort key and a value, in one of two layouts (PairLayout, pair_layout in search_host.hpp):
//                 narrow  key {query - first query : qbits, database position : pbits} in 32 bits,
//                         value {candidate : 20, query entry within the candidate : 12} in 32 bits
//                 wide    key (query - first query, database position >> shift) in 32 or 64 bits,
//                         value {database position : 32, candidate : 20, query entry : 12} in 64 bits
//                         (pages or sub-batches whose narrow key would need more than 32 bits; PRB_SEED_PAIR_WIDE=1)
//   (radix sort of the pairs by key.  The order is there for locality only - (query, position >> shift) - so the narrow
//   layout sorts on the key's bits [g, qbits + pbits) alone, g >= shift: 8 B per pair and pass instead of 12 B, and with
//   g = qbits + pbits - 16 two passes of the radix sort instead of three)
//   k_seed_extend pair -> SeedSearch::CalcInteractionEnergy's test (seed_search.cpp:47-99); a seed is walked at once
//                 (UngappedExtension::Run) and, if it is not above the -f threshold, kept (see SliceRec).  Where g > shift a
//                 workgroup first buckets its tile's pairs on the key bits [shift, g) the sort left out - a counting sort
//                 in LDS, at most 32 buckets - and takes them in bucket order: a wavefront's 64 pairs then come from about
//                 as narrow a span of the database as behind a sort on all the bits
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

// (Val = uint32_t: the narrow layout, shift = 0 and dbits = pbits; uint64_t: the wide one)
template <class Key, class Val>
__global__ __launch_bounds__(kBlock) void k_pair_key(const CandDev *__restrict__ cands, const int64_t *__restrict__ pair0, int ncand,
                                                     int64_t npairs, PageDev pg, int qmin, int shift, int dbits,
                                                     Key *__restrict__ key, Val *__restrict__ val) {
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
  if constexpr (sizeof(Val) == 4) val[p] = (uint32_t)ci | (jrel << kPairCandBits);
  else val[p] = (uint64_t)db_sp | ((uint64_t)(uint32_t)ci << 32) | ((uint64_t)jrel << (32 + kPairCandBits));
}

__device__ __forceinline__ int pair_cand(uint64_t v) { return (int)((v >> 32) & ((1u << kPairCandBits) - 1)); }
__device__ __forceinline__ int pair_cand(uint32_t v) { return (int)(v & ((1u << kPairCandBits) - 1)); }

// Under a pair mask (AllowDev): which of the chunk's pairs are searched at all.  Pair p's query is its candidate's, its
// target the sequence of its database SA entry (sa_seq; the entry from p's place among its candidate's pairs, as
// k_pair_key numbers them).  A wavefront's 64 answers are one ballot: the word and its population count are all that is
// written, so the scatter behind the scan of the counts reads no candidate and no bit of the mask again, the order of
// the pairs is kept and the result does not depend on how the wavefronts are scheduled.
template <class Val>
__global__ __launch_bounds__(kBlock) void k_allow_test(const CandDev *__restrict__ cands, const int64_t *__restrict__ pair0,
                                                       const Val *__restrict__ val, int64_t npairs, PageDev pg, AllowDev allow,
                                                       uint64_t *__restrict__ ballot, int32_t *__restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool ok = false;
  if (p < npairs) {
    const int ci = pair_cand(val[p]);
    const CandDev c = cands[ci];
    const uint32_t pl = (uint32_t)(p - pair0[ci]), qw = (uint32_t)(c.ep_q - c.sp_q + 1);
    ok = pair_allowed(allow, c.query, pg.sa_seq[c.sp_db + (int)(pl / qw)]);
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && p < npairs) {
    ballot[p >> 6] = m;
    count[p >> 6] = __popcll(m);
  }
}
template <class Key, class Val>
__global__ __launch_bounds__(kBlock) void k_allow_scatter(const Key *__restrict__ key_in, const Val *__restrict__ val_in, int64_t npairs,
                                                          const uint64_t *__restrict__ ballot, const int64_t *__restrict__ off,
                                                          Key *__restrict__ key_out, Val *__restrict__ val_out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npairs) return;
  const uint64_t m = ballot[p >> 6];
  const int lane = (int)(p & 63);
  if (!(m >> lane & 1)) return;
  const int64_t at = off[p >> 6] + __popcll(m & ((1ull << lane) - 1));
  key_out[at] = key_in[p];
  val_out[at] = val_in[p];
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
  const uint32_t *keys; // narrow layout: the sorted keys, the database position in their low `pbits` bits
  const void *vals;     // the sorted values: uint32_t (narrow layout) or uint64_t each
  int pbits;
  int lshift, lbits;    // narrow layout: a tile is taken in the order of its key bits [lshift, lshift + lbits) (0 bits: as it is)
  int64_t npairs;
  const double *qacc;
  double thr;
  SliceRec *slices;        // kFusePairs per workgroup
  int32_t *slice_count;    // records in each slice
  unsigned long long *nseed; // [0] += seeds, [1] = max(., length of the longest hit kept)
  int qcap;
};

constexpr int kFusePer = kFusePairs / kBlock;
static_assert(kFusePer * kBlock == kFusePairs, "pairs per workgroup");
static_assert(kFusePairs <= 65536 && kPairLocalBits <= 5, "a tile's order: 16-bit places, the buckets scanned by half a wavefront");
// the candidate of sorted pair x
template <bool kNarrow> __device__ __forceinline__ int sorted_pair_cand(const FuseArgs &f, int64_t x) {
  if constexpr (kNarrow) return pair_cand(static_cast<const uint32_t *>(f.vals)[x]);
  else return pair_cand(static_cast<const uint64_t *>(f.vals)[x]);
}
// The order of a tile lives in LDS as 2048 16-bit places (4 KB), not as the pairs themselves (16 KB): with the tables
// and a 2 kb query a workgroup holds 25.5 KB, five workgroups per CU is what the registers allow, and 41.5 KB would
// leave three.  The pairs are read again through the places; the tile's 16 KB were read a moment before.
template <int kAhead, bool kNarrow>
__global__ __launch_bounds__(kBlock) void k_seed_extend(FuseArgs f, QBatchDev qb, PageDev pg, SearchConst sc, ExtOpts o) {
  extern __shared__ __align__(16) uint8_t ungapped_smem[];
  __shared__ int32_t s_tab[kUtTotal];
  __shared__ unsigned s_kept, s_seeds, s_maxlen;
  __shared__ uint16_t s_place[kNarrow ? kFusePairs : 1];
  __shared__ unsigned s_bucket[kNarrow ? 1 << kPairLocalBits : 1];
  const int64_t b0 = (int64_t)blockIdx.x * kFusePairs;
  if (b0 >= f.npairs) return;
  const int64_t b1 = (b0 + kFusePairs < f.npairs ? b0 + kFusePairs : f.npairs) - 1;
  if (threadIdx.x == 0) {
    s_kept = 0;
    s_seeds = 0;
    s_maxlen = 0;
  }
  if constexpr (kNarrow)
    if (f.lbits > 0 && threadIdx.x < (1 << kPairLocalBits)) s_bucket[threadIdx.x] = 0;
  for (int t = threadIdx.x; t < kUtTotal; t += kBlock)
    s_tab[t] = t < kUtInternal   ? sc.stack37[t]
               : t < kUtMismatch ? sc.internal37[t - kUtInternal]
               : t < kUtInt11    ? sc.mismatchI37[t - kUtMismatch]
                                 : sc.int11[t - kUtInt11];
  const UngappedTabs tabs{s_tab + kUtStack, s_tab + kUtInternal, s_tab + kUtMismatch, s_tab + kUtInt11, sc.int22};
  // the pairs are sorted by query first: one query for the whole workgroup unless it sits on a boundary (the first and
  // the last pair as the sort left them: behind the tile's own ordering the queries of such a tile interleave)
  const int q0 = f.cands[sorted_pair_cand<kNarrow>(f, b0)].query;
  const int nslots = qb.len[q0] + 1;
  const bool staged = q0 == f.cands[sorted_pair_cand<kNarrow>(f, b1)].query && nslots <= f.qcap; // uniform over the workgroup
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
  const int ntile = (int)(b1 - b0) + 1;
  bool placed = false; // s_place[0 .. ntile) = the tile's pairs in bucket order (uniform over the workgroup)
  if constexpr (kNarrow) {
    placed = f.lbits > 0;
    if (placed) { // a counting sort of the tile on key bits [lshift, lshift + lbits): count, scan, place
      const unsigned bmask = (1u << f.lbits) - 1;
      unsigned bucket[kFusePer];
#pragma unroll
      for (int it = 0; it < kFusePer; it++) {
        const int i = it * kBlock + threadIdx.x;
        bucket[it] = 0;
        if (i < ntile) {
          bucket[it] = (f.keys[b0 + i] >> f.lshift) & bmask;
          atomicAdd(&s_bucket[bucket[it]], 1u);
        }
      }
      __syncthreads();
      if (threadIdx.x < 64) { // exclusive scan of the counts
        const unsigned cnt = lane < (1 << kPairLocalBits) ? s_bucket[lane] : 0;
        unsigned incl = cnt;
        for (int d = 1; d < (1 << kPairLocalBits); d <<= 1) {
          const unsigned up = (unsigned)__shfl_up((int)incl, d);
          if (lane >= d) incl += up;
        }
        if (lane < (1 << kPairLocalBits)) s_bucket[lane] = incl - cnt;
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < kFusePer; it++) {
        const int i = it * kBlock + threadIdx.x;
        if (i < ntile) s_place[atomicAdd(&s_bucket[bucket[it]], 1u)] = (uint16_t)i;
      }
      __syncthreads();
    }
  }
  SliceRec *slice = f.slices + b0;
  unsigned nseed = 0, maxlen = 0; // (the longest hit kept: the sort behind this packs the lengths into as many bits)
  for (int it = 0; it < kFusePer; it++) {
    const int i = it * kBlock + threadIdx.x; // (places beyond the tile's pairs are not filled: i < ntile comes first)
    bool keep = false;
    WalkHit w{};
    int query = 0;
    if (i < ntile) {
      int64_t x = b0 + i;
      int db_sp, jrel, ci;
      if constexpr (kNarrow) {
        if (placed) x = b0 + s_place[i];
        const uint32_t v = static_cast<const uint32_t *>(f.vals)[x];
        db_sp = (int)(f.keys[x] & ((1u << f.pbits) - 1));
        jrel = (int)(v >> kPairCandBits);
        ci = pair_cand(v);
      } else {
        const uint64_t v = static_cast<const uint64_t *>(f.vals)[x];
        db_sp = (int)(uint32_t)v;
        jrel = (int)(v >> (32 + kPairCandBits));
        ci = pair_cand(v);
      }
      const CandDev c = f.cands[ci];
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

// LDS slots per query array of a launch: the longest query of the batch, at most 7168 (9 B each: 63 KB per workgroup)
inline int query_lds_slots(int max_query_len) { return std::min((max_query_len + 1 + 3) & ~3, 7168); }

} // namespace

hipError_t launch_ungapped(HitSoA hits, int64_t n, const QBatchDev &qb, const PageDev &pg, const SearchConst &sc, ExtOpts o,
                           int max_query_len, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int qcap = query_lds_slots(max_query_len);
  const int64_t per_block = (int64_t)kBlock * kUngappedPer;
  hipLaunchKernelGGL(k_ungapped, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBlock), (size_t)qcap * 9, s, hits, n,
                     qb, pg, sc, o, qcap);
  return hipGetLastError();
}
hipError_t launch_blk_seq(const PageDev &pg, int32_t *blk_seq, hipStream_t s) {
  const int64_t nblk = blk_seq_entries(pg.nchars);
  hipLaunchKernelGGL(k_blk_seq, dim3((unsigned)((nblk + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pg, blk_seq, nblk);
  return hipGetLastError();
}
hipError_t launch_pair_keys(const CandDev *cands, const int64_t *pair0, int32_t ncand, int64_t npairs, const PageDev &pg, int qmin,
                            const PairLayout &lay, void *key, void *val, hipStream_t s) {
  if (lay.narrow)
    return launch_1d(k_pair_key<uint32_t, uint32_t>, npairs, kBlock, 0, s, cands, pair0, ncand, npairs, pg, qmin, 0, lay.pbits, (uint32_t *)key,
                     (uint32_t *)val);
  if (lay.wide_key())
    return launch_1d(k_pair_key<uint64_t, uint64_t>, npairs, kBlock, 0, s, cands, pair0, ncand, npairs, pg, qmin, lay.shift, lay.pbits,
                     (uint64_t *)key, (uint64_t *)val);
  return launch_1d(k_pair_key<uint32_t, uint64_t>, npairs, kBlock, 0, s, cands, pair0, ncand, npairs, pg, qmin, lay.shift, lay.pbits,
                   (uint32_t *)key, (uint64_t *)val);
}
hipError_t launch_allow_test(const CandDev *cands, const int64_t *pair0, const void *val, const PairLayout &lay, int64_t npairs,
                             const PageDev &pg, const AllowDev &allow, uint64_t *ballot, int32_t *count, hipStream_t s) {
  if (lay.narrow) return launch_1d(k_allow_test<uint32_t>, npairs, kBlock, 0, s, cands, pair0, (const uint32_t *)val, npairs, pg, allow, ballot, count);
  return launch_1d(k_allow_test<uint64_t>, npairs, kBlock, 0, s, cands, pair0, (const uint64_t *)val, npairs, pg, allow, ballot, count);
}
hipError_t launch_allow_scatter(const void *key_in, const void *val_in, int64_t npairs, const PairLayout &lay, const uint64_t *ballot,
                                const int64_t *off, void *key_out, void *val_out, hipStream_t s) {
  if (lay.narrow)
    return launch_1d(k_allow_scatter<uint32_t, uint32_t>, npairs, kBlock, 0, s, (const uint32_t *)key_in, (const uint32_t *)val_in, npairs, ballot,
                     off, (uint32_t *)key_out, (uint32_t *)val_out);
  if (lay.wide_key())
    return launch_1d(k_allow_scatter<uint64_t, uint64_t>, npairs, kBlock, 0, s, (const uint64_t *)key_in, (const uint64_t *)val_in, npairs, ballot,
                     off, (uint64_t *)key_out, (uint64_t *)val_out);
  return launch_1d(k_allow_scatter<uint32_t, uint64_t>, npairs, kBlock, 0, s, (const uint32_t *)key_in, (const uint64_t *)val_in, npairs, ballot, off,
                   (uint32_t *)key_out, (uint64_t *)val_out);
}
hipError_t launch_seed_extend(const CandDev *cands, const void *keys, const void *vals, const PairLayout &lay, int64_t npairs,
                              const QBatchDev &qb, const PageDev &pg, const SearchConst &sc, ExtOpts o, const double *qacc, double thr,
                              int max_query_len, void *slices, int32_t *slice_count, uint64_t *nseed, hipStream_t s) {
  if (npairs <= 0) return hipSuccess;
  const int qcap = query_lds_slots(max_query_len);
  const int lbits = lay.narrow ? std::min(lay.local_bits, kPairLocalBits) : 0;
  FuseArgs f{cands, lay.narrow ? static_cast<const uint32_t *>(keys) : nullptr, vals, lay.pbits, lay.begin - lbits, lbits, npairs, qacc, thr,
             static_cast<SliceRec *>(slices), slice_count, reinterpret_cast<unsigned long long *>(nseed), qcap};
  // (4, 5 or 6 positions fetched ahead instead of 8: the same 273-290 ms per configs[2] step)
  if (lay.narrow)
    hipLaunchKernelGGL((k_seed_extend<8, true>), dim3((unsigned)fused_slices(npairs)), dim3(kBlock), (size_t)qcap * 9, s, f, qb, pg, sc, o);
  else
    hipLaunchKernelGGL((k_seed_extend<8, false>), dim3((unsigned)fused_slices(npairs)), dim3(kBlock), (size_t)qcap * 9, s, f, qb, pg, sc, o);
  return hipGetLastError();
}
hipError_t launch_collect_slices(const void *slices, const int32_t *slice_count, const int64_t *slice_off, int64_t nslices, HitRec *out,
                                 hipStream_t s) {
  if (nslices <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_collect_slices, dim3((unsigned)nslices), dim3(kBlock), 0, s, static_cast<const SliceRec *>(slices), slice_count,
                     slice_off, out);
  return hipGetLastError();
}

} // namespace prb
