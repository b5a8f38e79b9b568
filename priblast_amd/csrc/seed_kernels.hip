// Seed expansion on gfx950: the seed candidates of a chunk (pairs of suffix-array intervals from the host's DFS) become
// the list of seed hits, a row = one (candidate, database SA entry) at a time.
//
//   k_seed<false> / <true> (count / emit), k_seed_qacc <-> SeedSearch::CalcInteractionEnergy, CalcAccessibility
//                                                                                  seed_search.cpp:47-99, 143-151
//   k_sa_seq                                           <-> SeedSearch::GetSeqIdAndStart  seed_search.cpp:101-141
//
// This is the list form of the seed path (PRB_SEED_FUSED=0, the seed-stage output, candidates too wide for the fused
// pass); ungapped_kernels.hip has the pass that goes from the pairs to extended hits at once.
#include "launch.hpp"
#include "search_device.hpp"
#include "search_kernels.hpp"

namespace prb {

namespace {

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
// `allow` (none, or one AllowDev - the instantiations without one are the kernels they were): a row whose (query, target)
// is not allowed counts no seed; the emit pass leaves out the rows that counted none.
template <bool kEmit, class... Allow>
__global__ __launch_bounds__(kBlock) void k_seed(const CandDev *__restrict__ cands, int ncand, int64_t nrows, QBatchDev qb,
                                                 PageDev pg, int delta, const double *__restrict__ qacc,
                                                 int32_t *__restrict__ row_count, int32_t *__restrict__ row_cand,
                                                 const int64_t *__restrict__ row_off, HitSoA hits,
                                                 const uint32_t *__restrict__ row_perm, Allow... allow) {
  static_assert(sizeof...(Allow) <= 1, "at most one mask");
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
  if constexpr (sizeof...(Allow) > 0) {
    if (kEmit) {
      if (row_off[slot + 1] == row_off[slot]) return; // (row_off has a total behind the last row)
    } else if (!(pair_allowed(allow, c.query, id) && ...)) {
      row_count[slot] = 0;
      return;
    }
  }
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

} // namespace

hipError_t launch_sa_seq(const PageDev &pg, int32_t *sa_seq, hipStream_t s) {
  return launch_1d(k_sa_seq, pg.nchars, kBlock, 0, s, pg, sa_seq);
}
hipError_t launch_seed_qacc(const CandDev *cands, int32_t ncand, int64_t nq_entries, const QBatchDev &qb, int delta, double *qacc,
                            hipStream_t s) {
  return launch_1d(k_seed_qacc, nq_entries, kBlock, 0, s, cands, ncand, nq_entries, qb, delta, qacc);
}
hipError_t launch_row_keys(const CandDev *cands, int32_t ncand, int64_t nrows, const PageDev &pg, int qmin, int shift, int dbits,
                           bool wide, int32_t *row_cand, void *key, uint32_t *val, hipStream_t s) {
  if (wide)
    return launch_1d(k_row_key<uint64_t>, nrows, kBlock, 0, s, cands, ncand, nrows, pg, qmin, shift, dbits, row_cand, (uint64_t *)key, val);
  return launch_1d(k_row_key<uint32_t>, nrows, kBlock, 0, s, cands, ncand, nrows, pg, qmin, shift, dbits, row_cand, (uint32_t *)key, val);
}
hipError_t launch_seed_count(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                             int delta, const double *qacc, int32_t *row_count, int32_t *row_cand, const uint32_t *row_perm,
                             hipStream_t s) {
  return launch_1d(k_seed<false>, nrows, kBlock, 0, s, cands, ncand, nrows, qb, pg, delta, qacc, row_count, row_cand,
                   (const int64_t *)nullptr, HitSoA{}, row_perm);
}
hipError_t launch_seed_emit(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                            int delta, const double *qacc, const int32_t *row_cand, const int64_t *row_off, HitSoA hits,
                            const uint32_t *row_perm, hipStream_t s) {
  return launch_1d(k_seed<true>, nrows, kBlock, 0, s, cands, ncand, nrows, qb, pg, delta, qacc, (int32_t *)nullptr,
                   const_cast<int32_t *>(row_cand), row_off, hits, row_perm);
}
hipError_t launch_seed_count_allowed(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                                     int delta, const double *qacc, int32_t *row_count, int32_t *row_cand, const uint32_t *row_perm,
                                     const AllowDev &allow, hipStream_t s) {
  return launch_1d(k_seed<false, AllowDev>, nrows, kBlock, 0, s, cands, ncand, nrows, qb, pg, delta, qacc, row_count, row_cand,
                   (const int64_t *)nullptr, HitSoA{}, row_perm, allow);
}
hipError_t launch_seed_emit_allowed(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                                    int delta, const double *qacc, const int32_t *row_cand, const int64_t *row_off, HitSoA hits,
                                    const uint32_t *row_perm, const AllowDev &allow, hipStream_t s) {
  return launch_1d(k_seed<true, AllowDev>, nrows, kBlock, 0, s, cands, ncand, nrows, qb, pg, delta, qacc, (int32_t *)nullptr,
                   const_cast<int32_t *>(row_cand), row_off, hits, row_perm, allow);
}

} // namespace prb
