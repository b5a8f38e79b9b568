// C ABI, part 3: the search of one page (SearchSeed / ExtendWithoutGap / ExtendWithGap,
// rna_interaction_search.cpp:264-320).  search_page cuts a batch into sub-batches of queries; search_range takes one
// sub-batch through the stages of DESIGN.md section 1, one function per stage over the sub-batch's state (SubSearch,
// search_stages.hpp).  The gapped stage's is in capi_gapped.hip.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "search_stages.hpp"

using namespace prb;

namespace prb {

// ------------------------------------------------------------------------- knobs
static bool env_off(const char *e) { return e && atoi(e) == 0; }
static SearchKnobs read_search_knobs() {
  SearchKnobs k;
  const char *e;
  e = getenv("PRB_SEARCH_PAIRS");
  k.budget = e ? atof(e) : 4.0e8;
  k.chunk_pairs = k.budget;
  if ((e = getenv("PRB_SEARCH_CHUNK_PAIRS"))) k.chunk_pairs = atof(e);
  e = getenv("PRB_SEED_ROW_SHIFT");
  k.row_shift = e ? std::min(atoi(e), 30) : 7;
  e = getenv("PRB_SEED_SORT_BITS");
  k.sort_bits = e ? std::max(atoi(e), 1) : 16;
  k.local_order = !env_off(getenv("PRB_SEED_LOCAL_ORDER"));
  e = getenv("PRB_SEED_PAIR_WIDE");
  k.pair_wide = e && atoi(e) != 0;
  k.fused = !env_off(getenv("PRB_SEED_FUSED"));
  k.front_ahead = !getenv("PRB_NO_FRONT_AHEAD");
  k.sort_four_keys = getenv("PRB_SORT_FOUR_KEYS") != nullptr;
  k.sort_two_lengths = getenv("PRB_SORT_TWO_LENGTHS") != nullptr;
  e = getenv("PRB_BIG_LIST_BYTES");
  k.big_list_bytes = e ? (size_t)atof(e) : (size_t)20 << 30;
  e = getenv("PRB_GAPPED_CHUNK_HITS");
  k.gapped_chunk_hits = e ? std::max<int64_t>(1, (int64_t)atof(e)) : 120000000;
  e = getenv("PRB_GAPPED_FIRST_TIER");
  k.first_tier = e ? std::min(std::max(atoi(e), 0), kWaveTier) : 0;
  k.wave_hbm = getenv("PRB_GAPPED_WAVE_HBM") != nullptr;
  k.no_resume = getenv("PRB_GAPPED_NO_RESUME") != nullptr;
  e = getenv("PRB_GAPPED_RESUME_CAP");
  k.resume_cap = e ? std::max(1, atoi(e)) : 0;
  k.front_paired = getenv("PRB_GAPPED_FRONT_PAIRED") != nullptr;
  e = getenv("PRB_GAPPED_SKIP_TIERS");
  k.skip_tiers = e ? atoi(e) : 0;
  k.front = !env_off(getenv("PRB_GAPPED_FRONT"));
  k.handover = !env_off(getenv("PRB_GAPPED_HANDOVER"));
  k.tiers.pair = !env_off(getenv("PRB_GAPPED_PAIR"));
  k.tiers.pool = !env_off(getenv("PRB_GAPPED_POOL"));
  GapTierKnobs &t = k.tiers;
  if ((e = getenv("PRB_GAPPED_LDS_PAD"))) sscanf(e, "%d,%d,%d", &t.pad[1], &t.pad[2], &t.pad[3]);
  t.pad_set = e != nullptr;
  if ((e = getenv("PRB_GAPPED_PERIOD"))) sscanf(e, "%d,%d,%d,%d", &t.period[0], &t.period[1], &t.period[2], &t.period[3]);
  t.period_set = e != nullptr;
  if ((e = getenv("PRB_GAPPED_EARLY"))) sscanf(e, "%d,%d,%d,%d", &t.early[0], &t.early[1], &t.early[2], &t.early[3]);
  t.early_set = e != nullptr;
  k.filter_tiles = !env_off(getenv("PRB_FILTER_TILES"));
  k.trace_no_long = getenv("PRB_TRACE_NO_LONG") != nullptr;
  e = getenv("PRB_TRACE_LONG_CAP");
  k.trace_long_cap = e ? std::max(1, atoi(e)) : 1024;
  k.trace_no_slots = getenv("PRB_TRACE_NO_SLOTS") != nullptr;
  e = getenv("PRB_TRACE_SLOT_CAP");
  k.trace_slot_cap = e ? std::min(kTraceCap, atoi(e)) : kTraceCap;
  e = getenv("PRB_DISTINCT_LDS_HITS");
  k.distinct_lds_hits = e ? atoi(e) : kSiteLdsHits;
  e = getenv("PRB_CHAIN_LDS_HITS");
  k.chain_lds_hits = e ? atoi(e) : kChainLdsHits;
  k.debug_rows = getenv("PRB_DEBUG_ROWS") != nullptr;
  k.debug_mem = getenv("PRB_DEBUG_MEM") != nullptr;
  return k;
}

// ------------------------------------------------------------------------- lists of hits (search_stages.hpp)
HitSoA carve_hits(uint8_t *p, int64_t n) {
  HitSoA h;
  const size_t n8 = ((size_t)n + 1) & ~(size_t)1; // keep the double arrays 8-byte aligned
  h.e_acc = reinterpret_cast<double *>(p);
  h.e_hyb = h.e_acc + n8;
  h.e_tot = h.e_hyb + n8;
  int32_t *ip = reinterpret_cast<int32_t *>(h.e_tot + n8);
  h.q_sp = ip;
  h.db_sp = ip + n8;
  h.q_len = ip + 2 * n8;
  h.db_len = ip + 3 * n8;
  h.db_id = ip + 4 * n8;
  h.db_id_start = ip + 5 * n8;
  h.query = ip + 6 * n8;
  return h;
}

// the radix sorts of the tables' merges (search_host.hpp)
int sort_target_keys(hipStream_t s, DevBuf &tmp, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits) {
  return sort_pairs(s, tmp, kin, kout, vin, vout, n, bits);
}
hipError_t sort_span_keys(void *tmp, size_t &bytes, uint64_t *kin, uint64_t *kout, uint32_t *vin, uint32_t *vout, size_t n, int bits, hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0, bits, s);
}

// Sorts the records `recs` (n hits) into `out` by the reference's comparator made total:
// (query, db_sp asc, q_sp asc, db_len desc, q_len desc, energy asc, hybridization part asc, accessibility part asc,
// input order).  perm_out[i] = index in `recs`.  form (optional): which form of the sort gave the order, a PRB_SORT_* of
// include/priblast_hip.h.
static int sort_hits(prb_ctx *ctx, SearchWs &w, const SearchKnobs &k, const HitRec *recs, HitSoA out, int64_t n, const SortBounds &sb,
                     uint32_t **perm_out, int32_t *form = nullptr) {
  int rc;
  int32_t why = PRB_SORT_GENERAL_FORCED;
  const size_t N = (size_t)n;
  {
    // one stable radix sort over a packed key + a pass over the runs of identical coordinates
    PackedKeyInfo f;
    f.qmin = sb.qmin;
    f.one_len = sb.eq_len_max > 0;
    f.lmax = f.one_len ? sb.eq_len_max : std::max(sb.max_qlen, sb.max_dblen);
    f.bl = bits_for(f.lmax);
    f.bq = bits_for(sb.max_qlen);
    f.bd = bits_for(sb.nchars);
    const int total = (f.one_len ? 1 : 2) * f.bl + f.bq + f.bd + bits_for(sb.qspan - 1);
    if (!k.sort_four_keys) why = PRB_SORT_GENERAL_WIDTH;
    if (total <= 64 && f.lmax <= 65535 && !k.sort_four_keys) {
      if ((rc = w.kP.ensure(N * 8)) || (rc = w.kTmp2.ensure(N * 8)) || (rc = w.kE.ensure(N * 8)) || (rc = w.kTmp.ensure(N * 8)) ||
          (rc = w.idxA.ensure(N * 4)) || (rc = w.idxB.ensure(N * 4)) || (rc = w.pending.ensure(16)))
        return rc;
      PRB_HIP(launch_make_packed_keys_recs(recs, n, f, w.kP.as<uint64_t>(), w.kE.as<uint64_t>(), w.idxA.as<uint32_t>(), ctx->stream));
      if ((rc = sort_pairs(ctx->stream, w.sortTmp, w.kP.as<uint64_t>(), w.kTmp2.as<uint64_t>(), w.idxA.as<uint32_t>(),
                           w.idxB.as<uint32_t>(), N, (unsigned)total)))
        return rc;
      PRB_HIP(launch_gather_u64(w.kE.as<uint64_t>(), w.idxB.as<uint32_t>(), w.kTmp.as<uint64_t>(), n, ctx->stream));
      PRB_HIP(hipMemsetAsync(w.pending.p, 0, 4, ctx->stream));
      PRB_HIP(launch_fix_ties(w.kTmp2.as<uint64_t>(), w.kTmp.as<uint64_t>(), w.idxB.as<uint32_t>(), n, recs, w.idxA.as<uint32_t>(),
                              w.pending.as<int32_t>(), ctx->stream));
      int32_t too_long = 0;
      PRB_HIP(hipMemcpyAsync(&too_long, w.pending.p, 4, hipMemcpyDeviceToHost, ctx->stream));
      PRB_HIP(hipStreamSynchronize(ctx->stream));
      if (!too_long) {
        PRB_HIP(launch_gather_recs_to_hits(recs, w.idxA.as<uint32_t>(), out, n, ctx->stream));
        *perm_out = w.idxA.as<uint32_t>();
        if (form) *form = f.one_len ? PRB_SORT_PACKED_ONE_LENGTH : PRB_SORT_PACKED_TWO_LENGTHS;
        return PRB_OK;
      }
      why = PRB_SORT_GENERAL_TIE_RUN;
    }
  }
  if (form) *form = why;
  // The general form works on the fields as arrays.  LSD: one stable radix sort per key, least significant first.
  if (k.debug_mem) fprintf(stderr, "[mem] sort: the general form (%lld hits)\n", (long long)n);
  if ((rc = w.hitsTmp.ensure(hits_bytes(n)))) return rc;
  const HitSoA in = carve_hits(w.hitsTmp, n);
  PRB_HIP(launch_gather_recs_to_hits(recs, nullptr, in, n, ctx->stream));
  if ((rc = w.kE.ensure(N * 8)) || (rc = w.kL.ensure(N * 4)) || (rc = w.kQ.ensure(N * 4)) || (rc = w.kP.ensure(N * 8)) ||
      (rc = w.kTmp.ensure(N * 8)) || (rc = w.kTmp2.ensure(N * 8)) || (rc = w.idxA.ensure(N * 4)) ||
      (rc = w.idxB.ensure(N * 4)))
    return rc;
  PRB_HIP(launch_make_keys(in, n, w.kE.as<uint64_t>(), w.kL.as<uint32_t>(), w.kQ.as<uint32_t>(), w.kP.as<uint64_t>(),
                           w.idxA.as<uint32_t>(), ctx->stream));
  uint32_t *ia = w.idxA.as<uint32_t>(), *ib = w.idxB.as<uint32_t>();
  auto sort_step = [&](auto *keys, unsigned bits) -> int { // (keys of 64 or 32 bits)
    using K = std::remove_pointer_t<decltype(keys)>;
    if (int r = sort_pairs(ctx->stream, w.sortTmp, keys, w.kTmp2.as<K>(), ia, ib, N, bits)) return r;
    std::swap(ia, ib);
    return PRB_OK;
  };
  // least significant first: accessibility part, hybridization part, energy
  PRB_HIP(launch_order_keys(in.e_acc, n, w.kTmp.as<uint64_t>(), ctx->stream));
  if ((rc = sort_step(w.kTmp.as<uint64_t>(), 64))) return rc; // keys in input order
  PRB_HIP(launch_order_keys(in.e_hyb, n, w.kTmp2.as<uint64_t>(), ctx->stream));
  PRB_HIP(launch_gather_u64(w.kTmp2.as<uint64_t>(), ia, w.kTmp.as<uint64_t>(), n, ctx->stream));
  if ((rc = sort_step(w.kTmp.as<uint64_t>(), 64))) return rc;
  PRB_HIP(launch_gather_u64(w.kE.as<uint64_t>(), ia, w.kTmp.as<uint64_t>(), n, ctx->stream));
  if ((rc = sort_step(w.kTmp.as<uint64_t>(), 64))) return rc;
  PRB_HIP(launch_gather_u32(w.kL.as<uint32_t>(), ia, w.kTmp.as<uint32_t>(), n, ctx->stream));
  if ((rc = sort_step(w.kTmp.as<uint32_t>(), 32))) return rc;
  PRB_HIP(launch_gather_u32(w.kQ.as<uint32_t>(), ia, w.kTmp.as<uint32_t>(), n, ctx->stream));
  if ((rc = sort_step(w.kTmp.as<uint32_t>(), 32))) return rc;
  PRB_HIP(launch_gather_u64(w.kP.as<uint64_t>(), ia, w.kTmp.as<uint64_t>(), n, ctx->stream));
  unsigned qbits = 1;
  while ((int64_t(1) << qbits) < (int64_t)sb.qmin + sb.qspan && qbits < 31) qbits++; // (the queries of the list are below that)
  if ((rc = sort_step(w.kTmp.as<uint64_t>(), 32 + qbits))) return rc;
  PRB_HIP(launch_gather_hits(in, ia, out, n, ctx->stream));
  *perm_out = ia;
  return PRB_OK;
}

struct MaxOp {
  __host__ __device__ int64_t operator()(const int64_t &a, const int64_t &b) const { return a > b ? a : b; }
};

// CheckRedundancy on the sorted list `h`; writes the indices of the survivors (ascending) to
// w.surv and returns their number.
static int filter_hits(prb_ctx *ctx, SearchWs &w, const HitSoA &h, int64_t n, double thr, bool tiles, int64_t *nsurv) {
  int rc;
  const size_t N = (size_t)n;
  *nsurv = 0;
  if (n == 0) return PRB_OK;
  if ((rc = w.endKey.ensure(N * 8)) || (rc = w.pmax.ensure(N * 8)) || (rc = w.state.ensure(N)) || (rc = w.keep.ensure(N)) ||
      (rc = w.pending.ensure(16)) || (rc = w.surv.ensure(N * 4)) || (rc = w.count.ensure(16)))
    return rc;
  PRB_HIP(launch_filter_init(h, n, thr, w.endKey.as<int64_t>(), w.state.as<uint8_t>(), ctx->stream));
  if ((rc = with_temp(w.scanTmp, "rocprim::inclusive_scan", [&](void *t, size_t &b) {
         return rocprim::inclusive_scan(t, b, w.endKey.as<int64_t>(), w.pmax.as<int64_t>(), N, MaxOp(), ctx->stream);
       })))
    return rc;
  for (int round = 0;; round++) {
    PRB_HIP(hipMemsetAsync(w.pending.p, 0, 4, ctx->stream));
    PRB_HIP(launch_filter_round(h, n, w.pmax.as<int64_t>(), w.state.as<uint8_t>(), w.pending.as<int32_t>(), tiles, ctx->stream));
    int32_t pend = 0;
    PRB_HIP(hipMemcpyAsync(&pend, w.pending.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    if (!pend) break;
    if (round > 100000) {
      set_error("redundancy filter did not converge");
      return PRB_ERR_STATE;
    }
  }
  PRB_HIP(launch_filter_final(h, n, w.pmax.as<int64_t>(), w.state.as<uint8_t>(), w.keep.as<uint8_t>(), tiles, ctx->stream));
  return select_flagged(ctx, w, nullptr, w.keep.as<uint8_t>(), w.surv.as<uint32_t>(), N, nsurv);
}

// PRB_DEBUG_MEM: free device memory at the stations of a search
static void mem_note(const char *where, const SearchWs &w) {
  static const bool on = getenv("PRB_DEBUG_MEM") != nullptr;
  if (!on) return;
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  fprintf(stderr, "[mem] %-18s free %7zu MiB | hitsA %6zu hitsB %6zu hitsC %6zu hitsTmp %6zu MiB\n", where, free_b >> 20, w.hitsA.cap >> 20,
          w.hitsB.cap >> 20, w.hitsC.cap >> 20, w.hitsTmp.cap >> 20);
}

// `need` bytes in a buffer whose first `have` bytes are kept.  (Grown with room to spare while memory allows: every
// growth is a copy of everything, and a list of 1e9 records - 64 GB - must still be able to grow next to its old copy.
// `spare_limit`: beyond that only a sixth - what is spare here is missing in whatever comes behind.)
int grow_keep(prb_ctx *ctx, DevBuf &buf, size_t have, size_t need, size_t spare_limit) {
  int rc;
  if (have > 0 && need > buf.cap) {
    DevBuf bigger;
    if ((rc = need > spare_limit ? PRB_ERR_NOMEM : bigger.ensure(need + need / 2)) && (rc = bigger.ensure(need + need / 6)) &&
        (rc = bigger.ensure(need)))
      return rc;
    PRB_HIP(hipMemcpyAsync(bigger.p, buf.p, have, hipMemcpyDeviceToDevice, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    buf.release();
    buf = bigger;
    return PRB_OK;
  }
  return buf.ensure(need);
}
// Room for `more` records behind the `have` records that `recbuf` holds (which are kept).  (Past 16 GB the list is
// grown with little to spare: the sort behind needs the memory.)
static int reserve_recs(prb_ctx *ctx, DevBuf &recbuf, int64_t have, int64_t more) {
  return grow_keep(ctx, recbuf, (size_t)have * sizeof(HitRec), ((size_t)have + (size_t)more) * sizeof(HitRec), (size_t)16 << 30);
}

// Drops the hits whose energy is above `thr` (they cannot survive CheckRedundancy nor influence
// it, see k_flag_not_above): recbuf <- the kept hits of `in`, in order, as records for the sort that
// follows; idxbuf[i] = index in `in`.
// `have` records already in recbuf are kept (the new ones are appended behind them).
int compact_below(prb_ctx *ctx, SearchWs &w, const HitSoA &in, int64_t n, double thr, DevBuf &idxbuf, DevBuf &recbuf, int64_t *m,
                  int64_t have) {
  int rc;
  *m = 0;
  if (n == 0) return PRB_OK;
  const size_t N = (size_t)n;
  if ((rc = w.keep.ensure(N)) || (rc = idxbuf.ensure(N * 4)) || (rc = w.count.ensure(16))) return rc;
  PRB_HIP(launch_flag_not_above(in.e_tot, n, thr, w.keep.as<uint8_t>(), ctx->stream));
  if ((rc = select_flagged(ctx, w, nullptr, w.keep.as<uint8_t>(), idxbuf.as<uint32_t>(), N, m))) return rc;
  if ((rc = reserve_recs(ctx, recbuf, have, std::max<int64_t>(*m, 1)))) return rc;
  PRB_HIP(launch_gather_hits_to_recs(in, idxbuf.as<uint32_t>(), recbuf.as<HitRec>() + have, *m, ctx->stream));
  return PRB_OK;
}

static int download_hits(prb_ctx *ctx, SearchWs &w, const HitSoA &h, int64_t n, std::vector<prb_hit> &out) {
  HostTimer ht(ctx, "host_download");
  const size_t base = out.size();
  if (n == 0) return PRB_OK;
  int rc;
  const size_t bytes = (size_t)n * sizeof(prb_hit);
  if ((rc = w.packed.ensure(bytes)) || (rc = w.pinned.ensure(bytes))) return rc;
  PRB_HIP(launch_pack_hits(h, n, nullptr, nullptr, -1, w.packed.p, ctx->stream));
  PRB_HIP(hipMemcpyAsync(w.pinned.p, w.packed.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (out.capacity() < base + (size_t)n) out.reserve(std::max(2 * out.capacity(), base + (size_t)n));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  const prb_hit *src = static_cast<const prb_hit *>(w.pinned.p);
  out.insert(out.end(), src, src + n);
  return PRB_OK;
}

// ------------------------------------------------------------------------- seeds -> hits under -f
// Candidates [c0, c1) of a sub-batch = its next chunk: as many as fit the pair budget (and the one-pass form's record)
static int32_t chunk_end(const CandDev *cd, int32_t ncand, int32_t c0, double chunk_pairs, double *pairs_out) {
  int32_t c1 = c0;
  double acc = 0;
  while (c1 < ncand) {
    const double pairs = (double)(cd[c1].ep_q - cd[c1].sp_q + 1) * (double)(cd[c1].ep_db - cd[c1].sp_db + 1);
    if (c1 > c0 && (acc + pairs > chunk_pairs || c1 - c0 >= kMaxFusedCands)) break;
    acc += pairs;
    c1++;
  }
  *pairs_out = acc;
  return c1;
}

// (query, database position >> row_shift) keys of a chunk's rows or pairs (k_row_key): the bits of the position part
// and of the whole key, and the lowest bit that the sort looks at (above 0 in the narrow layout of the pairs only)
struct RowKeyBits {
  int dbits, kbits;
  int begin = 0;
  bool wide() const { return kbits > 32; }
};
static RowKeyBits row_key_bits(const PageDev &pd, int row_shift, const CandDev *cd, int32_t nc) {
  const int dbits = bits_for(std::max<int64_t>(1, ((int64_t)pd.nchars - 1) >> row_shift));
  return RowKeyBits{dbits, dbits + bits_for(std::max<int64_t>(1, (int64_t)cd[nc - 1].query - cd[0].query))};
}
// the sort by those keys, which are 32 bits wide unless they need more
template <class V>
static int sort_by_row_key(hipStream_t s, DevBuf &tmp, const RowKeyBits &kb, DevBuf &kin, DevBuf &kout, const V *vin, V *vout, size_t n) {
  return kb.wide() ? sort_pairs(s, tmp, kin.as<uint64_t>(), kout.as<uint64_t>(), vin, vout, n, (unsigned)kb.begin, (unsigned)kb.kbits)
                   : sort_pairs(s, tmp, kin.as<uint32_t>(), kout.as<uint32_t>(), vin, vout, n, (unsigned)kb.begin, (unsigned)kb.kbits);
}
// a chunk's pairs in the layout `lay`, from (kin, vin) to (kout, vout)
static int sort_chunk_pairs(hipStream_t s, DevBuf &tmp, const PairLayout &lay, DevBuf &kin, DevBuf &kout, DevBuf &vin, DevBuf &vout, size_t n) {
  const RowKeyBits kb{lay.pbits, lay.kbits, lay.begin};
  return lay.narrow ? sort_by_row_key(s, tmp, kb, kin, kout, vin.as<uint32_t>(), vout.as<uint32_t>(), n)
                    : sort_by_row_key(s, tmp, kb, kin, kout, vin.as<uint64_t>(), vout.as<uint64_t>(), n);
}

// w.row_off[0..n] <- the exclusive scan of the counts w.row_count[0..n] (the last one a zero: row_off[n] is the total)
static int scan_row_counts(prb_ctx *ctx, SearchWs &w, int64_t n) {
  auto in = rocprim::make_transform_iterator(w.row_count.as<int32_t>(), ToI64());
  return with_temp(w.scanTmp, "rocprim::exclusive_scan", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, in, w.row_off.as<int64_t>(), (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), ctx->stream);
  });
}

// The front of the one-pass seed path (SearchWs::FrontStage) for the chunk whose candidates - row0 / qoff relative to
// the chunk - are the nc entries at cd (page-locked): everything is issued on `s`.  *np_out = its pairs, or -1 when a
// candidate has more query entries than a pair's value has bits for (nothing is issued then: the list form takes it).
// Under a pair mask (`allow`) the pairs that are not allowed are dropped behind their keys: a test, a scan over one count
// per 64 pairs and a scatter, in a bracket of the "allow" timer when the caller has the "seed" bracket open on `s`
// (`timed`).  The sort needs the number of pairs left, which is on its way to the host: finish_front does it.
static int issue_front(SearchWs &w, const prb_qbatch *qb, const PageDev &pd, int delta, const SearchKnobs &k, const CandDev *cd, int32_t nc,
                       int64_t cents, hipStream_t s, int64_t *np_out, const AllowDev *allow, prb_ctx *timed) {
  SearchWs::FrontStage &F = w.front;
  int rc;
  *np_out = -1;
  if ((rc = F.pair0_pin.ensure(((size_t)nc + 1) * 8))) return rc;
  int64_t *pair0 = static_cast<int64_t *>(F.pair0_pin.p);
  int64_t np = 0;
  for (int32_t c = 0; c < nc; c++) {
    const int64_t qw = cd[c].ep_q - cd[c].sp_q + 1;
    if (qw > kMaxFusedEntries) return PRB_OK;
    pair0[c] = np;
    np += qw * (int64_t)(cd[c].ep_db - cd[c].sp_db + 1);
  }
  pair0[nc] = np;
  const size_t NP = (size_t)np;
  const PairLayout lay = pair_layout(pd.nchars, (int64_t)cd[nc - 1].query - cd[0].query, k.row_shift, k.sort_bits, k.local_order, k.pair_wide);
  if ((rc = F.cands.ensure((size_t)nc * sizeof(CandDev))) || (rc = F.seed_qacc.ensure((size_t)std::max<int64_t>(cents, 1) * 8)) ||
      (rc = F.pair0.ensure(((size_t)nc + 1) * 8)) || (rc = F.keyA.ensure(NP * lay.key_bytes())) || (rc = F.keyB.ensure(NP * lay.key_bytes())) ||
      (rc = F.valA.ensure(NP * lay.val_bytes())) || (rc = F.valB.ensure(NP * lay.val_bytes())))
    return rc;
  PRB_HIP(hipMemcpyAsync(F.cands.p, cd, (size_t)nc * sizeof(CandDev), hipMemcpyHostToDevice, s));
  PRB_HIP(hipMemcpyAsync(F.pair0.p, pair0, ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, s));
  PRB_HIP(launch_seed_qacc(F.cands.as<CandDev>(), nc, cents, qb->view, delta, F.seed_qacc.as<double>(), s));
  PRB_HIP(launch_pair_keys(F.cands.as<CandDev>(), F.pair0.as<int64_t>(), nc, np, pd, cd[0].query, lay, F.keyA.p, F.valA.p, s));
  F.unsorted = false;
  F.np_all = np;
  F.lay = lay;
  F.keys = F.keyB.p;
  F.vals = F.valB.p;
  if (allow) {
    const int64_t nw = allow_words(np);
    if ((rc = F.ballot.ensure((size_t)nw * 8)) || (rc = F.wcount.ensure((size_t)(nw + 1) * 4)) || (rc = F.woff.ensure((size_t)(nw + 1) * 8)) ||
        (rc = F.kept_pin.ensure(8)))
      return rc;
    if (timed && ((rc = timed->time_end("seed", 1)) || (rc = timed->time_begin()))) return rc; // (the keys; the sort is counted where it runs)
    PRB_HIP(hipMemsetAsync(F.wcount.as<int32_t>() + nw, 0, 4, s)); // (the scan over nw + 1 counts ends with the total)
    PRB_HIP(launch_allow_test(F.cands.as<CandDev>(), F.pair0.as<int64_t>(), F.valA.p, lay, np, pd, *allow, F.ballot.as<uint64_t>(),
                              F.wcount.as<int32_t>(), s));
    auto counts = rocprim::make_transform_iterator(F.wcount.as<int32_t>(), ToI64());
    if ((rc = with_temp(F.scanTmp, "rocprim::exclusive_scan", [&](void *t, size_t &b) {
           return rocprim::exclusive_scan(t, b, counts, F.woff.as<int64_t>(), (int64_t)0, (size_t)nw + 1, rocprim::plus<int64_t>(), s);
         })))
      return rc;
    PRB_HIP(launch_allow_scatter(F.keyA.p, F.valA.p, np, lay, F.ballot.as<uint64_t>(), F.woff.as<int64_t>(), F.keyB.p, F.valB.p, s));
    PRB_HIP(hipMemcpyAsync(F.kept_pin.p, F.woff.as<int64_t>() + nw, 8, hipMemcpyDeviceToHost, s));
    if (timed && ((rc = timed->time_end(ModeTimer::kAllow, 3)) || (rc = timed->time_begin()))) return rc;
    F.unsorted = true;
    *np_out = np;
    return PRB_OK;
  }
  if ((rc = sort_chunk_pairs(s, F.sortTmp, lay, F.keyA, F.keyB, F.valA, F.valB, NP))) return rc;
  *np_out = np;
  return PRB_OK;
}

// Under a pair mask: the front stage's pairs were compacted (issue_front, on the context's stream or waited for by it);
// *np = how many are left, sorted now - none: nothing is launched
static int finish_front(prb_ctx *ctx, SearchWs &w, const SearchKnobs &k, int32_t nc, int64_t *np) {
  SearchWs::FrontStage &F = w.front;
  int rc;
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  F.unsorted = false;
  const int64_t kept = *static_cast<const int64_t *>(F.kept_pin.p);
  if (kept < 0 || kept > F.np_all) {
    set_error("pair mask: " + std::to_string(kept) + " of " + std::to_string(F.np_all) + " pairs kept");
    return PRB_ERR_STATE;
  }
  if (k.debug_rows) fprintf(stderr, "[allow] cands %d pairs %lld allowed %lld\n", nc, (long long)F.np_all, (long long)kept);
  *np = kept;
  if (kept == 0) return PRB_OK;
  if ((rc = sort_chunk_pairs(ctx->stream, F.sortTmp, F.lay, F.keyB, F.keyA, F.valB, F.valA, (size_t)kept))) return rc;
  F.keys = F.keyA.p;
  F.vals = F.valA.p;
  return PRB_OK;
}

// a chunk of consecutive candidates [c0, c1) of the sub-batch (rebased: row0 / qoff count from the chunk's first)
struct SeedChunk {
  int32_t c0, c1, nc;
  int64_t crows, cents; // its database SA entries (rows) and query SA entries
  double pairs;
};

static int count_hits_under_f(SubSearch &s, int64_t more) {
  s.nf += more;
  if (s.nf > (int64_t)UINT32_MAX - 16) {
    set_error("more than 4e9 hits under the -f threshold in one sub-batch: build the database in smaller pages (db -c)");
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}

// Seeds -> hits under the -f threshold in one pass over the chunk's np sorted pairs (k_seed_extend), which the front
// stage holds: appended to the records in w.hitsB.  (Entered with the "seed" bracket open.)
static int seed_chunk_one_pass(SubSearch &s, const SeedChunk &c, int64_t np) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  SearchWs::FrontStage &F = w.front;
  int rc;
  if ((rc = w.count.ensure(16))) return rc;
  if ((rc = ctx->time_end("seed", s.allow ? 1 : 2))) return rc; // (under a pair mask the keys were counted in front of "allow")
  if ((rc = ctx->time_begin())) return rc;
  const int64_t nsl = fused_slices(np);
  if ((rc = w.hitsA.ensure((size_t)nsl * kFusePairs * kSliceRecBytes)) || (rc = w.row_count.ensure((size_t)(nsl + 1) * 4)) ||
      (rc = w.row_off.ensure((size_t)(nsl + 1) * 8)))
    return rc;
  PRB_HIP(hipMemsetAsync(w.count.p, 0, 16, ctx->stream));
  PRB_HIP(hipMemsetAsync(w.row_count.as<int32_t>() + nsl, 0, 4, ctx->stream));
  PRB_HIP(launch_seed_extend(F.cands.as<CandDev>(), F.keys, F.vals, F.lay, np, s.qb->view, s.pd, s.sc, s.eo, F.seed_qacc.as<double>(),
                             s.opts.interaction_threshold, s.max_qlen, w.hitsA.p, w.row_count.as<int32_t>(), w.count.as<uint64_t>(),
                             ctx->stream));
  if ((rc = scan_row_counts(ctx, w, nsl))) return rc;
  uint64_t kept = 0, seeds_maxlen[2] = {0, 0};
  PRB_HIP(hipMemcpyAsync(seeds_maxlen, w.count.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipMemcpyAsync(&kept, w.row_off.as<int64_t>() + nsl, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  s.one_pass_maxlen = std::max<int64_t>(s.one_pass_maxlen, (int64_t)seeds_maxlen[1]);
  if (kept > 0) {
    if ((rc = reserve_recs(ctx, w.hitsB, s.nf, (int64_t)kept))) return rc;
    PRB_HIP(launch_collect_slices(w.hitsA.p, w.row_count.as<int32_t>(), w.row_off.as<int64_t>(), nsl, w.hitsB.as<HitRec>() + s.nf,
                                  ctx->stream));
  }
  if ((rc = ctx->time_end("ungapped", 1))) return rc;
  s.hs->counts[0] += (int64_t)seeds_maxlen[0];
  if (s.k.debug_rows)
    fprintf(stderr, "[pairs] cands %d pairs %lld seeds %lld kept %lld\n", c.nc, (long long)np, (long long)seeds_maxlen[0], (long long)kept);
  return count_hits_under_f(s, (int64_t)kept);
}

// The list form of a chunk: seeds counted, written, extended and thinned in passes of their own
static int seed_chunk_lists(SubSearch &s, const SeedChunk &c) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const CandDev *cd = s.b.cd + c.c0;
  const int32_t nc = c.nc;
  const int64_t crows = c.crows, cents = c.cents;
  const int delta = s.eo.delta;
  int rc;
  s.all_one_pass = false;
  if ((rc = w.cands.ensure((size_t)nc * sizeof(CandDev))) || (rc = w.row_count.ensure((size_t)(crows + 1) * 4)) ||
      (rc = w.row_off.ensure((size_t)(crows + 1) * 8)) || (rc = w.row_cand.ensure((size_t)(crows + 1) * 4)) ||
      (rc = w.seed_qacc.ensure((size_t)std::max<int64_t>(cents, 1) * 8)))
    return rc;
  PRB_HIP(hipMemcpyAsync(w.cands.p, cd, (size_t)nc * sizeof(CandDev), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ctx->time_begin())) return rc;
  // one extra zero entry so that the exclusive scan over crows+1 values also yields the total
  PRB_HIP(hipMemsetAsync(w.row_count.as<int32_t>() + crows, 0, 4, ctx->stream));
  PRB_HIP(launch_seed_qacc(w.cands.as<CandDev>(), nc, cents, s.qb->view, delta, w.seed_qacc.as<double>(), ctx->stream));
  // the rows in the order of (query, database position) - not for the seed-stage output, which keeps the reference's
  // emission order (candidate, database SA entry, query SA entry) - see k_row_key
  const uint32_t *row_perm = nullptr;
  if (s.last_stage != 1 && crows > 1 && crows < (int64_t)UINT32_MAX && s.k.row_shift >= 0) {
    const size_t NR = (size_t)crows;
    const RowKeyBits kb = row_key_bits(s.pd, s.k.row_shift, cd, nc);
    if ((rc = w.kP.ensure(NR * 8)) || (rc = w.kTmp2.ensure(NR * 8)) || (rc = w.idxA.ensure(NR * 4)) || (rc = w.idxB.ensure(NR * 4)))
      return rc;
    PRB_HIP(launch_row_keys(w.cands.as<CandDev>(), nc, crows, s.pd, cd[0].query, s.k.row_shift, kb.dbits, kb.wide(), w.row_cand.as<int32_t>(),
                            w.kP.p, w.idxA.as<uint32_t>(), ctx->stream));
    if ((rc = sort_by_row_key(ctx->stream, w.sortTmp, kb, w.kP, w.kTmp2, w.idxA.as<uint32_t>(), w.idxB.as<uint32_t>(), NR))) return rc;
    row_perm = w.idxB.as<uint32_t>();
  }
  if (s.allow)
    PRB_HIP(launch_seed_count_allowed(w.cands.as<CandDev>(), nc, crows, s.qb->view, s.pd, delta, w.seed_qacc.as<double>(),
                                      w.row_count.as<int32_t>(), w.row_cand.as<int32_t>(), row_perm, *s.allow, ctx->stream));
  else
    PRB_HIP(launch_seed_count(w.cands.as<CandDev>(), nc, crows, s.qb->view, s.pd, delta, w.seed_qacc.as<double>(),
                              w.row_count.as<int32_t>(), w.row_cand.as<int32_t>(), row_perm, ctx->stream));
  if ((rc = scan_row_counts(ctx, w, crows))) return rc;
  int64_t nseed = 0;
  PRB_HIP(hipMemcpyAsync(&nseed, w.row_off.as<int64_t>() + crows, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  s.hs->counts[0] += nseed;
  if (s.k.debug_rows)
    fprintf(stderr, "[rows] cands %d rows %lld qents %lld pairs %.0f seeds %lld\n", nc, (long long)crows, (long long)cents, c.pairs, (long long)nseed);
  if (nseed == 0) return ctx->time_end("seed", 2);
  if (nseed > (int64_t)UINT32_MAX - 16) {
    set_error("too many seed hits in one chunk of candidates (a single candidate with more than 4e9 seed hits?): lower "
              "PRB_SEARCH_CHUNK_PAIRS");
    return PRB_ERR_NOMEM;
  }
  if ((rc = w.hitsA.ensure(hits_bytes(nseed)))) return rc;
  HitSoA A = carve_hits(w.hitsA, nseed);
  if (s.allow)
    PRB_HIP(launch_seed_emit_allowed(w.cands.as<CandDev>(), nc, crows, s.qb->view, s.pd, delta, w.seed_qacc.as<double>(),
                                     w.row_cand.as<int32_t>(), w.row_off.as<int64_t>(), A, row_perm, *s.allow, ctx->stream));
  else
    PRB_HIP(launch_seed_emit(w.cands.as<CandDev>(), nc, crows, s.qb->view, s.pd, delta, w.seed_qacc.as<double>(),
                             w.row_cand.as<int32_t>(), w.row_off.as<int64_t>(), A, row_perm, ctx->stream));
  if ((rc = ctx->time_end("seed", 2))) return rc;
  if (s.last_stage == 1) return download_hits(ctx, w, A, nseed, s.hs->hits);
  // ---- ungapped extension; hits above the -f threshold are dropped before the sort (they cannot survive the filter) ----
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_ungapped(A, nseed, s.qb->view, s.pd, s.sc, s.eo, s.max_qlen, ctx->stream));
  if ((rc = ctx->time_end("ungapped", 1))) return rc;
  int64_t mc = 0;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = compact_below(ctx, w, A, nseed, s.opts.interaction_threshold, w.cidx, w.hitsB, &mc, s.nf))) return rc;
  if ((rc = ctx->time_end("filter", 2))) return rc;
  return count_hits_under_f(s, mc);
}

// The seeds of the sub-batch are produced, extended without gaps and thinned to the hits under the -f threshold
// (one seed in nine) in CHUNKS of consecutive candidates of at most `chunk_pairs` (query SA entry x database SA
// entry) pairs each; the survivors of all chunks, in candidate order, are what the sort and the redundancy filter
// then see.  So the seed pools are bounded by the pair budget whatever a single query brings - a 100 kb query
// against a 100 M character page has 1e10 seeds - while the filter still runs over whole queries.
static int seeds_to_hits(SubSearch &s) {
  SearchWs &w = s.w;
  CandDev *cd = s.b.cd;
  int rc;
  if ((rc = w.front.init())) return rc;
  for (int32_t c0 = 0; c0 < s.ncand;) {
    SeedChunk c;
    c.c0 = c0;
    c.c1 = chunk_end(cd, s.ncand, c0, s.k.chunk_pairs, &c.pairs);
    c.nc = c.c1 - c0;
    const int64_t row_base = cd[c0].row0, ent_base = cd[c0].qoff;
    c.crows = (c.c1 < s.ncand ? cd[c.c1].row0 : s.b.nrows) - row_base;
    c.cents = (c.c1 < s.ncand ? cd[c.c1].qoff : s.b.nqent) - ent_base;
    for (int32_t i = c0; i < c.c1; i++) {
      cd[i].row0 -= row_base;
      cd[i].qoff -= ent_base;
    }
    // the one-pass form needs the chunk's pairs sorted: the front stage has them already, or sorts them now
    int64_t np = -1;
    if (s.k.fused && s.last_stage != 1 && s.k.row_shift >= 0 && c.pairs < 4.0e9) {
      if ((rc = s.ctx->time_begin())) return rc;
      SearchWs::FrontStage &F = w.front;
      if (c0 == 0 && F.ahead && F.cd == cd && F.nc == c.nc) { // issued while the last sub-batch was extended: wait for it
        np = F.np;
        PRB_HIP(hipStreamWaitEvent(s.ctx->stream, F.done, 0));
      } else {
        if (F.ahead) PRB_HIP(hipStreamSynchronize(F.stream)); // (not what was expected: its buffers are taken over)
        if ((rc = issue_front(w, s.qb, s.pd, s.eo.delta, s.k, cd + c0, c.nc, c.cents, s.ctx->stream, &np, s.allow, s.ctx))) return rc;
      }
      F.ahead = false;
      if (np >= 0 && F.unsorted) {
        if ((rc = finish_front(s.ctx, w, s.k, c.nc, &np))) return rc;
        if (np == 0) { // the mask leaves nothing of the chunk: no sort, no extension
          if ((rc = s.ctx->time_end("seed", 0))) return rc;
          c0 = c.c1;
          continue;
        }
      }
    }
    if ((rc = np >= 0 ? seed_chunk_one_pass(s, c, np) : seed_chunk_lists(s, c))) return rc;
    c0 = c.c1;
  }
  return PRB_OK;
}

// ------------------------------------------------------------------------- sort, redundancy filter
// The nf records in w.hitsB sorted and filtered: the nung survivors in s.U (w.hitsA), their first-of-query flags in w.first
static int sort_filter_ungapped(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  int rc;
  // A list this long (one very long query against a large page: 1.2e9 hits pass -f for 45 kb against 100 M characters) needs
  // the memory that buffers of stages already over still hold: the seed pools now, the sort keys and the records behind the
  // sort.  (hipFree waits for the device: only where it is needed.)
  const bool big_list = hits_bytes(s.nf) > s.k.big_list_bytes;
  mem_note("seed chunks done", w);
  if (big_list) {
    w.trim_next = true;
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    w.front.release();
    for (DevBuf *b : {&w.hitsA, &w.hitsTmp, &w.row_count, &w.row_off, &w.row_cand, &w.seed_qacc, &w.cands, &w.trace, &w.keptU, &w.keptTrace})
      b->release();
    for (DevBuf &b : w.resumePool) b.release();
    // (and this context's Raccess workspace, up to 48 GB when it last took a large batch: its launches are over)
    for (DevBuf *b : {&ctx->ra_band, &ctx->ra_vec, &ctx->ra_codes, &ctx->ra_desc}) b->release();
    if ((rc = w.front.init())) return rc;
  }
  mem_note("before the sort", w);
  if ((rc = w.hitsC.ensure(hits_bytes(s.nf)))) return rc;
  HitSoA B = carve_hits(w.hitsC, s.nf);
  uint32_t *perm = nullptr;
  if ((rc = ctx->time_begin())) return rc;
  SortBounds sb1 = s.sb; // hits extended without gaps have one length: the key is 11 + (11 - bits of the longest) bits shorter
  if (s.all_one_pass && s.one_pass_maxlen > 0 && !s.k.sort_two_lengths) sb1.eq_len_max = (int32_t)s.one_pass_maxlen;
  if ((rc = sort_hits(ctx, w, s.k, w.hitsB.as<HitRec>(), B, s.nf, sb1, &perm))) return rc;
  if ((rc = ctx->time_end("sort", 9))) return rc;
  if (big_list) // (the records and the sort's keys are dead)
    for (DevBuf *b : {&w.hitsB, &w.kE, &w.kL, &w.kQ, &w.kP, &w.kTmp, &w.kTmp2, &w.idxA, &w.idxB, &w.sortTmp}) b->release();
  mem_note("sorted", w);
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = filter_hits(ctx, w, B, s.nf, s.opts.interaction_threshold, s.k.filter_tiles, &s.nung))) return rc;
  if ((rc = ctx->time_end("filter", 3))) return rc;
  s.hs->counts[1] += s.nung;
  if (s.nung == 0) return PRB_OK;
  // compact survivors into hitsA (its seed content is no longer needed; the last chunk's pool may be smaller than this list)
  if ((rc = w.hitsA.ensure(hits_bytes(s.nung)))) return rc;
  s.U = carve_hits(w.hitsA, s.nung);
  PRB_HIP(launch_gather_hits(B, w.surv.as<uint32_t>(), s.U, s.nung, ctx->stream));
  if ((rc = w.first.ensure((size_t)s.nung))) return rc;
  PRB_HIP(launch_mark_first(s.U.query, s.nung, w.first.as<uint8_t>(), ctx->stream));
  s.first = w.first.as<uint8_t>();
  return PRB_OK;
}

// last_stage == 2: the hits extended without gaps to the host, with the pairs of their diagonals
static int emit_ungapped(SubSearch &s) {
  prb_hitset *hs = s.hs;
  const size_t base = hs->hits.size();
  if (int rc = download_hits(s.ctx, s.w, s.U, s.nung, hs->hits)) return rc;
  // (soft-masked codes 6..9 mapped to their bases: the reference reads outside BP_pair for them)
  auto code_base = [](unsigned c) { return c <= 5 ? (int)c - 1 : (int)c - 5; };
  // GetBasePair (rna_interaction_search.cpp:371-385): complementary positions of the diagonal
  for (size_t i = base; i < hs->hits.size(); i++) {
    prb_hit &h = hs->hits[i];
    const uint8_t *qs = s.qb->enc.data() + s.qb->off[h.query];
    h.bp_offset = (int64_t)hs->bp.size() / 2;
    const int len = (int)(uint16_t)h.q_len;
    for (int j = 0; j < len; j++)
      if (s.ctx->params.bp_pair[code_base(qs[h.q_sp + j])][code_base(s.pg.seqs[h.db_sp + j])] != 0) {
        hs->bp.push_back(h.q_sp + j);
        hs->bp.push_back(h.db_sp + j);
        h.bp_count++;
      }
  }
  return PRB_OK;
}

// ------------------------------------------------------------------------- final sort + filter
// (hits above the -g threshold dropped first)
static int final_sort_filter(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  int rc;
  if (!s.chunked) {
    if ((rc = ctx->time_begin())) return rc;
    if ((rc = compact_below(ctx, w, s.G, s.nung, s.opts.final_threshold, w.cidx, w.hitsB, &s.ngap))) return rc;
    if ((rc = ctx->time_end("filter", 2))) return rc;
  }
  if (s.ngap == 0) return PRB_OK;
  if ((rc = w.hitsC.ensure(hits_bytes(s.ngap)))) return rc; // (more than a chunk's worth, possibly, when the stage ran in chunks)
  HitSoA S = carve_hits(w.hitsC, s.ngap); // G is dead after the compaction
  uint32_t *perm = nullptr;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = sort_hits(ctx, w, s.k, w.hitsB.as<HitRec>(), S, s.ngap, s.sb, &perm))) return rc;
  if ((rc = ctx->time_end("sort", 9))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = filter_hits(ctx, w, S, s.ngap, s.opts.final_threshold, s.k.filter_tiles, &s.nfin))) return rc;
  if ((rc = ctx->time_end("filter", 3))) return rc;
  s.hs->counts[2] += s.nfin;
  if (s.nfin == 0) return PRB_OK;
  // final hits, and for each the index of its pre-gapped state in U (for the traceback):
  // final -> sorted position -> position in the compacted list -> index in U
  if ((rc = w.hitsB.ensure(hits_bytes(s.nfin)))) return rc; // (the records of the compacted list are dead after the sort)
  s.F = carve_hits(w.hitsB, s.nfin);
  PRB_HIP(launch_gather_hits(S, w.surv.as<uint32_t>(), s.F, s.nfin, ctx->stream));
  if ((rc = w.subset2.ensure((size_t)s.nfin * 4)) || (rc = w.subset.ensure((size_t)s.nfin * 4))) return rc;
  PRB_HIP(launch_gather_u32(perm, w.surv.as<uint32_t>(), w.subset2.as<uint32_t>(), s.nfin, ctx->stream));
  PRB_HIP(launch_gather_u32(w.cidx.as<uint32_t>(), w.subset2.as<uint32_t>(), w.subset.as<uint32_t>(), s.nfin, ctx->stream));
  return PRB_OK;
}

// ------------------------------------------------------------------------- distinct sites, best chain
// The two selections inside the (query, db_id) runs of a final list (include/priblast_hip.h): what tells them apart
enum class SiteRule { kDistinct, kChain };
static const char *rule_name(SiteRule rule) { return rule == SiteRule::kChain ? "chain sites" : "distinct sites"; }
static ModeTimer rule_timer(SiteRule rule) { return rule == SiteRule::kChain ? ModeTimer::kChain : ModeTimer::kDistinct; }

// The selection of opts.distinct_sites / opts.chain_sites over the n hits of `h` (sorted, or a caller's list): keep flags
// in w.keep.  The scratch is what the redundancy filter has left behind (w.endKey, w.pmax, w.state) and a list of the
// gapped cascade.
static int select_sites(prb_ctx *ctx, SearchWs &w, const HitSoA &h, int64_t n, SiteRule rule, const SearchKnobs &k) {
  const size_t N = (size_t)n;
  const bool chain = rule == SiteRule::kChain;
  int rc;
  if (n > INT32_MAX) {
    set_error(std::string(rule_name(rule)) + ": more than 2^31 - 1 final hits in one list");
    return PRB_ERR_ARG;
  }
  if ((rc = w.pairHead.ensure(N)) || (rc = w.keep.ensure(N)) || (rc = w.state.ensure(N)) || (rc = w.endKey.ensure(N * (chain ? 8 : 4))) ||
      (rc = w.pmax.ensure(N * 4)) || (rc = w.listA.ensure((size_t)site_long_runs_max(n) * 4)) || (rc = w.pending.ensure(16)))
    return rc;
  PRB_HIP(launch_pair_heads(h.query, h.db_id, n, w.pairHead.as<uint8_t>(), ctx->stream));
  if (chain) {
    const ChainScratch scratch{w.listA.as<uint32_t>(), w.pending.as<uint32_t>(), w.endKey.as<double>(), w.pmax.as<int32_t>()};
    PRB_HIP(launch_chain_select(h, n, w.pairHead.as<uint8_t>(), k.chain_lds_hits, scratch, w.keep.as<uint8_t>(), ctx->stream));
  } else {
    const SiteScratch scratch{w.listA.as<uint32_t>(), w.pending.as<uint32_t>(), w.endKey.as<int32_t>(), w.pmax.as<int32_t>(), w.state.as<uint8_t>()};
    PRB_HIP(launch_site_select(h, n, w.pairHead.as<uint8_t>(), k.distinct_lds_hits, scratch, w.keep.as<uint8_t>(), ctx->stream));
  }
  return PRB_OK;
}

// opts.distinct_sites / opts.chain_sites: the final hits F thinned to what the rule keeps of each pair
// (include/priblast_hip.h), before the traceback - the last stage that touches every final hit - so that a dropped hit
// costs no traceback, no copy and no formatting.  F and w.subset (the pre-gapped indices the traceback and the `first`
// flags go by) are compacted alike, s.nfin becomes the number kept; everything behind works on that list unchanged.
// (counts[2] was taken before.)
static int thin_sites(SubSearch &s, SiteRule rule) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const ModeTimer timer = rule_timer(rule);
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = select_sites(ctx, w, s.F, s.nfin, rule, s.k))) return rc;
  int64_t nkeep = 0;
  if ((rc = w.surv.ensure((size_t)s.nfin * 4)) || (rc = w.count.ensure(16))) return rc;
  if ((rc = select_flagged(ctx, w, nullptr, w.keep.as<uint8_t>(), w.surv.as<uint32_t>(), (size_t)s.nfin, &nkeep))) return rc;
  if (nkeep <= 0 || nkeep > s.nfin) { // (every pair keeps a hit)
    set_error(std::string(rule_name(rule)) + ": " + std::to_string(nkeep) + " of " + std::to_string(s.nfin) + " final hits kept");
    return PRB_ERR_STATE;
  }
  if (nkeep == s.nfin) return ctx->time_end(timer, 4);
  if ((rc = w.hitsTmp.ensure(hits_bytes(nkeep))) || (rc = w.subset2.ensure((size_t)nkeep * 4))) return rc;
  const HitSoA kept = carve_hits(w.hitsTmp, nkeep);
  PRB_HIP(launch_gather_hits(s.F, w.surv.as<uint32_t>(), kept, nkeep, ctx->stream));
  PRB_HIP(launch_gather_u32(w.subset.as<uint32_t>(), w.surv.as<uint32_t>(), w.subset2.as<uint32_t>(), nkeep, ctx->stream));
  std::swap(w.subset, w.subset2);
  s.F = kept;
  s.nfin = nkeep;
  return ctx->time_end(timer, 6);
}
static int distinct_sites(SubSearch &s) { return thin_sites(s, SiteRule::kDistinct); }
static int chain_sites(SubSearch &s) { return thin_sites(s, SiteRule::kChain); }

// ------------------------------------------------------------------------- traceback
// Base pairs of the final hits: from the trace slots of the extension pass; the few hits the slots cannot describe
// (wave-kernel hits, chains longer than a slot) are extended again.  Leaves the "traceback" bracket open: what the
// emit path does before it closes it still counts there.
static int traceback(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const int64_t nfin = s.nfin;
  const size_t NF = (size_t)nfin;
  int rc;
  if ((rc = w.copy_init())) return rc;
  if (w.copy_pending) { // the last results' copy still reads the buffers that are written next
    PRB_HIP(hipStreamWaitEvent(ctx->stream, w.copy_done, 0));
    w.copy_pending = false;
  }
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = w.bpCount.ensure((NF + 1) * 4)) || (rc = w.bpOff.ensure((NF + 1) * 8)) || (rc = w.tierFin.ensure(NF)) ||
      (rc = w.ntraceFin.ensure(NF * 4)))
    return rc;
  // host copies of four per-hit arrays + the offsets, in one page-locked block that lives with the workspace (fresh
  // vectors of 3 MB each were an mmap, ~750 page faults and a munmap apiece, per sub-batch)
  const size_t tb_bytes = NF * 4 * 3 + NF + 16 + (NF + 1) * 8;
  if ((rc = w.tb_pinned.ensure(w.tb_pinned.cap >= tb_bytes ? tb_bytes : 2 * tb_bytes))) return rc;
  int64_t *off = static_cast<int64_t *>(w.tb_pinned.p);
  uint32_t *pre = reinterpret_cast<uint32_t *>(off + NF + 1); // index of each final hit's pre-gapped state in U
  int32_t *cnt = reinterpret_cast<int32_t *>(pre + NF);
  uint32_t *ntr = reinterpret_cast<uint32_t *>(cnt + NF);
  uint8_t *tier_fin = reinterpret_cast<uint8_t *>(ntr + NF);
  PRB_HIP(hipMemcpyAsync(pre, w.subset.p, NF * 4, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(launch_bp_count(s.U, nfin, w.subset.as<uint32_t>(), s.qb->view, s.pd, s.sc, s.ntrace_all, w.bpCount.as<int32_t>(), ctx->stream));
  PRB_HIP(hipMemcpyAsync(cnt, w.bpCount.p, NF * 4, hipMemcpyDeviceToHost, ctx->stream));
  // which kernel of the cascade completed each final hit, and its chain lengths
  PRB_HIP(launch_gather_u8(s.tier_all, w.subset.as<uint32_t>(), w.tierFin.as<uint8_t>(), nfin, ctx->stream));
  PRB_HIP(launch_gather_u32(reinterpret_cast<const uint32_t *>(s.ntrace_all), w.subset.as<uint32_t>(), w.ntraceFin.as<uint32_t>(), nfin,
                            ctx->stream));
  PRB_HIP(hipMemcpyAsync(tier_fin, w.tierFin.p, NF, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipMemcpyAsync(ntr, w.ntraceFin.p, NF * 4, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  off[0] = 0;
  for (int64_t i = 0; i < nfin; i++) off[i + 1] = off[i] + cnt[i];
  s.bp_total = off[nfin];
  if ((rc = w.bpOut.ensure((size_t)std::max<int64_t>(s.bp_total, 1) * 8))) return rc;
  PRB_HIP(hipMemcpyAsync(w.bpOff.p, off, (NF + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(launch_bp_expand(s.U, nfin, w.subset.as<uint32_t>(), s.qb->view, s.pd, s.sc, s.first, s.ntrace_all, s.tier_all, s.trace_all, s.lt,
                           w.bpOff.as<int64_t>(), w.bpOut.as<int32_t>(), ctx->stream));
  // the hits to extend again, by the kernel that completed them
  std::vector<uint32_t> tlist[kWaveTier + 1];
  std::vector<int64_t> toff[kWaveTier + 1];
  const int slot_cap = s.k.trace_slot_cap;
  for (int64_t i = 0; i < nfin; i++) {
    const int t = std::min<int>(tier_fin[i] & 7, kWaveTier);
    if (!s.k.trace_no_slots && (tier_fin[i] & 7) == kLongTraceTier && s.lt.slot) continue; // (its chains are on record: launch_bp_expand wrote its pairs)
    if (s.k.trace_no_slots || t == kWaveTier || (int)(ntr[i] & 0xFFFF) > slot_cap || (int)(ntr[i] >> 16) > slot_cap) {
      tlist[t].push_back(pre[i]);
      toff[t].push_back(off[i]);
    }
  }
  bool any_rerun = false;
  for (int t = 0; t <= kWaveTier; t++) {
    if (tlist[t].empty()) continue;
    const int64_t m = (int64_t)tlist[t].size();
    if (!any_rerun) {
      if ((rc = ctx->time_end("traceback", 1))) return rc;
      if ((rc = ctx->time_begin())) return rc;
      any_rerun = true;
    }
    if ((rc = w.bpOff2.ensure((size_t)m * 8)) || (rc = w.subset2.ensure((size_t)m * 4))) return rc;
    PRB_HIP(hipMemcpyAsync(w.bpOff2.p, toff[t].data(), (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
    PRB_HIP(hipMemcpyAsync(w.subset2.p, tlist[t].data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = retrace_tier(s, t, w.subset2.as<uint32_t>(), w.bpOff2.as<int64_t>(), m))) return rc;
    PRB_HIP(hipStreamSynchronize(ctx->stream)); // the staging buffers are reused by the next tier
  }
  if (any_rerun) {
    if ((rc = ctx->time_end("traceback_slow", 0))) return rc;
    if ((rc = ctx->time_begin())) return rc;
  }
  return PRB_OK;
}

// ------------------------------------------------------------------------- results
// A staging slot for results that leave the device: the background thread must be done with it
static int acquire_slot(SubSearch &s) {
  const int slot = s.hs->next_slot;
  s.hs->next_slot ^= 1;
  s.hs->drain->acquire(slot);
  return slot;
}
// w.packed (`bytes` of records) - and `nbp_ints` of base pairs at bp_src, if any - into the staging slot on the copy
// stream; the background thread appends them to the hit set
static int copy_out(SubSearch &s, int slot, size_t bytes, const int32_t *bp_src, int64_t nbp_ints) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  PRB_HIP(hipEventRecord(w.packed_ready, ctx->stream));
  PRB_HIP(hipStreamWaitEvent(w.copy_stream, w.packed_ready, 0));
  PRB_HIP(hipMemcpyAsync(w.pin_hits[slot].p, w.packed.p, bytes, hipMemcpyDeviceToHost, w.copy_stream));
  if (nbp_ints) PRB_HIP(hipMemcpyAsync(w.pin_bp[slot].p, bp_src, (size_t)nbp_ints * 4, hipMemcpyDeviceToHost, w.copy_stream));
  PRB_HIP(hipEventRecord(w.copy_done, w.copy_stream));
  w.copy_pending = true;
  return PRB_OK;
}
// (page-locking a fresh 50 MB block takes ~35 ms with the GPU idle: when a slot has to grow, to twice the need, so
// that the larger sub-batches to come still fit)
static int ensure_slot(PinnedBuf &b, size_t bytes) { return b.ensure(b.cap >= bytes ? bytes : 2 * bytes); }

// The base pairs that go with a sub-batch's hit records, in ints: the simplified output prints only the first and the
// last pair of a hit, so only those two are kept (w.bpEnds); the detailed output keeps every pair (w.bpOut)
static int64_t record_bp_ints(const SubSearch &s) { return s.opts.output_style == 0 ? s.nfin * 4 : s.bp_total * 2; }
// the final hits' end pairs, as the simplified output has them: w.bpEnds
static int bp_ends(SubSearch &s) {
  SearchWs &w = s.w;
  if (int rc = w.bpEnds.ensure((size_t)s.nfin * 16)) return rc;
  PRB_HIP(launch_bp_ends(w.bpOff.as<int64_t>(), s.nfin, w.bpOut.as<int32_t>(), w.bpEnds.as<int32_t>(), s.ctx->stream));
  return PRB_OK;
}
// the final hits' records into w.packed (the caller has sized it), their base-pair ranges counted from pair `bp_base`
// on; *bp_src = the record_bp_ints(s) ints that the ranges index
static int pack_records(SubSearch &s, int64_t bp_base, const int32_t **bp_src) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const int64_t nfin = s.nfin;
  if (s.opts.output_style == 0) {
    if (int rc = bp_ends(s)) return rc;
    PRB_HIP(launch_pack_hits(s.F, nfin, nullptr, nullptr, bp_base, w.packed.p, ctx->stream));
    *bp_src = w.bpEnds.as<int32_t>();
  } else {
    PRB_HIP(launch_pack_hits(s.F, nfin, w.bpCount.as<int32_t>(), w.bpOff.as<int64_t>(), bp_base, w.packed.p, ctx->stream));
    *bp_src = w.bpOut.as<int32_t>();
  }
  return PRB_OK;
}

// prb_search_page: records packed on the device (with their base-pair ranges), one asynchronous copy each for hits
// and pairs into a pinned slot.  Closes the "traceback" bracket.
static int emit_records(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  prb_hitset *hs = s.hs;
  const int64_t nfin = s.nfin;
  int rc;
  const int slot = acquire_slot(s);
  const int64_t bp_base_pairs = hs->bp_ints_total / 2;
  const int64_t nbp_ints = record_bp_ints(s);
  const size_t hit_bytes = (size_t)nfin * sizeof(prb_hit), bp_bytes = (size_t)std::max<int64_t>(nbp_ints, 1) * 4;
  if ((rc = w.packed.ensure(hit_bytes)) || (rc = ensure_slot(w.pin_hits[slot], hit_bytes)) || (rc = ensure_slot(w.pin_bp[slot], bp_bytes)))
    return rc;
  const int32_t *bp_src;
  if ((rc = pack_records(s, bp_base_pairs, &bp_src))) return rc;
  if ((rc = copy_out(s, slot, hit_bytes, bp_src, nbp_ints))) return rc;
  if (hs->on_device) { // device copies for the final hit gather (prb_gather_hits): no re-upload later
    if ((rc = hs->d_hits.append(w.packed.p, hit_bytes, ctx->stream)) || (rc = hs->d_bp.append(bp_src, (size_t)nbp_ints * 4, ctx->stream)))
      return rc;
  }
  PRB_HIP(hipEventRecord(hs->drain->ev[slot], w.copy_stream));
  hs->drain->submit(Drainer::Job{slot, nfin, nbp_ints});
  hs->hits_total += nfin;
  hs->bp_ints_total += nbp_ints;
  return ctx->time_end("traceback", 2);
}

// What everything per pair starts with: the final hits' end pairs (bp_ends), which closes the "traceback" bracket, then
// - in the bracket of the summary timer, left open - the pairs' runs of the list (contiguous: F is sorted by query, then
// db_sp, and a sub-batch is a range of whole queries): w.pairStart = the first hit of each of the *npairs pairs
static int pair_runs(SubSearch &s, int64_t *npairs) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const int64_t nfin = s.nfin;
  const size_t NF = (size_t)nfin;
  int rc;
  if ((rc = bp_ends(s))) return rc;
  if ((rc = ctx->time_end("traceback", 2))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = w.pairHead.ensure(NF)) || (rc = w.pairStart.ensure(NF * 4)) || (rc = w.count.ensure(16))) return rc;
  PRB_HIP(launch_pair_heads(s.F.query, s.F.db_id, nfin, w.pairHead.as<uint8_t>(), ctx->stream));
  if ((rc = select_flagged(ctx, w, nullptr, w.pairHead.as<uint8_t>(), w.pairStart.as<uint32_t>(), NF, npairs))) return rc;
  if (*npairs <= 0 || *npairs > nfin) {
    set_error("per-pair summary: " + std::to_string(*npairs) + " pairs for " + std::to_string(nfin) + " hits");
    return PRB_ERR_STATE;
  }
  return PRB_OK;
}
// ... and the runs folded into the pairs' records: prb_pair_summary[npairs] in w.packed
static int fold_pairs(SubSearch &s, int64_t npairs) {
  SearchWs &w = s.w;
  if (int rc = w.packed.ensure((size_t)npairs * sizeof(prb_pair_summary))) return rc;
  PRB_HIP(launch_pair_fold(s.F, s.nfin, w.pairStart.as<uint32_t>(), npairs, w.bpEnds.as<int32_t>(), w.packed.p, s.ctx->stream));
  return PRB_OK;
}

// prb_search_page_summary: the pairs' records reduced on the device; only they leave it
static int emit_summary(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  int rc;
  const int slot = acquire_slot(s);
  int64_t npairs = 0;
  if ((rc = pair_runs(s, &npairs))) return rc;
  const size_t rec_bytes = (size_t)npairs * sizeof(prb_pair_summary);
  if ((rc = ensure_slot(w.pin_hits[slot], rec_bytes)) || (rc = fold_pairs(s, npairs))) return rc;
  if ((rc = copy_out(s, slot, rec_bytes, nullptr, 0))) return rc;
  PRB_HIP(hipEventRecord(s.hs->drain->ev[slot], w.copy_stream));
  s.hs->drain->submit(Drainer::Job{slot, npairs, 0});
  s.hs->hits_total += s.nfin;
  return ctx->time_end(ModeTimer::kSummary, 3);
}

// Every prb_search_page_* of a result table: what the table's feed asks for (TableFeed, search_host.hpp) prepared in
// the brackets that are the driver's - "traceback" closed with the end pairs or the records, the summary timer's with
// the pairs' runs and their fold -, then the table takes the sub-batch in a bracket of its own.  Nothing leaves the device.
static int emit_to_table(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const TableFeed feed = s.table->feed();
  SubBatch b{s.page, s.b.q0, s.b.q1, s.qb->nq, s.pg.nseq, s.F, s.nfin};
  int rc;
  if (feed == TableFeed::kHitRecords) {
    if ((rc = w.packed.ensure((size_t)s.nfin * sizeof(prb_hit)))) return rc;
    if ((rc = pack_records(s, s.table->bp_base(), &b.fresh_bp))) return rc;
    if ((rc = ctx->time_end("traceback", 2))) return rc;
    b.records = w.packed.p;
  } else if (feed == TableFeed::kHits) {
    if ((rc = bp_ends(s))) return rc;
    if ((rc = ctx->time_end("traceback", 2))) return rc;
    b.ends = w.bpEnds.as<int32_t>();
  } else {
    const bool fold = feed == TableFeed::kPairRecords;
    if ((rc = pair_runs(s, &b.npairs))) return rc;
    if (fold && (rc = fold_pairs(s, b.npairs))) return rc;
    if ((rc = ctx->time_end(ModeTimer::kSummary, fold ? 3 : 2))) return rc;
    b.ends = w.bpEnds.as<int32_t>();
    b.pair_start = w.pairStart.as<uint32_t>();
    if (fold) b.records = w.packed.p;
  }
  if ((rc = s.table->take(b))) return rc;
  s.hs->hits_total += s.nfin;
  return PRB_OK;
}

// ------------------------------------------------------------------------- one sub-batch
// One sub-batch of queries through the GPU stages.  `b` = its seed candidates; `front_free` (may
// be empty): see SubSearch.
static int search_range(const PageSearch &p, const CandBatch &b, const std::function<void()> &front_free) {
  SubSearch s{p, b, front_free};
  int rc;
  if (s.w.trim_next) {
    PRB_HIP(hipStreamSynchronize(s.ctx->stream));
    s.w.trim();
  }
  if (b.ncand == 0) return PRB_OK;
  if (b.ncand > INT32_MAX) {
    set_error("too many seed candidates in one sub-batch: lower PRB_SEARCH_PAIRS, or build the database in smaller pages (db -c)");
    return PRB_ERR_NOMEM;
  }
  s.ncand = (int32_t)b.ncand;
  s.sb.qmin = b.cd[0].query; // the candidates are in query order
  s.sb.qspan = b.cd[s.ncand - 1].query - b.cd[0].query + 1;
  s.sb.max_qlen = s.max_qlen;
  s.sb.max_dblen = s.max_dblen;
  s.sb.nchars = s.pd.nchars;

  // seeds: one row per (candidate, db SA entry), extended without gaps, thinned to the hits under -f
  if ((rc = seeds_to_hits(s))) return rc;
  if (s.last_stage == 1 || s.nf == 0) return PRB_OK; // (the seeds went to the host chunk by chunk)
  if ((rc = sort_filter_ungapped(s))) return rc;
  if (s.nung == 0) return PRB_OK;
  if (s.last_stage == 2) return emit_ungapped(s);

  if ((rc = gapped_stage(s))) return rc;
  // The front of the NEXT sub-batch's seed path (bandwidth-bound, ~7 ms per configs[2] query) goes out here at the latest:
  // beside what is left of this sub-batch - the ~150 longest extensions on a wavefront each (2 ms, and 2 ms again for
  // their base pairs), the final sort and filter of a few hundred thousand hits, the copies to the host - the GPU is
  // nearly idle.  (Issued right behind k_seed_extend, even on a stream of the lowest priority, it cost the gapped
  // tiers 290 ms per step: its workgroups take LDS and wave slots that tier 0 fills completely.)
  call_front_free(s);
  if ((rc = final_sort_filter(s))) return rc;
  if (s.nfin == 0) return PRB_OK;
  if (s.opts.distinct_sites && (rc = distinct_sites(s))) return rc;
  if (s.opts.chain_sites && (rc = chain_sites(s))) return rc;
  if ((rc = traceback(s))) return rc;
  return s.mode == SearchMode::kRecords ? emit_records(s) : s.mode == SearchMode::kSummary ? emit_summary(s) : emit_to_table(s);
}

// ------------------------------------------------------------------------- one page
int check_search_args(const char *fn, const prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page,
                      const prb_ris_opts *opts, int32_t last_stage) {
  if (!ctx || !qb || !db || !opts || qb->ctx->device != ctx->device || db->ctx->device != ctx->device || page < 0 ||
      page >= (int32_t)db->pages.size() || last_stage < 1 || last_stage > 3) {
    set_error(std::string(fn) + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (!qb->have_acc || qb->W != db->hdr.maximal_span || qb->delta != db->hdr.min_accessible_length) {
    set_error(std::string(fn) + ": query accessibilities must be computed with the database's span / window parameters");
    return PRB_ERR_STATE;
  }
  if (qb->repeat_flag != db->hdr.repeat_flag) {
    set_error(std::string(fn) + ": query batch was encoded with a different repeat flag than the database");
    return PRB_ERR_STATE;
  }
  if (opts->drop_out_w_gap < 0 || opts->drop_out_w_gap > 30 || opts->drop_out_wo_gap < 1 || opts->drop_out_wo_gap > 15 ||
      opts->min_helix_length < 1 || opts->min_helix_length > 16 || opts->max_seed_length < 1 || opts->max_seed_length > 63) {
    set_error("unsupported option: need 0 <= -x <= 30, 1 <= -y <= 15 (beyond that the reference reads outside its "
              "31-entry loop tables), 1 <= -m <= 16, 1 <= -l <= 63 (the seed search keeps a path of 64 characters)");
    return PRB_ERR_ARG;
  }
  if (opts->distinct_sites != 0 && opts->distinct_sites != 1) {
    set_error(std::string(fn) + ": distinct_sites must be 0 or 1 (got " + std::to_string(opts->distinct_sites) + ")");
    return PRB_ERR_ARG;
  }
  if (opts->chain_sites != 0 && opts->chain_sites != 1) {
    set_error(std::string(fn) + ": chain_sites must be 0 or 1 (got " + std::to_string(opts->chain_sites) + ")");
    return PRB_ERR_ARG;
  }
  if (opts->chain_sites && opts->distinct_sites) {
    set_error(std::string(fn) + ": chain_sites and distinct_sites can't both be 1 (each of them selects among every final hit of a pair)");
    return PRB_ERR_ARG;
  }
  return PRB_OK;
}

// The queries [a, b) of a seed plan as a sub-batch: their candidates converted straight into page-locked memory
// (queries in parallel), rows and query entries numbered from 0.  (Candidates are converted once: the plan's are gone.)
static int convert_cands(prb_ctx *ctx, SeedPlan &plan, int32_t a, int32_t b, PinnedBuf &pin, CandBatch &out) {
  const int32_t nb = b - a;
  std::vector<int64_t> cbase((size_t)nb + 1, 0), rbase((size_t)nb + 1, 0), ebase((size_t)nb + 1, 0);
  for (int32_t k = 0; k < nb; k++) {
    cbase[k + 1] = cbase[k] + (int64_t)plan.per_q[a + k].size();
    rbase[k + 1] = rbase[k] + plan.qrows[a + k];
    ebase[k + 1] = ebase[k] + plan.qents[a + k];
  }
  out.q0 = a;
  out.q1 = b;
  out.ncand = cbase[nb];
  out.nrows = rbase[nb];
  out.nqent = ebase[nb];
  if (int r = pin.ensure((size_t)std::max<int64_t>(out.ncand, 1) * sizeof(CandDev))) return r;
  CandDev *cd = static_cast<CandDev *>(pin.p);
  out.cd = cd;
  HostTimer ht(ctx, "host_cands");
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min(8, host_threads(nb)))
  for (int32_t k = 0; k < nb; k++) {
    std::vector<SeedCandidate> &v = plan.per_q[a + k];
    CandDev *o = cd + cbase[k];
    int64_t row = rbase[k], ent = ebase[k];
    for (size_t i = 0; i < v.size(); i++) {
      const SeedCandidate &c = v[i];
      o[i] = CandDev{c.sp_q, c.ep_q, c.sp_db, c.ep_db, c.length, c.query, c.score, row, ent};
      row += (int64_t)c.ep_db - c.sp_db + 1;
      ent += (int64_t)c.ep_q - c.sp_q + 1;
    }
    std::vector<SeedCandidate>().swap(v);
  }
  return PRB_OK;
}

// queries [q0, *q1) = as many as fit the pair budget.  wait: for each query's DFS; else false when one is not done yet
static bool take_queries(SeedPlan &plan, int32_t q0, double budget, bool wait, int32_t *q1_out) {
  int32_t q1 = q0;
  double acc = 0;
  for (; q1 < plan.nq; q1++) {
    if (wait) plan.wait_for(q1);
    else if (!plan.done[q1].load(std::memory_order_acquire)) return false;
    if (q1 > q0 && acc + plan.qpairs[q1] > budget) break;
    acc += plan.qpairs[q1];
  }
  *q1_out = q1;
  return true;
}

int search_page(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, int32_t last_stage,
                SearchMode mode, prb_hitset **out, TableState *table) {
  const bool summary = reduces_to_pairs(mode);
  const char *fn = summary ? "prb_search_page_summary" : "prb_search_page";
  if (!out) {
    set_error(std::string(fn) + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (int rc = check_search_args(fn, ctx, qb, db, page, opts, last_stage)) return rc;
  *out = nullptr;
  PRB_HIP(hipSetDevice(ctx->device));
  AllowDev allow{};
  if (opts->allowed_pairs)
    if (int rc = use_pairmask(fn, ctx, qb, db, page, opts->allowed_pairs, &allow)) return rc;
  {
    // the page on the device (uploaded now unless it is resident or was prefetched), then - while it is searched -
    // the next page on the copy stream
    int slot = -1, rcp;
    if ((rcp = page_slot(ctx, db, page, -1, ctx->stream, &slot))) return rcp;
    PRB_HIP(hipStreamWaitEvent(ctx->stream, db->slot_ready[(size_t)slot], 0));
    const int next = page + 1 < (int32_t)db->pages.size() ? page + 1 : 0;
    if (db->copy_stream && db->mem.size() >= 2 && next != page && db->slot_of_page[(size_t)next] < 0) {
      int ns = -1;
      if ((rcp = page_slot(ctx, db, next, page, db->copy_stream, &ns))) return rcp;
      db->slot_used[(size_t)slot] = ++db->clock; // (the page being searched is the most recently used one)
    }
  }
  // Seed search proper: DFS over the two suffix arrays, per query, on host threads.  It runs
  // in the background while the GPU already works on the first sub-batches: the consumer below
  // only waits for the queries it is about to submit.  If the caller started it ahead
  // (prb_qbatch_seed_search_begin with the same page and options), that one is used.
  const int32_t nq = qb->nq;
  std::unique_ptr<SeedPlan> plan_owner;
  if (qb->plan && qb->plan->db == db && qb->plan->page == page && qb->plan->max_seed_length == opts->max_seed_length &&
      qb->plan->hybrid_threshold == opts->hybrid_threshold) {
    plan_owner = std::move(qb->plan);
  } else {
    plan_owner = start_seed_plan(ctx, qb, db, page, opts->max_seed_length, opts->hybrid_threshold);
  }
  SeedPlan &plan = *plan_owner;
  auto *hs = new prb_hitset();
  hs->device = ctx->device;
  hs->on_device = ctx->keep_device_records && last_stage == 3 && !summary;
  hs->d_hits.hint = ctx->keep_hint_hits;
  hs->d_bp.hint = ctx->keep_hint_bp;
  SearchWs &wsp = ws_of(ctx);
  Drainer drain(&hs->hits, &hs->bp, wsp.pin_hits, wsp.pin_bp);
  if (summary) drain.pairs = &hs->pairs;
  hs->drain = &drain;
  if (last_stage == 3 && !summary) { // a stream of similar batches: the last hit set's size, with a twentieth to spare, up front
    drain.hint_hits = ctx->host_hint_hits + ctx->host_hint_hits / 20;
    drain.hint_bp = ctx->host_hint_bp + ctx->host_hint_bp / 20;
  }
  int rc = drain.start();
  double wait_ms = 0;
  const SearchKnobs knobs = read_search_knobs();
  const int delta = db->hdr.min_accessible_length;
  PageSearch ps{ctx,
                wsp,
                qb,
                db->pages[(size_t)page],
                db->mem[(size_t)db->slot_of_page[(size_t)page]].view,
                static_cast<SearchConstMem *>(ctx->search_const)->view,
                ExtOpts{delta, opts->drop_out_wo_gap, opts->drop_out_w_gap, opts->min_helix_length},
                *opts,
                knobs,
                page,
                last_stage,
                mode,
                table,
                hs,
                0,
                0};
  if (opts->allowed_pairs) ps.allow = &allow;
  for (int32_t q = 0; q < nq; q++) ps.max_qlen = std::max(ps.max_qlen, qb->len[q]);
  for (int32_t L : ps.pg.seq_length) ps.max_dblen = std::max(ps.max_dblen, L);
  CandBatch next; // the sub-batch behind the current one, when it has been prepared ahead (next.q1 > next.q0)
  int parity = 0;
  for (int32_t q0 = 0; q0 < nq && rc == PRB_OK;) {
    CandBatch cur;
    if (next.q1 > next.q0 && next.q0 == q0) {
      cur = next;
    } else {
      const auto tw0 = std::chrono::steady_clock::now();
      int32_t q1 = q0;
      take_queries(plan, q0, knobs.budget, true, &q1);
      wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
      if ((rc = convert_cands(ctx, plan, q0, q1, wsp.cand_pinned[parity], cur))) break;
    }
    next = CandBatch{};
    const int32_t q1 = cur.q1;
    // While this sub-batch is sorted, filtered and extended: the candidates of the next one into the other page-locked
    // buffer and the front of its seed path onto the low-priority stream - if its queries' DFS is done (no waiting here).
    std::function<void()> front_free = [&]() {
      if (!knobs.front_ahead || q1 >= nq || last_stage == 1 || !knobs.fused || knobs.row_shift < 0) return;
      int32_t q2 = q1;
      if (!take_queries(plan, q1, knobs.budget, false, &q2)) return; // (the main loop will wait for it, and take it from there)
      CandBatch nb;
      if (convert_cands(ctx, plan, q1, q2, wsp.cand_pinned[parity ^ 1], nb) != PRB_OK) return;
      next = nb; // (candidates are converted once: `next` must be set)
      if (nb.ncand == 0 || nb.ncand > INT32_MAX) return;
      double pairs = 0;
      const int32_t c1 = chunk_end(nb.cd, (int32_t)nb.ncand, 0, knobs.chunk_pairs, &pairs);
      if (pairs >= 4.0e9) return;
      const int64_t cents = (c1 < nb.ncand ? nb.cd[c1].qoff : nb.nqent) - nb.cd[0].qoff;
      SearchWs::FrontStage &F = wsp.front;
      int64_t np = -1;
      if (issue_front(wsp, qb, ps.pd, delta, knobs, nb.cd, c1, cents, F.stream, &np, ps.allow, nullptr) != PRB_OK || np < 0 ||
          hipEventRecord(F.done, F.stream) != hipSuccess) {
        (void)hipStreamSynchronize(F.stream); // (whatever part of it was issued is not used)
        return;
      }
      F.ahead = true;
      F.cd = nb.cd;
      F.nc = c1;
      F.np = np;
    };
    {
      HostTimer ht(ctx, "host_search_range");
      rc = search_range(ps, cur, front_free);
      if (rc == PRB_ERR_NOMEM) // (the seed pools and the gapped stage's state are bounded by their chunk budgets; what grows with a
                               //  query is the list behind -f itself, ~200 B per hit with its sort keys)
        set_error(std::string(prb_last_error()) + " - the hits of queries " + std::to_string(q0) + ".." + std::to_string(q1 - 1) +
                  " that pass -f against this page do not fit the device (lower PRB_GAPPED_CHUNK_HITS / PRB_SEARCH_CHUNK_PAIRS if it is "
                  "their working state; else build the database in smaller pages, db -c, which bounds the list per page)");
    }
    // the pinned candidates are reused by the next sub-batch: their upload must be over
    if (rc == PRB_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PRB_ERR_HIP;
    q0 = q1;
    parity ^= 1;
    if (q0 < nq) { // extrapolated from the queries done so far, with a tenth to spare (never below the hint from the last set)
      const double scale = 1.1 * (double)nq / (double)q0;
      drain.hint_hits = std::max(drain.hint_hits.load(), (size_t)((double)hs->counts[2] * scale));
      drain.hint_bp = std::max(drain.hint_bp.load(), (size_t)((double)hs->bp_ints_total * scale));
    }
  }
  if (wsp.front.stream && wsp.front.ahead) { // (an error on the way: nothing of a front issued ahead stays in flight)
    (void)hipStreamSynchronize(wsp.front.stream);
    wsp.front.ahead = false;
  }
  plan.producer.join();
  {
    HostTimer ht(ctx, "host_drain_tail");
    const int drc = drain.finish();
    if (rc == PRB_OK) rc = drc;
    hs->drain = nullptr;
  }
  ctx->timers["host_dfs"].ms += plan.dfs_ms;  // wall time of the background DFS
  ctx->timers["host_dfs"].launches++;
  ctx->timers["host_dfs_wait"].ms += wait_ms; // what the GPU pipeline actually waited for it
  ctx->timers["host_dfs_wait"].launches++;
  if (rc != PRB_OK) {
    delete hs;
    return rc;
  }
  if (hs->on_device) {
    ctx->keep_hint_hits = hs->d_hits.used;
    ctx->keep_hint_bp = hs->d_bp.used;
  }
  if (last_stage == 3 && !summary) {
    ctx->host_hint_hits = hs->hits.size();
    ctx->host_hint_bp = hs->bp.size();
  }
  *out = hs;
  return PRB_OK;
}

} // namespace prb

extern "C" {

int prb_search_page(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, int32_t last_stage,
                    prb_hitset **out) {
  return search_page(ctx, qb, db, page, opts, last_stage, SearchMode::kRecords, out);
}

int prb_seed_pair_layout(int64_t nchars, int64_t query_span, int32_t row_shift, int32_t sort_bits, int32_t local_order, int32_t pair_wide,
                         int32_t out[6]) {
  if (!out || nchars < 1 || query_span < 0) {
    set_error("prb_seed_pair_layout: bad argument");
    return PRB_ERR_ARG;
  }
  const PairLayout L = pair_layout(nchars, query_span, std::min(row_shift, 30), std::max(sort_bits, 1), local_order != 0, pair_wide != 0);
  const int32_t v[6] = {L.narrow, L.pbits, L.kbits, L.begin, L.local_bits, L.wide_key()};
  std::copy(v, v + 6, out);
  return PRB_OK;
}

// prb_distinct_sites / prb_chain_sites: the caller's records as a list of the search's own layout (the fields the
// selections read; the others stay zero), one upload; the flags come back in one copy
static int select_callers_sites(const char *fn_name, prb_ctx *ctx, const prb_hit *hits, int64_t n, uint8_t *keep, prb::SiteRule rule) {
  const std::string fn = fn_name;
  if (!ctx || n < 0 || (n > 0 && (!hits || !keep))) {
    set_error(fn + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (n == 0) return PRB_OK;
  if (n > INT32_MAX) {
    set_error(fn + ": more than 2^31 - 1 hits");
    return PRB_ERR_ARG;
  }
  if (rule == prb::SiteRule::kChain) // the pass in list order needs every predecessor before its successors
    for (int64_t i = 1; i < n; i++)
      if (hits[i].query == hits[i - 1].query && hits[i].db_id == hits[i - 1].db_id && hits[i].db_sp < hits[i - 1].db_sp) {
        set_error(fn + ": hit " + std::to_string(i) + " has a lower db_sp than the hit before it in its run of equal (query, db_id)");
        return PRB_ERR_ARG;
      }
  PRB_HIP(hipSetDevice(ctx->device));
  SearchWs &w = ws_of(ctx);
  const SearchKnobs knobs = read_search_knobs();
  int rc;
  if ((rc = w.hitsTmp.ensure(hits_bytes(n)))) return rc;
  try {
    std::vector<uint8_t> host(hits_bytes(n), 0);
    const HitSoA hh = carve_hits(host.data(), n);
    for (int64_t i = 0; i < n; i++) {
      hh.q_sp[i] = hits[i].q_sp;
      hh.db_sp[i] = hits[i].db_sp;
      hh.q_len[i] = hits[i].q_len;
      hh.db_len[i] = hits[i].db_len;
      hh.db_id[i] = hits[i].db_id;
      hh.query[i] = hits[i].query;
      hh.e_tot[i] = hits[i].e_tot;
    }
    PRB_HIP(hipMemcpyAsync(w.hitsTmp.p, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the copy is staged, `host` may go)
  } catch (const std::exception &e) {
    set_error(fn + ": " + e.what());
    return PRB_ERR_NOMEM;
  }
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = select_sites(ctx, w, carve_hits(w.hitsTmp, n), n, rule, knobs))) return rc;
  if ((rc = ctx->time_end(rule_timer(rule), 3))) return rc;
  PRB_HIP(hipMemcpyAsync(keep, w.keep.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  return PRB_OK;
}
int prb_distinct_sites(prb_ctx *ctx, const prb_hit *hits, int64_t n, uint8_t *keep) {
  return select_callers_sites("prb_distinct_sites", ctx, hits, n, keep, prb::SiteRule::kDistinct);
}
int prb_chain_sites(prb_ctx *ctx, const prb_hit *hits, int64_t n, uint8_t *keep) {
  return select_callers_sites("prb_chain_sites", ctx, hits, n, keep, prb::SiteRule::kChain);
}

// A caller's records through the search's own sort and redundancy filter (sort_hits, filter_hits: what
// sort_filter_ungapped and final_sort_filter call), with the field bounds of the one-key sort taken from the list itself.
int prb_sort_filter(prb_ctx *ctx, const prb_hit *hits, int64_t n, double threshold, prb_hit *sorted, uint8_t *keep, int32_t *form) {
  if (!ctx || n < 0 || (n > 0 && (!hits || !sorted || !keep || !form))) {
    set_error("prb_sort_filter: bad argument");
    return PRB_ERR_ARG;
  }
  if (n == 0) return PRB_OK;
  if (n > INT32_MAX) {
    set_error("prb_sort_filter: more than 2^31 - 1 hits");
    return PRB_ERR_ARG;
  }
  const SearchKnobs knobs = read_search_knobs();
  SortBounds sb;
  int32_t qlo = INT32_MAX, qhi = 0, eq_len = 0;
  bool one_len = !knobs.sort_two_lengths;
  auto len16 = [](int32_t v) { return (int32_t)(uint16_t)v; }; // (the search's lengths are unsigned short, search_device.hpp)
  for (int64_t i = 0; i < n; i++) {
    const prb_hit &h = hits[i];
    const int64_t qend = (int64_t)h.q_sp + len16(h.q_len), dend = (int64_t)h.db_sp + len16(h.db_len);
    if (h.query < 0 || h.q_sp < 0 || h.db_sp < 0 || qend > INT32_MAX || dend > INT32_MAX) {
      set_error("prb_sort_filter: hit " + std::to_string(i) + " has a negative query or a coordinate outside 0 .. 2^31 - 1");
      return PRB_ERR_ARG;
    }
    qlo = std::min(qlo, h.query);
    qhi = std::max(qhi, h.query);
    sb.max_qlen = std::max(sb.max_qlen, (int32_t)qend);
    sb.max_dblen = std::max(sb.max_dblen, len16(h.db_len));
    sb.nchars = std::max(sb.nchars, (int32_t)dend);
    one_len = one_len && len16(h.q_len) == len16(h.db_len);
    eq_len = std::max(eq_len, len16(h.db_len));
  }
  sb.qmin = qlo;
  sb.qspan = qhi - qlo + 1;
  sb.eq_len_max = one_len ? eq_len : 0;
  PRB_HIP(hipSetDevice(ctx->device));
  SearchWs &w = ws_of(ctx);
  int rc;
  const size_t N = (size_t)n;
  if ((rc = w.hitsB.ensure(N * sizeof(HitRec))) || (rc = w.hitsC.ensure(hits_bytes(n))) || (rc = w.packed.ensure(N * sizeof(prb_hit))))
    return rc;
  try {
    std::vector<HitRec> host(N);
    for (int64_t i = 0; i < n; i++) {
      const prb_hit &h = hits[i];
      host[(size_t)i] = HitRec{h.q_sp, h.db_sp, h.q_len, h.db_len, h.db_id, h.db_id_start, h.query, 0, h.e_acc, h.e_hyb, h.e_tot, 0};
    }
    PRB_HIP(hipMemcpyAsync(w.hitsB.p, host.data(), N * sizeof(HitRec), hipMemcpyHostToDevice, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the copy is staged, `host` may go)
  } catch (const std::exception &e) {
    set_error(std::string("prb_sort_filter: ") + e.what());
    return PRB_ERR_NOMEM;
  }
  const HitSoA S = carve_hits(w.hitsC, n);
  uint32_t *perm = nullptr;
  int64_t nsurv = 0;
  if ((rc = sort_hits(ctx, w, knobs, w.hitsB.as<HitRec>(), S, n, sb, &perm, form))) return rc;
  if ((rc = filter_hits(ctx, w, S, n, threshold, knobs.filter_tiles, &nsurv))) return rc;
  PRB_HIP(launch_pack_hits(S, n, nullptr, nullptr, -1, w.packed.p, ctx->stream));
  PRB_HIP(hipMemcpyAsync(sorted, w.packed.p, N * sizeof(prb_hit), hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipMemcpyAsync(keep, w.keep.p, N, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  return PRB_OK;
}

int prb_search_page_summary(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_pairset **out) {
  if (!out) {
    set_error("prb_search_page_summary: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  prb_hitset *hs = nullptr;
  const int rc = search_page(ctx, qb, db, page, opts, 3, SearchMode::kSummary, &hs);
  if (rc != PRB_OK) return rc;
  auto *ps = new (std::nothrow) prb_pairset();
  if (!ps) {
    delete hs;
    set_error("prb_search_page_summary: out of host memory");
    return PRB_ERR_NOMEM;
  }
  ps->pairs.swap(hs->pairs);
  for (int i = 0; i < 3; i++) ps->counts[i] = hs->counts[i];
  delete hs;
  *out = ps;
  return PRB_OK;
}

int64_t prb_pairset_size(const prb_pairset *ps) { return ps ? (int64_t)ps->pairs.size() : -1; }
const prb_pair_summary *prb_pairset_pairs(const prb_pairset *ps) { return ps ? ps->pairs.data() : nullptr; }
void prb_pairset_counts(const prb_pairset *ps, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ps ? ps->counts[i] : 0;
}
void prb_pairset_free(prb_pairset *ps) { delete ps; }

int64_t prb_hitset_size(const prb_hitset *hs) { return !hs ? -1 : hs->ext_hits ? hs->ext_nhits : (int64_t)hs->hits.size(); }
const prb_hit *prb_hitset_hits(const prb_hitset *hs) { return !hs ? nullptr : hs->ext_hits ? hs->ext_hits : hs->hits.data(); }
const int32_t *prb_hitset_basepairs(const prb_hitset *hs, int64_t *count) {
  if (!hs) return nullptr;
  if (count) *count = (hs->ext_hits ? hs->ext_bp_ints : (int64_t)hs->bp.size()) / 2;
  return hs->ext_hits ? hs->ext_bp : hs->bp.data();
}
void prb_hitset_counts(const prb_hitset *hs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = hs ? hs->counts[i] : 0;
}
void prb_hitset_free(prb_hitset *hs) { delete hs; }

} // extern "C"
