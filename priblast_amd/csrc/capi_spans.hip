// C ABI, part 6: the two span tables - the per-position profile of a batch's queries (prb_profset_*) and the
// per-position coverage of a database's targets (prb_covset_*).  Both add every final hit's span to difference arrays
// and keep the best hit per position; the host code of their merges and finishes differs in the kernels it launches.
#include <cstring>

#include "capi_tables.hpp"

using namespace prb;

namespace {
// a slot of the profile table that some final hit covers (prb_profset_finish: `hits` holds the scanned counts)
struct ProfCovered {
  const int64_t *hits;
  __host__ __device__ bool operator()(const uint32_t &p) const { return hits[p] > 0; }
};
// the first slot of a region of the coverage table at depth D (prb_covset_finish: `queries` holds the scanned counts; a
// sequence's separator slot has none, so the slot in front of a sequence's first one is always below D)
struct CovHead {
  const int32_t *queries;
  int32_t D;
  __host__ __device__ bool operator()(const uint32_t &p) const { return queries[p] >= D && (p == 0 || queries[p - 1] < D); }
};
} // namespace

// ---- what the two tables' merges and finishes share
// A list of NF hits ordered by the low `bits` bits of its keys and the running maximum of the spans' ends, in b: keys()
// enqueues the kernel that writes (keyA, valA), the sort gives (keyB, valB), spans() enqueues the kernel that writes
// `span` in that order, the scan gives `scan`.  (The sort and the scan share b.sortTmp: both are sized before anything
// is enqueued.)
template <class Keys, class Spans> static int order_spans(prb_ctx *ctx, SpanBufs &b, size_t NF, int bits, Keys keys, Spans spans) {
  int rc;
  if ((rc = b.keyA.ensure(NF * 8)) || (rc = b.keyB.ensure(NF * 8)) || (rc = b.valA.ensure(NF * 4)) || (rc = b.valB.ensure(NF * 4)) ||
      (rc = b.span.ensure(NF * 8)) || (rc = b.scan.ensure(NF * 8)))
    return rc;
  auto sort_by_key = [&](void *tmp, size_t &bytes) {
    return sort_span_keys(tmp, bytes, b.keyA.as<uint64_t>(), b.keyB.as<uint64_t>(), b.valA.as<uint32_t>(), b.valB.as<uint32_t>(), NF, bits, ctx->stream);
  };
  auto scan_spans = [&](void *tmp, size_t &bytes) {
    return rocprim::inclusive_scan(tmp, bytes, b.span.as<uint64_t>(), b.scan.as<uint64_t>(), NF, rocprim::maximum<uint64_t>(), ctx->stream);
  };
  size_t tmp_sort = 0, tmp_scan = 0;
  PRB_HIP(sort_by_key(nullptr, tmp_sort));
  PRB_HIP(scan_spans(nullptr, tmp_scan));
  if ((rc = b.sortTmp.ensure(std::max<size_t>({tmp_sort, tmp_scan, 1})))) return rc;
  PRB_HIP(keys());
  PRB_HIP(sort_by_key(b.sortTmp.p, tmp_sort));
  PRB_HIP(spans());
  PRB_HIP(scan_spans(b.sortTmp.p, tmp_scan));
  return PRB_OK;
}

// What a finish reads of its table's P slots: the two difference arrays and the scratch columns their counts are scanned
// into (free once everything is merged), where the selected slots go, the table's flag of a span out of place and what
// to say of it, and the most slots that can be selected
struct SpanFinish {
  size_t P;
  const unsigned long long *hdiff;
  int64_t *hits;
  int32_t *cdiff;
  int32_t *counts;
  uint32_t *selected;
  const uint32_t *bad;
  const char *bad_span;
  size_t most;
  const char *bad_count;
};
// The counts scanned, the slots that `pick` takes selected in order and, where there are any, `rows` sized to them,
// rows_kernel(how many, b.span.p) enqueued and its records copied to `rows`.  (The scans and the select share b.sortTmp:
// all are sized before the first is enqueued.)  Synchronises.
template <class Pick, class Row, class RowsKernel>
static int select_rows(const char *fn_name, prb_ctx *ctx, SpanBufs &b, const SpanFinish &f, Pick pick, std::vector<Row> &rows, RowsKernel rows_kernel) {
  int rc;
  if ((rc = b.keyA.ensure(16))) return rc;
  auto scan_hits = [&](void *tmp, size_t &bytes) {
    return rocprim::inclusive_scan(tmp, bytes, reinterpret_cast<const int64_t *>(f.hdiff), f.hits, f.P, rocprim::plus<int64_t>(), ctx->stream);
  };
  auto scan_counts = [&](void *tmp, size_t &bytes) {
    return rocprim::inclusive_scan(tmp, bytes, f.cdiff, f.counts, f.P, rocprim::plus<int32_t>(), ctx->stream);
  };
  auto select_picked = [&](void *tmp, size_t &bytes) {
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), f.selected, b.keyA.as<size_t>(), f.P, pick, ctx->stream);
  };
  size_t tmp_h = 0, tmp_c = 0, tmp_s = 0;
  PRB_HIP(scan_hits(nullptr, tmp_h));
  PRB_HIP(scan_counts(nullptr, tmp_c));
  PRB_HIP(select_picked(nullptr, tmp_s));
  if ((rc = b.sortTmp.ensure(std::max<size_t>({tmp_h, tmp_c, tmp_s, 1})))) return rc;
  PRB_HIP(scan_hits(b.sortTmp.p, tmp_h));
  PRB_HIP(scan_counts(b.sortTmp.p, tmp_c));
  PRB_HIP(select_picked(b.sortTmp.p, tmp_s));
  size_t nsel = 0;
  uint32_t bad = 0;
  PRB_HIP(hipMemcpyAsync(&nsel, b.keyA.p, sizeof nsel, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipMemcpyAsync(&bad, f.bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if (bad || nsel > f.most) return refuse(fn_name, bad ? f.bad_span : f.bad_count, PRB_ERR_STATE);
  if (!nsel) return PRB_OK;
  try {
    rows.resize(nsel);
  } catch (const std::exception &e) {
    return refuse(fn_name, e.what(), PRB_ERR_NOMEM);
  }
  if ((rc = b.span.ensure(nsel * sizeof(Row)))) return rc;
  PRB_HIP(rows_kernel((int64_t)nsel, b.span.p));
  PRB_HIP(hipMemcpyAsync(rows.data(), b.span.p, nsel * sizeof(Row), hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  return PRB_OK;
}

// ---- the per-position profile (prb_profset_*) ----
// every slot of the table back to "no hit", on its own device and stream; its stream is idle on return
static int clear_profile_table(prb_profset &ps) {
  hipStream_t stream = ps.ctx->stream;
  const size_t P = (size_t)ps.slots();
  const ProfTab t = ps.view();
  PRB_HIP(hipSetDevice(ps.ctx->device));
  PRB_HIP(hipMemsetAsync(ps.table.p, 0, ps.bytes(), stream));
  PRB_HIP(hipMemsetAsync(t.key, 0xFF, 3 * P * 8, stream)); // key, tie, skey: none yet
  PRB_HIP(hipMemsetAsync(t.stie, 0xFF, P * 4, stream));
  PRB_HIP(hipMemcpyAsync(ps.table.p, ps.off.data(), ps.off.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipStreamSynchronize(stream));
  return PRB_OK;
}

// prb_search_page_profile, per sub-batch: the hits by (pair, first position of the span), the running maximum of the
// spans' ends per pair, the difference arrays, the sub-batch's best hit per position and its merge into the table's, in
// a bracket of the "profile" timer
static int merge_profile(prb_ctx *ctx, prb_profset *ps, int32_t page, int32_t q0, int32_t q1, const HitSoA &F, int64_t nfin, const int32_t *ends,
                       const uint32_t *pair_start, int64_t npairs) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  const ProfTab t = ps->view();
  // the pair index above bit 32, as many bits as it needs
  int bits = 32;
  while (bits < 64 && ((uint64_t)(npairs - 1) >> (bits - 32)) != 0) bits++;
  // (pair << 32 | 1 + last position: the running maximum of a pair never looks past the pair's own hits)
  if ((rc = order_spans(
           ctx, *ps, (size_t)nfin, bits,
           [&] { return launch_prof_keys(nfin, pair_start, npairs, ends, ps->keyA.as<uint64_t>(), ps->valA.as<uint32_t>(), ctx->stream); },
           [&] { return launch_prof_span(nfin, ps->keyB.as<uint64_t>(), ps->valB.as<uint32_t>(), ends, ps->span.as<uint64_t>(), ctx->stream); })))
    return rc;
  PRB_HIP(launch_prof_add(F, nfin, ps->keyB.as<uint64_t>(), ps->valB.as<uint32_t>(), ps->scan.as<uint64_t>(), ends, t, ctx->stream));
  PRB_HIP(launch_prof_min(F, nfin, ps->valB.as<uint32_t>(), ends, t, ctx->stream));
  PRB_HIP(launch_prof_merge(F, ends, t, ps->off[(size_t)q0], ps->off[(size_t)q1], page, ctx->stream));
  return ctx->time_end(ModeTimer::kProfile, 8);
}
int prb_profset::take(const SubBatch &b) { return merge_profile(ctx, this, b.page, b.q0, b.q1, b.F, b.nfin, b.ends, b.pair_start, b.npairs); }

// ---- the per-target coverage (prb_covset_*) ----
// every slot of the table back to "no hit", on its own device and stream; its stream is idle on return
static int clear_coverage_table(prb_covset &cs) {
  hipStream_t stream = cs.ctx->stream;
  const size_t P = (size_t)cs.slots();
  const CovTab t = cs.view();
  PRB_HIP(hipSetDevice(cs.ctx->device));
  PRB_HIP(hipMemsetAsync(cs.table.p, 0, cs.bytes(), stream));
  if (P) PRB_HIP(hipMemsetAsync(t.key, 0xFF, 4 * P * 8, stream)); // key, tie, skey, stie: none yet
  PRB_HIP(hipMemcpyAsync(cs.table.p, cs.seq_lo.data(), cs.seq_lo.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipMemcpyAsync(cs.table.as<int64_t>() + cs.seq_lo.size(), cs.tbase.data(), cs.tbase.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipStreamSynchronize(stream));
  return PRB_OK;
}

// What prb_search_page_coverage and prb_covset_add_hits share: the list by (query, first position of the span) - a
// sequence's positions are contiguous in the page's text, so that is by (query, target, first position) -, the running
// maximum of the spans' ends per query, the difference arrays, and the four passes of the best hits.  In a bracket of
// the "coverage" timer.
static int merge_coverage(prb_ctx *ctx, prb_covset *cs, int32_t page, const CovHits &h, int32_t nq) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = cs->place.ensure((size_t)h.n * 4))) return rc;
  const CovTab t = cs->view();
  const CovPage pg = cs->page_view((size_t)page);
  uint32_t *place = cs->place.as<uint32_t>();
  const int bits = 32 + bits_for(std::max(nq - 1, 1)); // the position, and above it the query
  if ((rc = order_spans(
           ctx, *cs, (size_t)h.n, bits, [&] { return launch_cov_keys(h, t, pg, cs->keyA.as<uint64_t>(), cs->valA.as<uint32_t>(), place, ctx->stream); },
           [&] { return launch_cov_span(h, cs->keyB.as<uint64_t>(), cs->valB.as<uint32_t>(), t, pg, cs->span.as<uint64_t>(), ctx->stream); })))
    return rc;
  PRB_HIP(launch_cov_add(h, cs->keyB.as<uint64_t>(), cs->valB.as<uint32_t>(), cs->scan.as<uint64_t>(), t, pg, ctx->stream));
  PRB_HIP(launch_cov_min(h, cs->valB.as<uint32_t>(), place, cs->ids.as<int32_t>(), t, pg, ctx->stream));
  return ctx->time_end(ModeTimer::kCoverage, 9);
}
int prb_covset::take(const SubBatch &b) {
  return merge_coverage(ctx, this, b.page, CovHits{b.nfin, b.F.query, b.F.db_id, b.F.e_tot, b.ends}, b.nq);
}

extern "C" {

int prb_profset_create(prb_ctx *ctx, const prb_qbatch *qb, prb_profset **out) {
  std::unique_ptr<prb_profset> ps;
  if (int rc = new_table("prb_profset_create", ctx && qb, out, ps)) return rc;
  ps->ctx = ctx;
  ps->qb = qb;
  ps->nq = qb->nq;
  ps->qlen = qb->len;
  ps->off.assign((size_t)qb->nq + 1, 0);
  for (int32_t q = 0; q < qb->nq; q++) ps->off[(size_t)q + 1] = ps->off[(size_t)q] + qb->len[(size_t)q] + 1;
  PRB_HIP(hipSetDevice(ctx->device));
  if (ps->table.ensure(ps->bytes()) != PRB_OK)
    return refuse("prb_profset_create", "can't allocate the per-position table (" + std::to_string(ps->bytes() >> 20) + " MB of HBM for " +
                                            std::to_string(ps->slots()) + " query positions)",
                  PRB_ERR_NOMEM);
  if (int rc = clear_profile_table(*ps)) return rc;
  *out = ps.release();
  return PRB_OK;
}

int prb_profset_merge(prb_ctx *ctx, prb_profset *dst, prb_profset *src) {
  if (int rc = merge_tables_guard("prb_profset_merge", "profile", ctx, dst, src)) return rc;
  return join_tables(
      "prb_profset_merge", ModeTimer::kProfile, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_prof_join(dst->view(), dst->view_of(static_cast<char *>(block)), dst->slots(), ctx->stream));
        return PRB_OK;
      },
      clear_profile_table);
}

int prb_search_page_profile(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_profset *ps) {
  return merge_page("prb_search_page_profile", "profile", "prb_profset_finish", ps, ctx, qb, db, page, opts);
}

// the covered positions selected on the device (Hits > 0 after the scans), their rows built there and copied once
int prb_profset_finish(prb_ctx *ctx, prb_profset *ps) {
  if (int rc = finish_guard("prb_profset_finish", "profile", ctx, ps)) return rc;
  if (ps->finished) return PRB_OK; // (the rows are on the host already)
  const size_t P = (size_t)ps->slots();
  ps->rows.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (P > 0) {
    int rc;
    if ((rc = ctx->time_begin())) return rc;
    const ProfTab t = ps->view();
    // counts: hits into skey's slots, targets into stie's
    int64_t *hits = reinterpret_cast<int64_t *>(t.skey);
    int32_t *targets = reinterpret_cast<int32_t *>(t.stie);
    if ((rc = ps->valA.ensure(P * 4))) return rc;
    const SpanFinish f{P, t.hdiff, hits, t.tdiff, targets, ps->valA.as<uint32_t>(), t.bad, "a final hit's span lies outside its query", P, "bad row count"};
    if ((rc = select_rows("prb_profset_finish", ctx, *ps, f, ProfCovered{hits}, ps->rows, [&](int64_t nsel, void *rows) {
           return launch_prof_rows(t, f.selected, nsel, hits, targets, rows, ctx->stream);
         })))
      return rc;
    if ((rc = ctx->time_end(ModeTimer::kProfile, ps->rows.empty() ? 3 : 4))) return rc;
  }
  ps->finished = true;
  ps->release(); // (only the host rows are needed from here on)
  return PRB_OK;
}

int64_t prb_profset_size(const prb_profset *ps) { return ps ? (int64_t)ps->rows.size() : -1; }
const prb_profile_pos *prb_profset_rows(const prb_profset *ps) { return ps ? ps->rows.data() : nullptr; }
void prb_profset_counts(const prb_profset *ps, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ps ? ps->counts[i] : 0;
}
void prb_profset_free(prb_profset *ps) {
  delete ps;
}

int prb_covset_create(prb_ctx *ctx, prb_db *db, prb_covset **out) {
  std::unique_ptr<prb_covset> cs;
  if (int rc = new_table("prb_covset_create", ctx && db && db->ctx->device == ctx->device, out, cs)) return rc;
  cs->ctx = ctx;
  cs->db = db;
  try {
    cs->tbase.assign(db->pages.size() + 1, 0);
    cs->slot0.assign(db->pages.size() + 1, 0);
    for (size_t p = 0; p < db->pages.size(); p++) {
      const DbPage &pg = db->pages[p];
      cs->tbase[p + 1] = cs->tbase[p] + pg.nseq;
      for (int32_t i = 0; i < pg.nseq; i++) cs->seq_lo.push_back(cs->slot0[p] + pg.start_pos[(size_t)i]);
      cs->slot0[p + 1] = cs->slot0[p] + (int64_t)pg.seqs.size(); // (the text: every sequence and the separator behind it)
    }
    cs->seq_lo.push_back(cs->slot0.back());
    cs->merged.resize(db->pages.size());
  } catch (const std::exception &e) {
    return refuse("prb_covset_create", e.what(), PRB_ERR_NOMEM);
  }
  if (cs->slots() > (int64_t)UINT32_MAX)
    return refuse("prb_covset_create", "the database has " + std::to_string(cs->slots()) + " positions (at most 2^32 - 1)");
  PRB_HIP(hipSetDevice(ctx->device));
  if (cs->table.ensure(cs->bytes()) != PRB_OK)
    return refuse("prb_covset_create", "can't allocate the coverage table (" + std::to_string(cs->bytes() >> 20) + " MB of HBM for " +
                                           std::to_string(cs->slots()) + " positions of " + std::to_string(cs->targets()) + " targets)",
                  PRB_ERR_NOMEM);
  if (int rc = clear_coverage_table(*cs)) return rc;
  *out = cs.release();
  return PRB_OK;
}

int prb_search_page_coverage(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *query_ids,
                             prb_covset *cs) {
  return merge_run_page("prb_search_page_coverage", "coverage", "prb_covset_finish", cs, ctx, qb, db, page, opts, query_ids);
}

// the caller's list checked on the host - a refused call leaves the table as it was -, then as columns to the device and
// through the merge of a sub-batch
int prb_covset_add_hits(prb_ctx *ctx, prb_covset *cs, int32_t page, const int32_t *query_ids, int32_t nq, const prb_hit *hits, int64_t nhits,
                        const int32_t *basepairs, int64_t npairs) {
  const std::string fn = "prb_covset_add_hits";
  if (!ctx || !cs || nq < 0 || (nq && !query_ids) || nhits < 0 || nhits > INT32_MAX || npairs < 0 || (nhits && (!hits || !basepairs)))
    return refuse(fn, "bad argument");
  if (page < 0 || (size_t)page >= cs->merged.size()) return refuse(fn, "page " + std::to_string(page) + " out of range");
  const CovPage pg = cs->page_view((size_t)page);
  std::vector<int32_t> query, db_id, ends;
  std::vector<double> e_tot;
  try {
    query.resize((size_t)nhits);
    db_id.resize((size_t)nhits);
    e_tot.resize((size_t)nhits);
    ends.resize((size_t)nhits * 4);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  for (int64_t i = 0; i < nhits; i++) {
    const prb_hit &x = hits[i];
    if (x.query < 0 || x.query >= nq || (i && x.query < hits[i - 1].query) || x.db_id < 0 || x.db_id >= pg.nseq || x.bp_count < 1 ||
        x.bp_offset < 0 || x.bp_offset + x.bp_count > npairs)
      return refuse(fn, "hit record " + std::to_string(i) + " is inconsistent");
    const int32_t *first = basepairs + 2 * x.bp_offset, *last = basepairs + 2 * (x.bp_offset + x.bp_count - 1);
    const int64_t lo = std::min(first[1], last[1]), hi = std::max(first[1], last[1]);
    const int64_t s0 = cs->seq_lo[(size_t)(pg.target0 + x.db_id)] - pg.slot0, sep = cs->seq_lo[(size_t)(pg.target0 + x.db_id) + 1] - pg.slot0 - 1;
    if (lo < s0 || hi >= sep) return refuse(fn, "the span of hit record " + std::to_string(i) + " leaves its sequence", PRB_ERR_STATE);
    query[(size_t)i] = x.query;
    db_id[(size_t)i] = x.db_id;
    e_tot[(size_t)i] = x.e_tot;
    ends[4 * (size_t)i] = first[0], ends[4 * (size_t)i + 1] = first[1], ends[4 * (size_t)i + 2] = last[0], ends[4 * (size_t)i + 3] = last[1];
  }
  if (int rc = run_table_guard(fn, "coverage", "prb_covset_finish", cs, ctx, cs->db, page, -1, -1, query_ids, nq)) return rc;
  if (!nhits) return PRB_OK;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  cs->broken = true; // (until the merge is whole)
  int rc;
  const size_t N = (size_t)nhits;
  if ((rc = upload_ids(ctx, cs, query_ids, nq))) return rc;
  if ((rc = cs->h_query.ensure(N * 4)) || (rc = cs->h_db_id.ensure(N * 4)) || (rc = cs->h_e_tot.ensure(N * 8)) || (rc = cs->h_ends.ensure(N * 16)))
    return rc;
  PRB_HIP(hipMemcpyAsync(cs->h_query.p, query.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_db_id.p, db_id.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_e_tot.p, e_tot.data(), N * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_ends.p, ends.data(), N * 16, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the vectors go)
  if ((rc = merge_coverage(ctx, cs, page, CovHits{nhits, cs->h_query.as<int32_t>(), cs->h_db_id.as<int32_t>(), cs->h_e_tot.as<double>(),
                                                  cs->h_ends.as<int32_t>()},
                           nq)))
    return rc;
  cs->broken = false;
  return PRB_OK;
}

int prb_covset_merge(prb_ctx *ctx, prb_covset *dst, prb_covset *src) {
  if (int rc = run_tables_guard("prb_covset_merge", "coverage", ctx, dst, src, [&]() -> std::string {
        return dst->seq_lo == src->seq_lo ? "" : "the coverage tables were made for different databases";
      }))
    return rc;
  return join_tables(
      "prb_covset_merge", ModeTimer::kCoverage, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_cov_join(dst->view(), dst->view_of(static_cast<char *>(block)), dst->slots(), ctx->stream));
        return PRB_OK;
      },
      clear_coverage_table);
}

// the counts scanned into the scratch columns, the regions' first slots selected, a wavefront per region, one copy
int prb_covset_finish(prb_ctx *ctx, prb_covset *cs, int32_t min_queries) {
  if (int rc = finish_guard("prb_covset_finish", "coverage", ctx, cs)) return rc;
  if (cs->finished) return PRB_OK; // (the records are on the host already)
  if (min_queries < 1 || min_queries > 1000000)
    return refuse("prb_covset_finish", "need 1 <= min_queries <= 1000000 (got " + std::to_string(min_queries) + ")");
  const size_t P = (size_t)cs->slots();
  cs->regions.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (P > 0) {
    int rc;
    if ((rc = ctx->time_begin())) return rc;
    const CovTab t = cs->view();
    // counts: hits into skey's slots, queries into the first half of stie's; the regions' first slots (at most one for
    // two slots) into the second half
    int64_t *hits = reinterpret_cast<int64_t *>(t.skey);
    int32_t *queries = reinterpret_cast<int32_t *>(t.stie);
    const SpanFinish f{P,     t.hdiff, hits, t.qdiff, queries, reinterpret_cast<uint32_t *>(t.stie) + P, t.bad, "a final hit's span leaves its sequence",
                       (P + 1) / 2, "bad region count"};
    if ((rc = select_rows("prb_covset_finish", ctx, *cs, f, CovHead{queries, min_queries}, cs->regions, [&](int64_t nreg, void *rows) {
           return launch_cov_regions(t, cs->tbase_dev(), (int32_t)cs->merged.size(), cs->targets(), f.selected, nreg, hits, queries, min_queries, rows,
                                     ctx->stream);
         })))
      return rc;
    // (the slots run along the page's text, which holds the sequences reversed: a target's regions arrive by start
    // descending)
    const size_t nreg = cs->regions.size();
    for (size_t i = 0, j; i < nreg; i = j) {
      for (j = i + 1; j < nreg && cs->regions[j].page == cs->regions[i].page && cs->regions[j].db_id == cs->regions[i].db_id;) j++;
      std::reverse(cs->regions.begin() + (ptrdiff_t)i, cs->regions.begin() + (ptrdiff_t)j);
    }
    if ((rc = ctx->time_end(ModeTimer::kCoverage, nreg ? 4 : 3))) return rc;
  }
  cs->finished = true;
  cs->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_covset_size(const prb_covset *cs) { return cs ? (int64_t)cs->regions.size() : -1; }
const prb_target_region *prb_covset_regions(const prb_covset *cs) { return cs ? cs->regions.data() : nullptr; }
void prb_covset_counts(const prb_covset *cs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = cs ? cs->counts[i] : 0;
}
void prb_covset_free(prb_covset *cs) {
  delete cs;
}

} // extern "C"
