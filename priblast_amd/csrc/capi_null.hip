// C ABI, part 10: the null table of one batch - per observed (query, target) pair, how the query's decoys fare against
// the same target (prb_nullset_*, `ris -t -z N [-H H]`).  The kernels are in null_kernels.hip.  Every check of a call is made on
// the host before anything is enqueued: a refused call leaves the table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kFinishFn = "prb_nullset_finish";

// What every call that merges into the table checks of it first
int null_guard(const std::string &fn, const prb_ctx *ctx, const prb_nullset *ns, int32_t page) {
  if (!ctx || !ns) return refuse(fn, "bad argument");
  if (ns->ctx != ctx) return refuse(fn, "the null table was made with another context");
  if (ns->broken) return refuse(fn, "an earlier merge into this null table failed", PRB_ERR_STATE);
  if (ns->bad) return refuse(fn, "a record merged into this null table named a query, a sequence, an owner or a decoy outside it", PRB_ERR_STATE);
  if (ns->finished) return refuse(fn, std::string("the null table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  if (page < 0 || (size_t)page >= ns->observed.size())
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(ns->observed.size()) + ")");
  return PRB_OK;
}

// the real batch's page: observed once
int observed_guard(const std::string &fn, const prb_nullset *ns, int32_t page) {
  if (ns->observed[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already observed in this null table");
  return PRB_OK;
}

// A batch of ndq decoys for `page`: the page is observed, and the batch is new to the page (decoys_guard over the page's bits)
int decoy_batch_guard(const std::string &fn, const prb_nullset *ns, int32_t page, const int32_t *owner, const int32_t *decoy, int32_t ndq) {
  if (!ns->observed[(size_t)page])
    return refuse(fn, "page " + std::to_string(page) + " is not observed yet (the real batch's search comes first)", PRB_ERR_STATE);
  return decoys_guard(fn, ns, ns->bit0(page), owner, decoy, ndq, " is already merged for page " + std::to_string(page));
}

// A caller's list of pair records of `page` (its queries below nq_list)
int page_list_guard(const std::string &fn, const prb_nullset *ns, int32_t page, int32_t nq_list, const prb_pair_summary *pairs, int64_t n) {
  return records_guard(fn, ns->tbase[(size_t)page + 1] - ns->tbase[(size_t)page], nq_list, pairs, n);
}

} // namespace

// prb_search_page_observed (per sub-batch) and prb_nullset_observe: the records into their slots, in a bracket of the
// "null" timer
static int merge_null_observed(prb_ctx *ctx, prb_nullset *ns, int32_t page, const void *packed, int64_t npairs) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_null_observe(packed, npairs, ns->view(), ns->page_view((size_t)page), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kNull, 1))) return rc;
  return fetch_bad(ctx, ns);
}
// prb_search_page_decoys (per sub-batch) and prb_nullset_add_pairs: the records folded into the counters, likewise
static int merge_null_decoys(prb_ctx *ctx, prb_nullset *ns, int32_t page, const void *packed, int64_t npairs) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_null_count(packed, npairs, ns->own.as<int32_t>(), ns->own.as<int32_t>() + ns->ndq, ns->ndq, ns->view(),
                            ns->page_view((size_t)page), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kNull, 1))) return rc;
  return fetch_bad(ctx, ns);
}
// a sub-batch of the batch being searched: a decoy batch's while prb_search_page_decoys says so, else the real one's
int prb_nullset::take(const SubBatch &b) {
  return decoy_phase ? merge_null_decoys(ctx, this, b.page, b.records, b.npairs) : merge_null_observed(ctx, this, b.page, b.records, b.npairs);
}

extern "C" {

int prb_nullset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t ndecoys, prb_nullset **out) {
  const char *fn = "prb_nullset_create";
  std::unique_ptr<prb_nullset> ns;
  const bool args_ok = ctx && qb && db && qb->ctx->device == ctx->device && db->ctx->device == ctx->device;
  if (int rc = new_table(fn, args_ok, out, ns,
                         ndecoys < 1 || ndecoys > 100000 ? "need 1 <= ndecoys <= 100000 (got " + std::to_string(ndecoys) + ")" : ""))
    return rc;
  try {
    ns->tbase.assign(db->pages.size() + 1, 0);
    for (size_t p = 0; p < db->pages.size(); p++) ns->tbase[p + 1] = ns->tbase[p] + db->pages[p].nseq;
    ns->observed.assign(db->pages.size(), 0);
    ns->npages = (int32_t)db->pages.size();
    ns->nq = qb->nq;
    ns->ndecoys = ndecoys;
    ns->merged.assign((size_t)((ns->triples() + 63) / 64), 0);
    ns->live_q.assign((size_t)ns->nq, -1);
    ns->needs.assign((size_t)ns->nq, ndecoys);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  if (ns->slots() > (int64_t)UINT32_MAX)
    return refuse(fn, "the batch and the database have " + std::to_string(ns->slots()) + " (query, target) pairs (at most 2^32 - 1)");
  ns->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  ns->db = db;
  ns->qb = qb;
  PRB_HIP(hipSetDevice(ctx->device));
  const size_t S = (size_t)ns->slots();
  if (ns->table.ensure(std::max<size_t>(S * sizeof(NullSlot), 16)) != PRB_OK || ns->obs.ensure(std::max<size_t>(S, 16)) != PRB_OK ||
      ns->live.ensure(std::max<size_t>(S, 16)) != PRB_OK || ns->live_dev.ensure(std::max<size_t>((size_t)ns->nq * 8, 16)) != PRB_OK ||
      ns->badflag.ensure(16) != PRB_OK || ns->tbase_dev.ensure(ns->tbase.size() * 8) != PRB_OK)
    return refuse(fn, "can't allocate the null table (" + std::to_string((S * (sizeof(NullSlot) + 2)) >> 20) + " MB of HBM for " + std::to_string(ns->nq) +
                          " queries x " + std::to_string(ns->targets()) + " targets)",
                  PRB_ERR_NOMEM);
  PRB_HIP(hipMemsetAsync(ns->badflag.p, 0, 16, ctx->stream));
  PRB_HIP(hipMemcpyAsync(ns->tbase_dev.p, ns->tbase.data(), ns->tbase.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(launch_null_clear(ns->view(), ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  *out = ns.release();
  return PRB_OK;
}

int prb_search_page_observed(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_nullset *ns) {
  const char *fn = "prb_search_page_observed";
  if (!ns) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, qb, db, page, opts, 3)) return rc;
  if (ns->qb != qb || ns->nq != qb->nq || ns->db != db) return refuse(fn, "the null table was made for another query batch or another database");
  if (int rc = null_guard(fn, ctx, ns, page)) return rc;
  if (int rc = selection_guard(fn, "null table", ns, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, qb, db, opts)) return rc;
  if (int rc = observed_guard(fn, ns, page)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  ns->observed[(size_t)page] = 1;
  ns->broken = true; // (until the merge is whole)
  if (int rc = search_into_table(ns, ctx, qb, db, page, opts, ns->counts)) return rc;
  ns->broken = false;
  return PRB_OK;
}

int prb_search_page_decoys(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *owner,
                           const int32_t *decoy, prb_nullset *ns) {
  const char *fn = "prb_search_page_decoys";
  if (!ns || !owner || !decoy) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, dqb, db, page, opts, 3)) return rc;
  if (ns->db != db) return refuse(fn, "the null table was made for another database");
  if (int rc = null_guard(fn, ctx, ns, page)) return rc;
  if (int rc = selection_guard(fn, "null table", ns, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, dqb, db, opts)) return rc;
  if (int rc = decoy_batch_guard(fn, ns, page, owner, decoy, dqb->nq)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  ns->broken = true; // (until the merge is whole)
  mark_decoys(ns, ns->bit0(page), owner, decoy, dqb->nq);
  if (int rc = upload_owners(ctx, ns, owner, decoy, dqb->nq)) return rc;
  ns->decoy_phase = true;
  const int rc = search_into_table(ns, ctx, dqb, db, page, opts, ns->decoy_counts, false);
  ns->decoy_phase = false;
  if (rc) return rc;
  ns->broken = false;
  return PRB_OK;
}

int prb_nullset_observe(prb_ctx *ctx, prb_nullset *ns, int32_t page, const prb_pair_summary *pairs, int64_t n) {
  const char *fn = "prb_nullset_observe";
  if (n < 0 || n > INT32_MAX || (n && !pairs)) return refuse(fn, "bad argument");
  if (int rc = null_guard(fn, ctx, ns, page)) return rc;
  if (int rc = observed_guard(fn, ns, page)) return rc;
  if (int rc = page_list_guard(fn, ns, page, ns->nq, pairs, n)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  ns->observed[(size_t)page] = 1;
  if (!n) return PRB_OK;
  ns->broken = true; // (until the merge is whole)
  if (int rc = upload_records(ctx, ns->h_rec, pairs, n)) return rc;
  if (int rc = merge_null_observed(ctx, ns, page, ns->h_rec.p, n)) return rc;
  ns->broken = false;
  return PRB_OK;
}

int prb_nullset_add_pairs(prb_ctx *ctx, prb_nullset *ns, int32_t page, const int32_t *owner, const int32_t *decoy, int32_t nq,
                          const prb_pair_summary *pairs, int64_t n) {
  const char *fn = "prb_nullset_add_pairs";
  if (nq < 0 || (nq && (!owner || !decoy)) || n < 0 || n > INT32_MAX || (n && !pairs)) return refuse(fn, "bad argument");
  if (int rc = null_guard(fn, ctx, ns, page)) return rc;
  if (int rc = decoy_batch_guard(fn, ns, page, owner, decoy, nq)) return rc;
  if (int rc = page_list_guard(fn, ns, page, nq, pairs, n)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  mark_decoys(ns, ns->bit0(page), owner, decoy, nq);
  if (!n) return PRB_OK; // (decoys without a hit: they are merged)
  ns->broken = true; // (until the merge is whole)
  if (int rc = upload_owners(ctx, ns, owner, decoy, nq)) return rc;
  if (int rc = upload_records(ctx, ns->h_rec, pairs, n)) return rc;
  if (int rc = merge_null_decoys(ctx, ns, page, ns->h_rec.p, n)) return rc;
  ns->broken = false;
  return PRB_OK;
}

// prb_nullset_finish_fdr, between the selection and the gather: the figures of the nsel selected slots ns->sel into
// ns->fdr_out, in the selection's order.  Two brackets of the "fdr" timer: the key pass, which also counts the observed
// pairs per query - the host checks `tests` against the counts and turns them into the segments' bounds -, then the sort
// by (query, p-key) - capi_search.hip's (search_host.hpp: no sort is instantiated here) -, the rank pass, the step-up pass
// and the scatter.  A refusal of `tests` leaves the table as it was.
static int rank_fdr(const char *fn, prb_ctx *ctx, prb_nullset *ns, int64_t nsel, const int64_t *tests) {
  const size_t n = (size_t)nsel, NQ = (size_t)ns->nq;
  int rc;
  ScratchBuf keyA, keyB, valA, valB, frac, ent, qv, cnt, off, tests_dev, tmp;
  if ((rc = keyA.ensure(n * 8)) || (rc = keyB.ensure(n * 8)) || (rc = valA.ensure(n * 4)) || (rc = valB.ensure(n * 4)) || (rc = frac.ensure(n * 8)) ||
      (rc = ent.ensure(n * 16)) || (rc = qv.ensure(n * 16)) || (rc = cnt.ensure(NQ * 4)) || (rc = off.ensure((NQ + 1) * 8)) ||
      (rc = tests_dev.ensure(NQ * 8)) || (rc = ns->fdr_out.ensure(n * sizeof(prb_null_fdr))))
    return rc;
  const int bits = kFdrKeyBits + bits_for(std::max(0, ns->nq - 1));
  auto sort_keys = [&](void *t, size_t &b) {
    return sort_span_keys(t, b, keyA.as<uint64_t>(), keyB.as<uint64_t>(), valA.as<uint32_t>(), valB.as<uint32_t>(), n, bits, ctx->stream);
  };
  size_t tmp_bytes = 0;
  PRB_HIP(sort_keys(nullptr, tmp_bytes));
  if ((rc = tmp.ensure(std::max<size_t>(tmp_bytes, 16)))) return rc;
  std::vector<uint32_t> c;
  std::vector<int64_t> o, tq;
  try {
    c.assign(NQ, 0);
    o.assign(NQ + 1, 0);
    tq.assign(NQ, ns->targets());
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(hipMemsetAsync(cnt.p, 0, NQ * 4, ctx->stream));
  PRB_HIP(launch_fdr_keys(ns->view(), ns->sel.as<uint32_t>(), nsel, keyA.as<unsigned long long>(), valA.as<uint32_t>(), frac.as<uint2>(),
                          cnt.as<uint32_t>(), ctx->stream));
  PRB_HIP(hipMemcpyAsync(c.data(), cnt.p, NQ * 4, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kFdr, 1))) return rc; // (synchronises: the copy is over)
  if ((rc = fetch_bad(ctx, ns))) return rc;
  if (ns->bad) return refuse(fn, "a selected slot lies outside the null table, or its null_le exceeds the decoys it has seen", PRB_ERR_STATE);
  for (size_t q = 0; q < NQ; q++) {
    if (tests) tq[q] = tests[q];
    if ((int64_t)c[q] > tq[q])
      return refuse(fn, "tests[" + std::to_string(q) + "] = " + std::to_string(tq[q]) + " is below the " + std::to_string(c[q]) +
                            " observed pairs of query " + std::to_string(q));
    o[q + 1] = o[q] + (int64_t)c[q];
  }
  if (o[NQ] != nsel) { // (the device's counts and its selection disagree: the table is not to be trusted)
    ns->broken = true;
    return refuse(fn, "the queries' segments hold " + std::to_string(o[NQ]) + " pairs, the selection " + std::to_string(nsel), PRB_ERR_STATE);
  }
  PRB_HIP(hipMemcpyAsync(off.p, o.data(), (NQ + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(tests_dev.p, tq.data(), NQ * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory)
  const FdrTab f{keyB.as<unsigned long long>(), valB.as<uint32_t>(), off.as<int64_t>(), tests_dev.as<int64_t>(), frac.as<uint2>(),
                 ent.as<uint4>(),               qv.as<uint4>(),      ns->badflag.as<uint32_t>(), nsel, ns->nq};
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(sort_keys(tmp.p, tmp_bytes));
  PRB_HIP(launch_fdr_rank(f, ctx->stream));
  PRB_HIP(launch_fdr_stepup(f, ctx->stream));
  PRB_HIP(launch_fdr_scatter(f, ns->fdr_out.p, ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kFdr, 4))) return rc; // (synchronises: the scratch is read no more)
  if ((rc = fetch_bad(ctx, ns))) return rc;
  if (ns->bad) return refuse(fn, "an index of the ranking lies outside its list", PRB_ERR_STATE);
  return PRB_OK;
}

// the observed slots selected on the device, their records gathered there and copied once; with_fdr: their figures
// ranked between the two (rank_fdr) and copied beside them
static int finish_null(const char *fn, prb_ctx *ctx, prb_nullset *ns, bool with_fdr, const int64_t *tests) {
  if (int rc = finish_guard(fn, "null", ctx, ns)) return rc;
  if (ns->finished) return PRB_OK; // (the records are on the host already)
  if (ns->bad) return refuse(fn, "a record merged into this null table named a query, a sequence, an owner or a decoy outside it", PRB_ERR_STATE);
  if (!ns->retired_upto) {
    if (ns->nmerged != ns->triples())
      return refuse(fn, std::to_string(ns->nmerged) + " of " + std::to_string(ns->triples()) + " (query, decoy, page) searches are merged: every decoy of every query against every page comes first",
                    PRB_ERR_STATE);
  } else { // (retired pairs: a query without live pairs needs no decoy from the boundary on that found it so)
    int64_t need = 0, have = 0;
    for (int32_t q = 0; q < ns->nq; q++)
      for (int32_t page = 0; page < ns->npages; page++)
        for (int32_t d = 0; d < ns->needs[(size_t)q]; d++) need++, have += ns->merged_bit(page, q, d);
    if (have != need)
      return refuse(fn, std::to_string(have) + " of " + std::to_string(need) + " (query, decoy, page) searches are merged: every decoy of every query that has live pairs against every page comes first",
                    PRB_ERR_STATE);
  }
  if (with_fdr) {
    if (ns->targets() >= (int64_t)1 << 30)
      return refuse(fn, "the database has " + std::to_string(ns->targets()) + " targets (fewer than 2^30 for the q-values: their cross products stay within 64 bits)");
    if (ns->nq > 1 << 23) return refuse(fn, "the batch has " + std::to_string(ns->nq) + " queries (at most 2^23 for the q-values: the sort key holds the query above 41 bits)");
    for (int32_t q = 0; tests && q < ns->nq; q++)
      if (tests[q] < 1 || tests[q] >= (int64_t)1 << 31)
        return refuse(fn, "need 1 <= tests[q] < 2^31 (tests[" + std::to_string(q) + "] = " + std::to_string(tests[q]) + ")");
  }
  ns->pairs.clear();
  ns->fdr.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  const int64_t S = ns->slots();
  if (S > 0) {
    int rc;
    SearchWs &w = ws_of(ctx);
    if ((rc = ns->sel.ensure((size_t)S * 4)) || (rc = w.count.ensure(16))) return rc;
    if ((rc = ctx->time_begin())) return rc;
    int64_t nsel = 0;
    if ((rc = select_flagged(ctx, w, nullptr, ns->obs.as<uint8_t>(), ns->sel.as<uint32_t>(), (size_t)S, &nsel))) return rc;
    if (nsel < 0 || nsel > S) return refuse(fn, "bad record count " + std::to_string(nsel), PRB_ERR_STATE);
    const bool ranked = with_fdr && nsel > 0;
    if (ranked) { // (the selection's share of the "null" timer; the gather's follows the ranking)
      if ((rc = ctx->time_end(ModeTimer::kNull, 1))) return rc;
      if ((rc = rank_fdr(fn, ctx, ns, nsel, tests))) return rc;
      if ((rc = ctx->time_begin())) return rc;
    }
    if (nsel) {
      try {
        ns->pairs.resize((size_t)nsel);
        if (ranked) ns->fdr.resize((size_t)nsel);
      } catch (const std::exception &e) {
        ns->pairs.clear();
        return refuse(fn, e.what(), PRB_ERR_NOMEM);
      }
      const size_t bytes = (size_t)nsel * sizeof(prb_null_pair);
      if ((rc = ns->out.ensure(bytes))) return rc;
      PRB_HIP(launch_null_gather(ns->view(), ns->sel.as<uint32_t>(), nsel, ns->tbase_dev.as<int64_t>(), (int32_t)ns->observed.size(), ns->out.p,
                                 ctx->stream));
      PRB_HIP(hipMemcpyAsync(ns->pairs.data(), ns->out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
      if (ranked) PRB_HIP(hipMemcpyAsync(ns->fdr.data(), ns->fdr_out.p, (size_t)nsel * sizeof(prb_null_fdr), hipMemcpyDeviceToHost, ctx->stream));
    }
    if ((rc = ctx->time_end(ModeTimer::kNull, ranked ? 1 : nsel ? 2 : 1))) return rc; // (synchronises: the copy is over)
    if ((rc = fetch_bad(ctx, ns))) return rc;
    if (ns->bad) {
      ns->pairs.clear();
      ns->fdr.clear();
      return refuse(fn, "a selected slot lies outside the null table", PRB_ERR_STATE);
    }
  }
  ns->finished = true;
  ns->has_fdr = with_fdr;
  ns->release(); // (only the host records are needed from here on)
  return PRB_OK;
}
int prb_nullset_finish(prb_ctx *ctx, prb_nullset *ns) { return finish_null(kFinishFn, ctx, ns, false, nullptr); }
int prb_nullset_finish_fdr(prb_ctx *ctx, prb_nullset *ns, const int64_t *tests) { return finish_null("prb_nullset_finish_fdr", ctx, ns, true, tests); }

// One pass over the slots (k_null_retire), the live slots left per query counted there and copied to the host
int prb_nullset_retire(prb_ctx *ctx, prb_nullset *ns, int64_t min_le, int32_t upto, int64_t *live_per_query) {
  const char *fn = "prb_nullset_retire";
  if (int rc = null_guard(fn, ctx, ns, 0)) return rc;
  if (upto <= ns->retired_upto || upto > ns->ndecoys)
    return refuse(fn, "need " + std::to_string(ns->retired_upto) + " < upto <= " + std::to_string(ns->ndecoys) + " (got " + std::to_string(upto) +
                          "): above that of the call before, and at most the table's decoys per query");
  if (min_le < 1) return refuse(fn, "need min_le >= 1 (got " + std::to_string(min_le) + ")");
  for (size_t p = 0; p < ns->observed.size(); p++)
    if (!ns->observed[p]) return refuse(fn, "page " + std::to_string(p) + " is not observed yet (the real batch's search comes first)", PRB_ERR_STATE);
  // (a query that has live pairs had them at every call before: its decoys below the last boundary were checked there)
  for (int32_t q = 0; q < ns->nq; q++)
    if (ns->live_q[(size_t)q])
      for (int32_t page = 0; page < ns->npages; page++)
        for (int32_t d = ns->retired_upto; d < upto; d++)
          if (!ns->merged_bit(page, q, d))
            return refuse(fn, "decoy " + std::to_string(d) + " of query " + std::to_string(q) + " is not merged for page " + std::to_string(page) +
                                  ": every decoy below " + std::to_string(upto) + " of every query that has live pairs comes first",
                          PRB_ERR_STATE);
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> left;
  try {
    left.assign((size_t)ns->nq, 0);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  if (ns->slots() > 0) {
    ns->broken = true; // (until the pass is whole)
    int rc;
    if ((rc = ctx->time_begin())) return rc;
    PRB_HIP(hipMemsetAsync(ns->live_dev.p, 0, (size_t)ns->nq * 8, ctx->stream));
    PRB_HIP(launch_null_retire(ns->view(), (unsigned long long)min_le, (uint32_t)upto, ns->live_dev.as<unsigned long long>(), ctx->stream));
    PRB_HIP(hipMemcpyAsync(left.data(), ns->live_dev.p, (size_t)ns->nq * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kNull, 1))) return rc; // (synchronises: the copy is over)
    if ((rc = fetch_bad(ctx, ns))) return rc;
    ns->broken = false;
  }
  for (int32_t q = 0; q < ns->nq; q++) {
    if (ns->live_q[(size_t)q] && !left[(size_t)q]) ns->needs[(size_t)q] = upto;
    ns->live_q[(size_t)q] = left[(size_t)q];
    if (live_per_query) live_per_query[q] = left[(size_t)q];
  }
  ns->retired_upto = upto;
  return PRB_OK;
}

int64_t prb_nullset_size(const prb_nullset *ns) { return ns ? (int64_t)ns->pairs.size() : -1; }
const prb_null_pair *prb_nullset_pairs(const prb_nullset *ns) { return ns ? ns->pairs.data() : nullptr; }
const prb_null_fdr *prb_nullset_fdr(const prb_nullset *ns) { return ns && ns->has_fdr ? ns->fdr.data() : nullptr; }
int32_t prb_fdr_chunk(void) { return kFdrChunk; }
void prb_nullset_counts(const prb_nullset *ns, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ns ? ns->counts[i] : 0;
}
void prb_nullset_decoy_counts(const prb_nullset *ns, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ns ? ns->decoy_counts[i] : 0;
}
void prb_nullset_free(prb_nullset *ns) { delete ns; }

} // extern "C"
