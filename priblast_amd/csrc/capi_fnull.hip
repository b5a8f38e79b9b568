// C ABI, part 16: the feature null table of one batch - per kept (query, feature) record of a finished feature table,
// how the query's decoys fare against the same feature (prb_fnullset_*, `ris -t -A FILE -F N`).  The kernels are in
// fnull_kernels.hip.  Every check of a call is made on the host before anything is enqueued: a refused call leaves the
// table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kFinishFn = "prb_fnullset_finish";
const char *const kBadRecord = "a hit or a record merged into this feature null table named a query, a sequence, a page, a feature, an owner or a "
                               "decoy outside it, or its span left its sequence";

// What every call on an unfinished table checks of it first
int fnull_guard(const std::string &fn, const prb_ctx *ctx, const prb_fnullset *t) {
  if (!ctx || !t) return refuse(fn, "bad argument");
  if (t->ctx != ctx) return refuse(fn, "the feature null table was made with another context");
  if (t->broken) return refuse(fn, "an earlier merge into this feature null table failed", PRB_ERR_STATE);
  if (t->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (t->finished) return refuse(fn, std::string("the feature null table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  return PRB_OK;
}
// ... and a call that merges a page into the open batch
int page_guard(const std::string &fn, const prb_fnullset *t, int32_t page) {
  if (!t->open) return refuse(fn, "no decoy batch is open (prb_fnullset_begin comes first)", PRB_ERR_STATE);
  if (page < 0 || (size_t)page >= t->page_merged.size())
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(t->page_merged.size()) + ")");
  if (t->page_merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged in the open decoy batch");
  return PRB_OK;
}

// the device's `bad` flag to the host: raised = the call is refused
int refuse_if_bad(prb_ctx *ctx, prb_fnullset *t, const char *fn) {
  if (int rc = fetch_bad(ctx, t)) return rc;
  if (t->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  return PRB_OK;
}

} // namespace

// prb_search_page_fnull (per sub-batch) and prb_fnullset_add_hits: the list's items folded into the scratch cells, in a
// bracket of the "fnull" timer.  start == nullptr: the runs of the list are made here first.
static int merge_fnull_hits(prb_ctx *ctx, prb_fnullset *t, int32_t page, const FeatHits &h, const uint32_t *start, int64_t npairs) {
  const char *fn = "prb_search_page_fnull";
  int rc;
  if (page < 0 || (size_t)page >= t->annot->pages.size() || !t->open) return refuse(fn, "page out of range", PRB_ERR_STATE);
  if (h.n <= 0) return PRB_OK;
  if (h.n > (int64_t)UINT32_MAX) return refuse(fn, "a list of " + std::to_string(h.n) + " hits (at most 2^32 - 1)");
  const FeatPage pg = t->annot->page_view((size_t)page);
  const int32_t ndq = (int32_t)t->owner.size();
  if ((rc = ctx->time_begin())) return rc;
  int64_t launches = 0;
  if (!start) {
    if ((rc = hit_list_runs(ctx, h, t->head, t->start, &start, &npairs))) return rc;
    launches += 2;
  }
  if (npairs <= 0 || npairs > h.n) return refuse(fn, std::to_string(npairs) + " pair runs for " + std::to_string(h.n) + " hits", PRB_ERR_STATE);
  const size_t N = (size_t)npairs + 1;
  if ((rc = t->cnt.ensure(N * 4)) || (rc = t->ioff.ensure(N * 8))) return rc;
  PRB_HIP(hipMemsetAsync(t->badflag.p, 0, 16, ctx->stream));
  uint32_t *flags = t->badflag.as<uint32_t>(); // bad, nlong
  FeatWork w{t->cnt.as<int32_t>(), t->ioff.as<int64_t>(), nullptr, nullptr, nullptr, flags + 1, flags};
  PRB_HIP(launch_feat_count(h, start, npairs, pg, ndq, w, ctx->stream));
  auto counts = rocprim::make_transform_iterator(t->cnt.as<int32_t>(), ToI64());
  if ((rc = with_temp(t->scanTmp, "rocprim::exclusive_scan", [&](void *tmp, size_t &b) {
         return rocprim::exclusive_scan(tmp, b, counts, t->ioff.as<int64_t>(), (int64_t)0, N, rocprim::plus<int64_t>(), ctx->stream);
       })))
    return rc;
  launches += 2;
  int64_t nitems = 0;
  PRB_HIP(hipMemcpyAsync(&nitems, t->ioff.as<int64_t>() + npairs, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if (nitems < 0 || nitems > (int64_t)UINT32_MAX)
    return refuse(fn, std::to_string(nitems) + " (pair, feature) items in one sub-batch (at most 2^32 - 1): lower PRB_SEARCH_PAIRS", PRB_ERR_STATE);
  if (nitems > 0) {
    if ((rc = t->long_list.ensure((size_t)nitems * 4))) return rc;
    w.long_list = t->long_list.as<uint32_t>();
    const FNullTab tab = t->view();
    PRB_HIP(launch_fnull_items(h, start, npairs, nitems, pg, w, tab, ctx->stream));
    PRB_HIP(launch_fnull_items_long(h, start, npairs, nitems, pg, w, tab, ctx->stream));
    launches += 2;
  }
  if ((rc = ctx->time_end(ModeTimer::kFnull, launches))) return rc;
  return refuse_if_bad(ctx, t, fn);
}
int prb_fnullset::take(const SubBatch &b) {
  return merge_fnull_hits(ctx, this, b.page, FeatHits{b.nfin, b.F.query, b.F.db_id, b.F.e_tot, b.F.e_acc, b.F.e_hyb, b.ends}, b.pair_start, b.npairs);
}

// prb_fnullset_create, from within the feature table's finish: recs_dev[0, nrec) = the gathered records, still on the
// device, and fs->recs the same on the host.  The table builds the lookup - the keys sorted once with the records'
// indices, the queries' first keys from the host's copy -, the energy keys and the counters.
int prb::keep_feature_records(prb_ctx *ctx, prb_fnullset *t, prb_featset *fs, const void *recs_dev, int64_t nrec) {
  const char *fn = "prb_fnullset_create";
  t->nkept = nrec;
  try {
    t->qoff.assign((size_t)t->nq + 1, 0);
    for (const prb_feature_pair &r : fs->recs) {
      if (r.s.query < 0 || r.s.query >= t->nq) return refuse(fn, "a record of the feature table names a query outside it", PRB_ERR_STATE);
      t->qoff[(size_t)r.s.query + 1]++;
    }
    for (size_t q = 0; q < (size_t)t->nq; q++) t->qoff[q + 1] += t->qoff[q];
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  const size_t K = (size_t)std::max<int64_t>(nrec, 1), Q = t->qoff.size();
  ScratchBuf keyIn, idxIn; // the keys and the records' indices before the sort
  if (t->table.ensure(K * sizeof(GNullCount)) != PRB_OK || t->kept.ensure(K * sizeof(prb_feature_pair)) != PRB_OK || t->key.ensure(K * 8) != PRB_OK ||
      t->rec.ensure(K * 4) != PRB_OK || keyIn.ensure(K * 8) != PRB_OK || idxIn.ensure(K * 4) != PRB_OK || t->qoff_dev.ensure(Q * 8) != PRB_OK ||
      t->badflag.ensure(16) != PRB_OK)
    return refuse(fn, "can't allocate the feature null table (" + std::to_string((K * (sizeof(GNullCount) + sizeof(prb_feature_pair) + 24)) >> 20) +
                          " MB of HBM for " + std::to_string(nrec) + " records)",
                  PRB_ERR_NOMEM);
  int rc;
  PRB_HIP(hipMemsetAsync(t->badflag.p, 0, 16, ctx->stream));
  PRB_HIP(hipMemcpyAsync(t->qoff_dev.p, t->qoff.data(), Q * 8, hipMemcpyHostToDevice, ctx->stream));
  if (nrec > 0) {
    const int bits = 32 + bits_for(std::max<int64_t>(0, (int64_t)t->nq - 1));
    auto sort_keys = [&](void *tmp, size_t &b) {
      return sort_span_keys(tmp, b, keyIn.as<uint64_t>(), t->key.as<uint64_t>(), idxIn.as<uint32_t>(), t->rec.as<uint32_t>(), (size_t)nrec, bits,
                            ctx->stream);
    };
    size_t tmp_bytes = 0;
    PRB_HIP(sort_keys(nullptr, tmp_bytes));
    if ((rc = t->scanTmp.ensure(std::max<size_t>(tmp_bytes, 16)))) return rc;
    if ((rc = ctx->time_begin())) return rc;
    PRB_HIP(launch_fnull_keep(recs_dev, t->view(), t->kept.p, keyIn.as<unsigned long long>(), idxIn.as<uint32_t>(), ctx->stream));
    PRB_HIP(sort_keys(t->scanTmp.p, tmp_bytes));
    PRB_HIP(launch_fnull_order(t->view(), ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kFnull, 3))) return rc;
  }
  if ((rc = refuse_if_bad(ctx, t, fn))) return rc; // (synchronises: the host's qoff is uploaded)
  return PRB_OK;
}

// prb_fnullset_create (n = 0) and prb_fnullset_create_top (n > 0: over each query's n best records, as
// prb_featset_finish_top ranks them - the kept records, the lookup and every scratch are sized by those alone)
static int create_fnullset(const char *fn, prb_ctx *ctx, prb_featset *fs, int32_t ndecoys, int32_t n, prb_fnullset **out) {
  std::unique_ptr<prb_fnullset> t;
  if (int rc = new_table(fn, ctx && fs, out, t,
                         ndecoys < 1 || ndecoys > 100000 ? "need 1 <= ndecoys <= 100000 (got " + std::to_string(ndecoys) + ")" : ""))
    return rc;
  if (int rc = finish_guard(fn, "feature", ctx, fs)) return rc;
  if (fs->bad) return refuse(fn, "a hit merged into the feature table named a query or a sequence outside it, or its span left its sequence", PRB_ERR_STATE);
  if (fs->finished) return refuse(fn, "the feature table is finished already (prb_featset_finish, prb_featset_finish_top)", PRB_ERR_STATE);
  if (!fs->db) return refuse(fn, "no page is merged into the feature table: the real batch against every page comes first", PRB_ERR_STATE);
  for (size_t p = 0; p < fs->merged.size(); p++)
    if (!fs->merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged into the feature table: the real batch against every page comes first", PRB_ERR_STATE);
  try {
    t->page_merged.assign(fs->merged.size(), 0);
    t->merged.assign((size_t)(((int64_t)fs->nq * ndecoys + 63) / 64), 0);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  t->nq = fs->nq;
  t->annot = fs->annot;
  t->ndecoys = ndecoys;
  t->distinct = fs->distinct;
  t->chain = fs->chain;
  t->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  t->db = fs->db;
  if (int rc = finish_featset(fn, ctx, fs, n, t.get())) return rc;
  *out = t.release();
  return PRB_OK;
}

extern "C" {

int prb_fnullset_create(prb_ctx *ctx, prb_featset *fs, int32_t ndecoys, prb_fnullset **out) {
  return create_fnullset("prb_fnullset_create", ctx, fs, ndecoys, 0, out);
}
int prb_fnullset_create_top(prb_ctx *ctx, prb_featset *fs, int32_t ndecoys, int32_t n, prb_fnullset **out) {
  const char *fn = "prb_fnullset_create_top";
  if (const std::string why = bad_n(n); !why.empty()) {
    if (out) *out = nullptr;
    return refuse(fn, why);
  }
  return create_fnullset(fn, ctx, fs, ndecoys, n, out);
}

int prb_fnullset_begin(prb_ctx *ctx, prb_fnullset *t, const int32_t *owner, const int32_t *decoy, int32_t ndq) {
  const char *fn = "prb_fnullset_begin";
  if (int rc = fnull_guard(fn, ctx, t)) return rc;
  if (ndq < 1 || !owner || !decoy) return refuse(fn, "bad argument (a batch has one decoy at least)");
  if (t->open) return refuse(fn, "a decoy batch is open (prb_fnullset_end comes first)", PRB_ERR_STATE);
  if (int rc = decoys_guard(fn, t, 0, owner, decoy, ndq, " belongs to a batch closed before")) return rc;
  // the cells: per decoy as many as its owner has kept records, one behind the other
  std::vector<int64_t> doff;
  try {
    doff.assign((size_t)ndq + 1, 0);
    for (int32_t k = 0; k < ndq; k++) doff[(size_t)k + 1] = doff[(size_t)k] + (t->qoff[(size_t)owner[k] + 1] - t->qoff[(size_t)owner[k]]);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  const int64_t ncells = doff.back();
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // the scratch: every cell is empty between two batches (the close empties what it counts), so only new memory is filled
  const size_t bytes = (size_t)std::max<int64_t>(ncells, 1) * 8;
  const size_t cap_before = t->cell.cap;
  const bool have = t->cell.ensure(bytes) == PRB_OK;
  if (have && t->cell.cap != cap_before) PRB_HIP(hipMemsetAsync(t->cell.p, 0xFF, t->cell.cap, ctx->stream));
  if (!have || t->own.ensure((size_t)ndq * 8) != PRB_OK || t->doff.ensure(((size_t)ndq + 1) * 8) != PRB_OK)
    return refuse(fn, "can't allocate the scratch of the decoy batch (" + std::to_string(bytes >> 20) + " MB of HBM for " + std::to_string(ncells) +
                          " (decoy, kept record) cells of " + std::to_string(ndq) + " decoys); open smaller batches",
                  PRB_ERR_NOMEM);
  PRB_HIP(hipMemcpyAsync(t->doff.p, doff.data(), ((size_t)ndq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = upload_owners(ctx, t, owner, decoy, ndq)) return rc; // (the room is there; synchronises)
  try {
    t->owner.assign(owner, owner + ndq);
    t->decoy.assign(decoy, decoy + ndq);
  } catch (const std::exception &e) {
    t->owner.clear();
    t->decoy.clear();
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  t->ncells = ncells;
  std::fill(t->page_merged.begin(), t->page_merged.end(), 0);
  t->open = true;
  return PRB_OK;
}

int prb_search_page_fnull(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_fnullset *t) {
  const char *fn = "prb_search_page_fnull";
  if (!t) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, dqb, db, page, opts, 3)) return rc;
  if (t->db != db) return refuse(fn, "the feature null table was made for another database");
  if (int rc = fnull_guard(fn, ctx, t)) return rc;
  if (int rc = page_guard(fn, t, page)) return rc;
  if ((size_t)dqb->nq != t->owner.size())
    return refuse(fn, "the open decoy batch has " + std::to_string(t->owner.size()) + " decoys; this query batch has " + std::to_string(dqb->nq));
  if (int rc = selection_guard(fn, "feature null table", t, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, dqb, db, opts)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  t->page_merged[(size_t)page] = 1;
  t->broken = true; // (until the merge is whole)
  if (int rc = search_into_table(t, ctx, dqb, db, page, opts, t->counts, false)) return rc;
  t->broken = false;
  return PRB_OK;
}

int prb_fnullset_add_hits(prb_ctx *ctx, prb_fnullset *t, int32_t page, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                          int64_t npairs) {
  const std::string fn = "prb_fnullset_add_hits";
  if (nhits < 0 || nhits > INT32_MAX || npairs < 0 || (nhits && (!hits || !basepairs))) return refuse(fn, "bad argument");
  if (int rc = fnull_guard(fn, ctx, t)) return rc;
  if (int rc = page_guard(fn, t, page)) return rc;
  HitColumns cols;
  if (int rc = check_hit_list(fn, t->annot->pages[(size_t)page], (int32_t)t->owner.size(), hits, nhits, basepairs, npairs, cols)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  t->page_merged[(size_t)page] = 1;
  if (!nhits) return PRB_OK; // (decoys without a hit in the page: it is merged)
  t->broken = true; // (until the merge is whole)
  int rc;
  FeatHits h;
  DevBuf *const bufs[6] = {&t->h_query, &t->h_db_id, &t->h_e_tot, &t->h_e_acc, &t->h_e_hyb, &t->h_ends};
  if ((rc = upload_hit_list(ctx, cols, bufs, &h))) return rc;
  if ((rc = merge_fnull_hits(ctx, t, page, h, nullptr, 0))) return rc;
  t->broken = false;
  return PRB_OK;
}

int prb_fnullset_end(prb_ctx *ctx, prb_fnullset *t) {
  const char *fn = "prb_fnullset_end";
  if (int rc = fnull_guard(fn, ctx, t)) return rc;
  if (!t->open) return refuse(fn, "no decoy batch is open", PRB_ERR_STATE);
  for (size_t p = 0; p < t->page_merged.size(); p++)
    if (!t->page_merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged in the open decoy batch: every page comes first", PRB_ERR_STATE);
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  int rc;
  t->broken = true; // (until the close is whole)
  if (t->ncells > 0) {
    if ((rc = ctx->time_begin())) return rc;
    PRB_HIP(launch_fnull_close(t->view(), ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kFnull, 1))) return rc;
    if ((rc = refuse_if_bad(ctx, t, fn))) return rc;
  }
  t->broken = false;
  mark_decoys(t, 0, t->owner.data(), t->decoy.data(), (int32_t)t->owner.size());
  t->owner.clear();
  t->decoy.clear();
  t->ncells = 0;
  t->open = false;
  return PRB_OK;
}

// the kept records with their counters gathered on the device and copied once
int prb_fnullset_finish(prb_ctx *ctx, prb_fnullset *t) {
  const char *fn = kFinishFn;
  if (int rc = finish_guard(fn, "feature null", ctx, t)) return rc;
  if (t->finished) return PRB_OK; // (the records are on the host already)
  if (t->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (t->open) return refuse(fn, "a decoy batch is open (prb_fnullset_end comes first)", PRB_ERR_STATE);
  if (t->nmerged != t->decoys_all())
    return refuse(fn, std::to_string(t->nmerged) + " of " + std::to_string(t->decoys_all()) + " (query, decoy) pairs are closed: every decoy of every query comes first",
                  PRB_ERR_STATE);
  t->recs.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (t->nkept > 0) {
    int rc;
    try {
      t->recs.resize((size_t)t->nkept);
    } catch (const std::exception &e) {
      return refuse(fn, e.what(), PRB_ERR_NOMEM);
    }
    const size_t bytes = (size_t)t->nkept * sizeof(prb_fnull_pair);
    if ((rc = t->out.ensure(bytes))) return rc;
    if ((rc = ctx->time_begin())) return rc;
    PRB_HIP(launch_fnull_gather(t->view(), t->kept.p, t->out.p, ctx->stream));
    PRB_HIP(hipMemcpyAsync(t->recs.data(), t->out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kFnull, 1))) return rc; // (synchronises: the copy is over)
  }
  t->finished = true;
  t->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_fnullset_size(const prb_fnullset *t) { return t ? (int64_t)t->recs.size() : -1; }
const prb_fnull_pair *prb_fnullset_records(const prb_fnullset *t) { return t ? t->recs.data() : nullptr; }
void prb_fnullset_decoy_counts(const prb_fnullset *t, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = t ? t->counts[i] : 0;
}
void prb_fnullset_free(prb_fnullset *t) { delete t; }

} // extern "C"
