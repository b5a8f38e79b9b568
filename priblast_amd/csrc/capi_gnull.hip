// C ABI, part 12: the group null table of one batch - per kept (query, group) record of a finished group table, how the
// query's decoys fare against the same group (prb_gnullset_*, `ris -t -G FILE -P N`).  The kernels are in
// gnull_kernels.hip.  Every check of a call is made on the host before anything is enqueued: a refused call leaves the
// table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kFinishFn = "prb_gnullset_finish";
const char *const kBadRecord = "a record merged into this group null table named a query, a sequence, a page, a group, an owner or a decoy outside it";

// What every call on an unfinished table checks of it first
int gnull_guard(const std::string &fn, const prb_ctx *ctx, const prb_gnullset *gn) {
  if (!ctx || !gn) return refuse(fn, "bad argument");
  if (gn->ctx != ctx) return refuse(fn, "the group null table was made with another context");
  if (gn->broken) return refuse(fn, "an earlier merge into this group null table failed", PRB_ERR_STATE);
  if (gn->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (gn->finished) return refuse(fn, std::string("the group null table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  return PRB_OK;
}
// ... and a call that merges a page into the open batch
int page_guard(const std::string &fn, const prb_gnullset *gn, int32_t page) {
  if (!gn->open) return refuse(fn, "no decoy batch is open (prb_gnullset_begin comes first)", PRB_ERR_STATE);
  if (page < 0 || (size_t)page >= gn->page_merged.size())
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(gn->page_merged.size()) + ")");
  if (gn->page_merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged in the open decoy batch");
  return PRB_OK;
}

// the device's `bad` flag to the host: raised = the call is refused
int refuse_if_bad(prb_ctx *ctx, prb_gnullset *gn, const char *fn) {
  if (int rc = fetch_bad(ctx, gn)) return rc;
  if (gn->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  return PRB_OK;
}

} // namespace

// prb_search_page_gnull (per sub-batch) and prb_gnullset_add_pairs: the records folded into the scratch cells, in a
// bracket of the "gnull" timer
static int merge_gnull_pairs(prb_ctx *ctx, prb_gnullset *gn, int32_t page, const void *packed, int64_t npairs) {
  int rc;
  if (page < 0 || (size_t)page >= gn->map_dev.size() || !gn->open) return refuse("prb_search_page_gnull", "page out of range", PRB_ERR_STATE);
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_gnull_fold(packed, npairs, gn->view(), gn->page_view((size_t)page), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kGnull, 1))) return rc;
  return refuse_if_bad(ctx, gn, "prb_search_page_gnull");
}
int prb_gnullset::take(const SubBatch &b) { return merge_gnull_pairs(ctx, this, b.page, b.records, b.npairs); }

// prb_gnullset_create, from within the group table's finish: recs_dev[0, nrec) = the gathered records, still on the
// device.  The table takes the page maps over and builds the lookup, the keys and the counters.
int prb::keep_group_records(prb_ctx *ctx, prb_gnullset *gn, prb_groupset *gs, const void *recs_dev, int64_t nrec) {
  const char *fn = "prb_gnullset_create";
  gn->nkept = nrec;
  const size_t S = (size_t)gn->slots(), K = (size_t)std::max<int64_t>(nrec, 1);
  if (gn->lookup.ensure(S * 4) != PRB_OK || gn->table.ensure(K * sizeof(GNullCount)) != PRB_OK || gn->kept.ensure(K * sizeof(prb_group_pair)) != PRB_OK ||
      gn->badflag.ensure(16) != PRB_OK)
    return refuse(fn, "can't allocate the group null table (" + std::to_string((S * 4 + K * (sizeof(GNullCount) + sizeof(prb_group_pair))) >> 20) +
                          " MB of HBM for " + std::to_string(gn->nq) + " queries x " + std::to_string(gn->ngroups) + " groups)",
                  PRB_ERR_NOMEM);
  int rc;
  PRB_HIP(hipMemsetAsync(gn->badflag.p, 0, 16, ctx->stream));
  PRB_HIP(hipMemsetAsync(gn->lookup.p, 0xFF, S * 4, ctx->stream)); // (every (query, group): not kept)
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_gnull_keep(recs_dev, gn->view(), gn->kept.p, ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kGnull, nrec ? 1 : 0))) return rc;
  if ((rc = refuse_if_bad(ctx, gn, fn))) return rc;
  gn->map_dev = std::move(gs->map_dev);
  gs->map_dev.clear();
  return PRB_OK;
}

extern "C" {

int prb_gnullset_create(prb_ctx *ctx, prb_groupset *gs, int32_t n, int32_t ndecoys, prb_gnullset **out) {
  const char *fn = "prb_gnullset_create";
  std::unique_ptr<prb_gnullset> gn;
  if (int rc = new_table(fn, ctx && gs, out, gn,
                         ndecoys < 1 || ndecoys > 100000 ? "need 1 <= ndecoys <= 100000 (got " + std::to_string(ndecoys) + ")"
                         : n < 0 || n > kTopMaxN         ? "need 0 <= n <= " + std::to_string(kTopMaxN) + " (got " + std::to_string(n) + ")"
                                                         : ""))
    return rc;
  if (int rc = finish_guard(fn, "group", ctx, gs)) return rc;
  if (gs->bad) return refuse(fn, "a record merged into the group table named a query, a sequence, a page or a group outside it", PRB_ERR_STATE);
  if (gs->finished) return refuse(fn, "the group table is finished already (prb_groupset_finish)", PRB_ERR_STATE);
  for (size_t p = 0; p < gs->merged.size(); p++)
    if (!gs->merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged into the group table: the real batch against every page comes first", PRB_ERR_STATE);
  try {
    gn->map = gs->map;
    gn->page_merged.assign(gs->map.size(), 0);
    gn->merged.assign((size_t)(((int64_t)gs->nq * ndecoys + 63) / 64), 0);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  gn->nq = gs->nq;
  gn->ngroups = gs->ngroups;
  gn->ndecoys = ndecoys;
  gn->distinct = gs->distinct;
  gn->chain = gs->chain;
  gn->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  gn->db = gs->db;
  if (int rc = finish_groupset(fn, ctx, gs, n, gn.get())) return rc;
  *out = gn.release();
  return PRB_OK;
}

int prb_gnullset_begin(prb_ctx *ctx, prb_gnullset *gn, const int32_t *owner, const int32_t *decoy, int32_t ndq) {
  const char *fn = "prb_gnullset_begin";
  if (int rc = gnull_guard(fn, ctx, gn)) return rc;
  if (ndq < 1 || !owner || !decoy) return refuse(fn, "bad argument (a batch has one decoy at least)");
  if (gn->open) return refuse(fn, "a decoy batch is open (prb_gnullset_end comes first)", PRB_ERR_STATE);
  if (int rc = decoys_guard(fn, gn, 0, owner, decoy, ndq, " belongs to a batch closed before")) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // the scratch: every cell is empty between two batches (the close empties what it counts), so only new memory is filled
  const size_t bytes = (size_t)ndq * (size_t)gn->ngroups * 8;
  const size_t cap_before = gn->cell.cap;
  const bool have = gn->cell.ensure(bytes) == PRB_OK;
  if (have && gn->cell.cap != cap_before) PRB_HIP(hipMemsetAsync(gn->cell.p, 0xFF, gn->cell.cap, ctx->stream));
  if (!have || gn->own.ensure((size_t)ndq * 8) != PRB_OK)
    return refuse(fn, "can't allocate the scratch of the decoy batch (" + std::to_string(bytes >> 20) + " MB of HBM for " + std::to_string(ndq) +
                          " decoys x " + std::to_string(gn->ngroups) + " groups); open smaller batches",
                  PRB_ERR_NOMEM);
  if (int rc = upload_owners(ctx, gn, owner, decoy, ndq)) return rc; // (the room is there)
  try {
    gn->owner.assign(owner, owner + ndq);
    gn->decoy.assign(decoy, decoy + ndq);
  } catch (const std::exception &e) {
    gn->owner.clear();
    gn->decoy.clear();
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  std::fill(gn->page_merged.begin(), gn->page_merged.end(), 0);
  gn->open = true;
  return PRB_OK;
}

int prb_search_page_gnull(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_gnullset *gn) {
  const char *fn = "prb_search_page_gnull";
  if (!gn) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, dqb, db, page, opts, 3)) return rc;
  if (gn->db != db) return refuse(fn, "the group null table was made for another database");
  if (int rc = gnull_guard(fn, ctx, gn)) return rc;
  if (int rc = page_guard(fn, gn, page)) return rc;
  if ((size_t)dqb->nq != gn->owner.size())
    return refuse(fn, "the open decoy batch has " + std::to_string(gn->owner.size()) + " decoys; this query batch has " + std::to_string(dqb->nq));
  if (int rc = selection_guard(fn, "group null table", gn, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, dqb, db, opts)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  gn->page_merged[(size_t)page] = 1;
  gn->broken = true; // (until the merge is whole)
  if (int rc = search_into_table(gn, ctx, dqb, db, page, opts, gn->counts)) return rc;
  gn->broken = false;
  return PRB_OK;
}

int prb_gnullset_add_pairs(prb_ctx *ctx, prb_gnullset *gn, int32_t page, const prb_pair_summary *pairs, int64_t n) {
  const char *fn = "prb_gnullset_add_pairs";
  if (n < 0 || n > INT32_MAX || (n && !pairs)) return refuse(fn, "bad argument");
  if (int rc = gnull_guard(fn, ctx, gn)) return rc;
  if (int rc = page_guard(fn, gn, page)) return rc;
  if (int rc = records_guard(fn, (int64_t)gn->map[(size_t)page].size(), (int64_t)gn->owner.size(), pairs, n)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  gn->page_merged[(size_t)page] = 1;
  if (!n) return PRB_OK; // (decoys without a hit in the page: it is merged)
  gn->broken = true; // (until the merge is whole)
  if (int rc = upload_records(ctx, gn->h_rec, pairs, n)) return rc;
  if (int rc = merge_gnull_pairs(ctx, gn, page, gn->h_rec.p, n)) return rc;
  gn->broken = false;
  return PRB_OK;
}

int prb_gnullset_end(prb_ctx *ctx, prb_gnullset *gn) {
  const char *fn = "prb_gnullset_end";
  if (int rc = gnull_guard(fn, ctx, gn)) return rc;
  if (!gn->open) return refuse(fn, "no decoy batch is open", PRB_ERR_STATE);
  for (size_t p = 0; p < gn->page_merged.size(); p++)
    if (!gn->page_merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged in the open decoy batch: every page comes first", PRB_ERR_STATE);
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  int rc;
  gn->broken = true; // (until the close is whole)
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_gnull_close(gn->view(), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kGnull, 1))) return rc;
  if ((rc = refuse_if_bad(ctx, gn, fn))) return rc;
  gn->broken = false;
  mark_decoys(gn, 0, gn->owner.data(), gn->decoy.data(), (int32_t)gn->owner.size());
  gn->owner.clear();
  gn->decoy.clear();
  gn->open = false;
  return PRB_OK;
}

// the kept records with their counters gathered on the device and copied once
int prb_gnullset_finish(prb_ctx *ctx, prb_gnullset *gn) {
  const char *fn = kFinishFn;
  if (int rc = finish_guard(fn, "group null", ctx, gn)) return rc;
  if (gn->finished) return PRB_OK; // (the records are on the host already)
  if (gn->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (gn->open) return refuse(fn, "a decoy batch is open (prb_gnullset_end comes first)", PRB_ERR_STATE);
  if (gn->nmerged != gn->decoys_all())
    return refuse(fn, std::to_string(gn->nmerged) + " of " + std::to_string(gn->decoys_all()) + " (query, decoy) pairs are closed: every decoy of every query comes first",
                  PRB_ERR_STATE);
  gn->pairs.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (gn->nkept > 0) {
    int rc;
    try {
      gn->pairs.resize((size_t)gn->nkept);
    } catch (const std::exception &e) {
      return refuse(fn, e.what(), PRB_ERR_NOMEM);
    }
    const size_t bytes = (size_t)gn->nkept * sizeof(prb_gnull_pair);
    if ((rc = gn->out.ensure(bytes))) return rc;
    if ((rc = ctx->time_begin())) return rc;
    PRB_HIP(launch_gnull_gather(gn->view(), gn->kept.p, gn->out.p, ctx->stream));
    PRB_HIP(hipMemcpyAsync(gn->pairs.data(), gn->out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kGnull, 1))) return rc; // (synchronises: the copy is over)
  }
  gn->finished = true;
  gn->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_gnullset_size(const prb_gnullset *gn) { return gn ? (int64_t)gn->pairs.size() : -1; }
const prb_gnull_pair *prb_gnullset_pairs(const prb_gnullset *gn) { return gn ? gn->pairs.data() : nullptr; }
void prb_gnullset_decoy_counts(const prb_gnullset *gn, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = gn ? gn->counts[i] : 0;
}
void prb_gnullset_free(prb_gnullset *gn) { delete gn; }

} // extern "C"
