// C ABI, part 12: the group ranking table of a run - the N best queries of every group of database sequences, over as
// many batches as the caller likes (prb_grouprank_*, `ris -t -G FILE -R N`): a ranked run table (capi_ranked.hpp), fed on
// the device from each batch's complete group table (capi_groups.hip) or from a caller's records.  Every check of a call
// is made on the host before anything is enqueued: a refused call leaves the table as it was.
#include "capi_ranked.hpp"

using namespace prb;

static const RankedNouns kNouns{"group ranking",
                                "group",
                                "groups",
                                "table",
                                "candidates",
                                "prb_grouprank_finish",
                                "a candidate merged into this group ranking table named a slot, a group, a query or an identifier outside it",
                                ModeTimer::kGroupRank};

extern "C" {

int prb_grouprank_create(prb_ctx *ctx, int32_t ngroups, int32_t n, prb_grouprank **out) {
  const char *fn = "prb_grouprank_create";
  std::unique_ptr<prb_grouprank> t;
  std::string why = bad_n(n);
  if (why.empty() && ngroups < 1) why = "need ngroups >= 1 (got " + std::to_string(ngroups) + ")";
  if (int rc = new_table(fn, ctx != nullptr, out, t, why)) return rc;
  t->n = n;
  t->ngroups = ngroups;
  try {
    t->tbase = {0, (int64_t)ngroups};
    t->merged.resize(1);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  t->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  PRB_HIP(hipSetDevice(ctx->device));
  if (t->table.ensure(t->bytes()) != PRB_OK || t->badflag.ensure(16) != PRB_OK)
    return refuse(fn, "can't allocate the group ranking table (" + std::to_string(t->bytes() >> 20) + " MB of HBM for " + std::to_string(ngroups) +
                          " groups of " + std::to_string(n) + " slots)",
                  PRB_ERR_NOMEM);
  PRB_HIP(hipMemsetAsync(t->badflag.p, 0, 16, ctx->stream));
  if (int rc = t->clear()) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_grouprank_add_groupset(prb_ctx *ctx, prb_grouprank *t, const prb_groupset *gs, const int32_t *query_ids) {
  const char *fn = "prb_grouprank_add_groupset";
  if (!ctx || !t || !gs || !query_ids) return refuse(fn, "bad argument");
  if (int rc = ranked_guard(fn, kNouns, ctx, t)) return rc;
  if (gs->ctx != ctx) return refuse(fn, "the group table was made with another context");
  if (gs->broken) return refuse(fn, "an earlier merge into the group table failed", PRB_ERR_STATE);
  if (gs->bad) return refuse(fn, "a record merged into the group table named a query, a sequence, a page or a group outside it", PRB_ERR_STATE);
  if (gs->finished) return refuse(fn, "the group table is finished already (prb_groupset_finish)", PRB_ERR_STATE);
  if (gs->ngroups != t->ngroups)
    return refuse(fn, "the group table has " + std::to_string(gs->ngroups) + " groups, the group ranking table " + std::to_string(t->ngroups));
  for (size_t p = 0; p < gs->merged.size(); p++)
    if (!gs->merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged into the group table: a group's minimum over some of its members is not ranked",
                    PRB_ERR_STATE);
  const int64_t S = gs->slots();
  if (S <= 0 || S > (int64_t)UINT32_MAX) return refuse(fn, "the group table has " + std::to_string(S) + " slots");
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // (the last check: a call that passes has its identifiers marked as merged)
  if (int rc = run_table_guard(fn, kNouns.what, kNouns.finish_fn, t, ctx, t->db, 0, gs->distinct, gs->chain, query_ids, gs->nq)) return rc;
  t->broken = true; // (until the merge is whole)
  int rc;
  SearchWs &w = ws_of(ctx);
  if ((rc = upload_ids(ctx, t, query_ids, gs->nq))) return rc;
  if ((rc = w.count.ensure(16)) || (rc = t->occ.ensure((size_t)S)) || (rc = t->sel.ensure((size_t)S * 4))) return rc;
  const GroupTab tab = gs->view();
  if ((rc = ctx->time_begin())) return rc;
  // one linear pass over the dense slots - the flags and their compaction -, then work on the occupied ones only
  int64_t ncand = 0;
  PRB_HIP(launch_group_flags(tab, t->occ.as<uint8_t>(), ctx->stream));
  if ((rc = select_flagged(ctx, w, nullptr, t->occ.as<uint8_t>(), t->sel.as<uint32_t>(), (size_t)S, &ncand))) return rc;
  if (ncand < 0 || ncand > S || ncand > INT32_MAX) return refuse(fn, "bad candidate count " + std::to_string(ncand), PRB_ERR_STATE);
  const GroupSlotFeed feed{tab, t->sel.as<uint32_t>(), ncand, t->ids.as<int32_t>(), t->badflag.as<uint32_t>()};
  if ((rc = feed_ranked(fn, kNouns, ctx, t, feed, ncand, 2))) return rc;
  for (int i = 0; i < 3; i++) t->counts[i] += gs->counts[i];
  if (gs->distinct >= 0) t->distinct = gs->distinct;
  if (gs->chain >= 0) t->chain = gs->chain;
  t->broken = false;
  return PRB_OK;
}

int prb_grouprank_add_records(prb_ctx *ctx, prb_grouprank *t, const prb_group_pair *recs, int64_t n) {
  return add_ranked_records(
      "prb_grouprank_add_records", kNouns, ctx, t, recs, n, [](const prb_group_pair &r) { return r.group; },
      [](const prb_group_pair &r) { return r.s.query; });
}
int prb_grouprank_merge(prb_ctx *ctx, prb_grouprank *dst, prb_grouprank *src) {
  return merge_ranked_tables("prb_grouprank_merge", kNouns, ctx, dst, src, nothing_to_carry);
}
int prb_grouprank_finish(prb_ctx *ctx, prb_grouprank *t) { return finish_ranked(kNouns, ctx, t); }

int64_t prb_grouprank_size(const prb_grouprank *t) { return t ? (int64_t)t->recs.size() : -1; }
const prb_group_pair *prb_grouprank_pairs(const prb_grouprank *t) { return t ? t->recs.data() : nullptr; }
void prb_grouprank_counts(const prb_grouprank *t, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = t ? t->counts[i] : 0;
}
void prb_grouprank_free(prb_grouprank *t) { delete t; }

} // extern "C"
