// C ABI, part 17: the feature ranking table of a run - the N best queries of every annotated feature, over as many
// batches as the caller likes (prb_featrank_*, `ris -t -A FILE -B N`): a ranked run table (capi_ranked.hpp), fed on the
// device from each batch's complete, unfinished feature table (capi_features.hip) or from a caller's records.  Every
// check of a call is made on the host before anything is enqueued: a refused call leaves the table as it was.
#include "capi_ranked.hpp"

using namespace prb;

static const RankedNouns kNouns{"feature ranking",
                                "feature",
                                "features",
                                "annotation",
                                "candidates",
                                "prb_featrank_finish",
                                "a candidate merged into this feature ranking table named a feature, a query or an identifier outside it",
                                ModeTimer::kFeatRank};

extern "C" {

int prb_featrank_create(prb_ctx *ctx, const prb_annot *an, int32_t n, prb_featrank **out) {
  const char *fn = "prb_featrank_create";
  std::unique_ptr<prb_featrank> t;
  std::string why = bad_n(n);
  if (why.empty() && an && an->n < 1) why = "the annotation has no feature";
  if (why.empty() && an && an->n > INT32_MAX) why = "the annotation has " + std::to_string(an->n) + " features";
  if (int rc = new_table(fn, ctx && an && an->ctx->device == ctx->device, out, t, why)) return rc;
  t->n = n;
  t->nfeat = (int32_t)an->n;
  t->annot = an;
  try {
    t->tbase = {0, (int64_t)t->nfeat};
    t->merged.resize(1);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  t->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  PRB_HIP(hipSetDevice(ctx->device));
  if (t->table.ensure(t->bytes()) != PRB_OK || t->badflag.ensure(16) != PRB_OK)
    return refuse(fn, "can't allocate the feature ranking table (" + std::to_string(t->bytes() >> 20) + " MB of HBM for " + std::to_string(t->nfeat) +
                          " features of " + std::to_string(n) + " slots)",
                  PRB_ERR_NOMEM);
  PRB_HIP(hipMemsetAsync(t->badflag.p, 0, 16, ctx->stream));
  if (int rc = t->clear()) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_featrank_add_featset(prb_ctx *ctx, prb_featrank *t, const prb_featset *fs, const int32_t *query_ids) {
  const char *fn = "prb_featrank_add_featset";
  if (!ctx || !t || !fs || !query_ids) return refuse(fn, "bad argument");
  if (int rc = ranked_guard(fn, kNouns, ctx, t)) return rc;
  if (fs->ctx != ctx) return refuse(fn, "the feature table was made with another context");
  if (fs->broken) return refuse(fn, "an earlier merge into the feature table failed", PRB_ERR_STATE);
  if (fs->bad) return refuse(fn, "a hit merged into the feature table named a query or a sequence outside it, or its span left its sequence", PRB_ERR_STATE);
  if (fs->finished) return refuse(fn, "the feature table is finished already (prb_featset_finish)", PRB_ERR_STATE);
  if (fs->annot != t->annot && !(fs->annot->n == t->annot->n && fs->annot->pages == t->annot->pages))
    return refuse(fn, "the feature table and the feature ranking table were made with different annotations");
  for (size_t p = 0; p < fs->merged.size(); p++)
    if (!fs->merged[p])
      return refuse(fn, "page " + std::to_string(p) + " is not merged into the feature table: every identifier is merged once, so half a batch is not ranked",
                    PRB_ERR_STATE);
  const int64_t R = fs->nrec;
  if (R < 0 || R > INT32_MAX || fs->nq < 1)
    return refuse(fn, "the feature table has " + std::to_string(R) + " records of " + std::to_string(fs->nq) + " queries (at most 2^31 - 1 can be ranked)");
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // (the last check: a call that passes has its identifiers marked as merged)
  if (int rc = run_table_guard(fn, kNouns.what, kNouns.finish_fn, t, ctx, t->db, 0, fs->distinct, fs->chain, query_ids, fs->nq)) return rc;
  if (R) {
    t->broken = true; // (until the merge is whole)
    int rc;
    if ((rc = upload_ids(ctx, t, query_ids, fs->nq))) return rc;
    const FeatTableFeed feed{fs->recs_of(fs->table.p), R, t->ids.as<int32_t>(), fs->nq, t->nfeat, t->badflag.as<uint32_t>()};
    if ((rc = ctx->time_begin())) return rc;
    if ((rc = feed_ranked(fn, kNouns, ctx, t, feed, R))) return rc;
    t->broken = false;
  }
  for (int i = 0; i < 3; i++) t->counts[i] += fs->counts[i];
  t->unassigned += fs->unassigned;
  if (fs->distinct >= 0) t->distinct = fs->distinct;
  if (fs->chain >= 0) t->chain = fs->chain;
  return PRB_OK;
}

int prb_featrank_add_records(prb_ctx *ctx, prb_featrank *t, const prb_featrank_pair *recs, int64_t n) {
  return add_ranked_records(
      "prb_featrank_add_records", kNouns, ctx, t, recs, n, [](const prb_featrank_pair &r) { return r.f.feature; },
      [](const prb_featrank_pair &r) { return r.f.s.query; });
}
int prb_featrank_merge(prb_ctx *ctx, prb_featrank *dst, prb_featrank *src) {
  return merge_ranked_tables("prb_featrank_merge", kNouns, ctx, dst, src, [](prb_featrank *d, const prb_featrank *s) { d->unassigned += s->unassigned; });
}
int prb_featrank_finish(prb_ctx *ctx, prb_featrank *t) { return finish_ranked(kNouns, ctx, t); }

int64_t prb_featrank_size(const prb_featrank *t) { return t ? (int64_t)t->recs.size() : -1; }
const prb_featrank_pair *prb_featrank_records(const prb_featrank *t) { return t ? t->recs.data() : nullptr; }
void prb_featrank_counts(const prb_featrank *t, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = t ? t->counts[i] : 0;
}
int64_t prb_featrank_unassigned(const prb_featrank *t) { return t ? t->unassigned : -1; }
void prb_featrank_free(prb_featrank *t) { delete t; }

} // extern "C"
