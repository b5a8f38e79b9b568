// C ABI, part 17: the feature ranking table of a run - the N best queries of every annotated feature, over as many
// batches as the caller likes (prb_featrank_*, `ris -t -A FILE -B N`).  It is fed on the device from each batch's complete,
// unfinished feature table (capi_features.hip) or from a caller's records; the kernels are in featrank_kernels.hip, the
// ranked lists themselves the per-target table's (rank_kernels.hpp).  Every check of a call is made on the host before
// anything is enqueued: a refused call leaves the table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kWhat = "feature ranking";
const char *const kFinishFn = "prb_featrank_finish";
const char *const kBadCandidate = "a candidate merged into this feature ranking table named a feature, a query or an identifier outside it";

// every key, payload slot and fill count of the table back to "nothing", on its own device and stream
int clear_featrank(prb_featrank &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, t.bytes(), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  t.unassigned = 0;
  return PRB_OK;
}

// what both merges check of the table first
int table_guard(const char *fn, const prb_ctx *ctx, const prb_featrank *t) {
  if (t->ctx != ctx) return refuse(fn, "the feature ranking table was made with another context");
  if (t->broken) return refuse(fn, "an earlier merge into this feature ranking table failed", PRB_ERR_STATE);
  if (t->bad) return refuse(fn, kBadCandidate, PRB_ERR_STATE);
  if (t->finished) return refuse(fn, std::string("the feature ranking table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  return PRB_OK;
}

// behind a merge: the device's flag
int bad_guard(const char *fn, prb_ctx *ctx, prb_featrank *t) {
  if (int rc = fetch_bad(ctx, t)) return rc;
  return t->bad ? refuse(fn, kBadCandidate, PRB_ERR_STATE) : PRB_OK;
}

} // namespace

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
  if (int rc = clear_featrank(*t)) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_featrank_add_featset(prb_ctx *ctx, prb_featrank *t, const prb_featset *fs, const int32_t *query_ids) {
  const char *fn = "prb_featrank_add_featset";
  if (!ctx || !t || !fs || !query_ids) return refuse(fn, "bad argument");
  if (int rc = table_guard(fn, ctx, t)) return rc;
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
  if (int rc = run_table_guard(fn, kWhat, kFinishFn, t, ctx, t->db, 0, fs->distinct, fs->chain, query_ids, fs->nq)) return rc;
  if (R) {
    t->broken = true; // (until the merge is whole)
    int rc;
    SearchWs &w = ws_of(ctx);
    if ((rc = upload_ids(ctx, t, query_ids, fs->nq))) return rc;
    if ((rc = w.count.ensure(16))) return rc;
    const FeatRankFeed feed{fs->recs_of(fs->table.p), R, t->ids.as<int32_t>(), fs->nq, t->nfeat};
    uint32_t *bad = t->badflag.as<uint32_t>();
    if ((rc = ctx->time_begin())) return rc;
    if ((rc = merge_ranked_candidates(
             ctx, w, t, kWhat, "features", t->nfeat, R,
             [&](uint32_t *key, uint32_t *val) { return launch_featrank_table_features(feed, key, val, bad, ctx->stream); },
             [&](const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head) {
               return launch_featrank_table_runs(feed, key, val, rkey, head, bad, ctx->stream);
             },
             [&](const GroupRankRuns &r) {
               return launch_featrank_table_merge(feed, r, t->n, t->keys_of(t->table.p), t->slots_of(t->table.p), t->fill_of(t->table.p), ctx->stream);
             })))
      return rc;
    if ((rc = ctx->time_end(ModeTimer::kFeatRank, 5))) return rc;
    if ((rc = bad_guard(fn, ctx, t))) return rc;
    t->broken = false;
  }
  for (int i = 0; i < 3; i++) t->counts[i] += fs->counts[i];
  t->unassigned += fs->unassigned;
  if (fs->distinct >= 0) t->distinct = fs->distinct;
  if (fs->chain >= 0) t->chain = fs->chain;
  return PRB_OK;
}

int prb_featrank_add_records(prb_ctx *ctx, prb_featrank *t, const prb_featrank_pair *recs, int64_t n) {
  const char *fn = "prb_featrank_add_records";
  if (!ctx || !t || n < 0 || n > INT32_MAX || (n && !recs)) return refuse(fn, "bad argument");
  if (int rc = table_guard(fn, ctx, t)) return rc;
  std::vector<int32_t> ids;
  try {
    std::vector<int64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const prb_feature_pair &r = recs[i].f;
      if (r.feature < 0 || r.feature >= t->nfeat)
        return refuse(fn, "record " + std::to_string(i) + " names feature " + std::to_string(r.feature) + " (the annotation has " +
                              std::to_string(t->nfeat) + ")");
      if (r.s.query < 0) return refuse(fn, "query identifier " + std::to_string(r.s.query) + " is below 0");
      keys[(size_t)i] = (int64_t)r.s.query * t->nfeat + r.feature;
    }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size(); i++) {
      if (i && keys[i] == keys[i - 1])
        return refuse(fn, "query identifier " + std::to_string(keys[i] / t->nfeat) + " is given twice for feature " + std::to_string(keys[i] % t->nfeat));
      const int32_t id = (int32_t)(keys[i] / t->nfeat);
      if (ids.empty() || ids.back() != id) ids.push_back(id);
    }
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // (the last check: a call that passes has its identifiers marked as merged)
  if (int rc = run_table_guard(fn, kWhat, kFinishFn, t, ctx, t->db, 0, -1, -1, ids.data(), (int32_t)ids.size())) return rc;
  if (!n) return PRB_OK;
  t->broken = true; // (until the merge is whole)
  int rc;
  SearchWs &w = ws_of(ctx);
  const size_t bytes = (size_t)n * sizeof(prb_featrank_pair);
  if ((rc = w.count.ensure(16)) || (rc = t->h_rec.ensure(bytes))) return rc;
  PRB_HIP(hipMemcpyAsync(t->h_rec.p, recs, bytes, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  uint32_t *bad = t->badflag.as<uint32_t>();
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = merge_ranked_candidates(
           ctx, w, t, kWhat, "features", t->nfeat, n,
           [&](uint32_t *key, uint32_t *val) { return launch_featrank_record_features(t->h_rec.p, n, t->nfeat, key, val, bad, ctx->stream); },
           [&](const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head) {
             return launch_featrank_record_runs(t->h_rec.p, n, t->nfeat, key, val, rkey, head, bad, ctx->stream);
           },
           [&](const GroupRankRuns &r) {
             return launch_featrank_record_merge(t->h_rec.p, n, r, t->nfeat, t->n, t->keys_of(t->table.p), t->slots_of(t->table.p),
                                                 t->fill_of(t->table.p), ctx->stream);
           })))
    return rc;
  if ((rc = ctx->time_end(ModeTimer::kFeatRank, 5))) return rc;
  if ((rc = bad_guard(fn, ctx, t))) return rc;
  t->broken = false;
  return PRB_OK;
}

int prb_featrank_merge(prb_ctx *ctx, prb_featrank *dst, prb_featrank *src) {
  const char *fn = "prb_featrank_merge";
  if (int rc = run_tables_guard(fn, kWhat, ctx, dst, src, [&]() -> std::string {
        if (dst->nfeat != src->nfeat)
          return "the feature ranking tables have " + std::to_string(dst->nfeat) + " and " + std::to_string(src->nfeat) + " features";
        if (dst->n != src->n)
          return "the feature ranking tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per feature";
        return "";
      }))
    return rc;
  if (dst->bad || src->bad) return refuse(fn, kBadCandidate, PRB_ERR_STATE);
  const int64_t src_unassigned = src->unassigned;
  return join_tables(
      fn, ModeTimer::kFeatRank, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_featrank_join(dst->keys_of(dst->table.p), dst->slots_of(dst->table.p), dst->fill_of(dst->table.p), dst->keys_of(block),
                                     dst->slots_of(block), dst->fill_of(block), dst->nfeat, dst->n, ctx->stream));
        dst->unassigned += src_unassigned;
        return PRB_OK;
      },
      clear_featrank);
}

// the fills scanned, the filled slots gathered by feature and rank on the device, one copy
int prb_featrank_finish(prb_ctx *ctx, prb_featrank *t) {
  if (int rc = finish_guard(kFinishFn, kWhat, ctx, t)) return rc;
  if (t->finished) return PRB_OK; // (the records are on the host already)
  if (t->bad) return refuse(kFinishFn, kBadCandidate, PRB_ERR_STATE);
  PRB_HIP(hipSetDevice(ctx->device));
  if (int rc = finish_ranked(kFinishFn, ctx, t->fill_of(t->table.p), t->nfeat, t->entries(), t->recs,
                             [&](const int64_t *off, int64_t total, void *out) {
                               return launch_featrank_gather(t->keys_of(t->table.p), t->slots_of(t->table.p), off, t->nfeat, t->n, total, out,
                                                             ctx->stream);
                             }))
    return rc;
  t->finished = true;
  t->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_featrank_size(const prb_featrank *t) { return t ? (int64_t)t->recs.size() : -1; }
const prb_featrank_pair *prb_featrank_records(const prb_featrank *t) { return t ? t->recs.data() : nullptr; }
void prb_featrank_counts(const prb_featrank *t, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = t ? t->counts[i] : 0;
}
int64_t prb_featrank_unassigned(const prb_featrank *t) { return t ? t->unassigned : -1; }
void prb_featrank_free(prb_featrank *t) { delete t; }

} // extern "C"
