// C ABI, part 5: the per-target table of a run - the N best queries of every target (page, db_id) of one database,
// over as many batches as the caller likes (prb_targetset_*): a ranked run table (capi_ranked.hpp) fed by the searches
// themselves.
#include "capi_ranked.hpp"

using namespace prb;

static const RankedNouns kNouns{"per-target", "target", "targets", "table", "pairs", "prb_targetset_finish", "", ModeTimer::kTargets};

// prb_search_page_targets, per sub-batch: the pairs' records - their `query` turned into the caller's identifier -
// grouped by target (a stable sort by db_id: a target's records stay in query order; always, whatever the sub-batch
// holds) and every target's run merged into the per-target table by a wavefront, in a bracket of the "targets" timer
int prb_targetset::take(const SubBatch &b) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  const PairFeed feed{b.records, b.npairs, ids.as<int32_t>(), b.nq, b.page, b.nseq, tbase[(size_t)b.page]};
  if ((rc = merge_ranked_candidates(ctx, this, kNouns, feed, b.nseq, b.npairs))) return rc;
  return ctx->time_end(ModeTimer::kTargets, 5);
}

extern "C" {

int prb_targetset_create(prb_ctx *ctx, prb_db *db, int32_t n, prb_targetset **out) {
  std::unique_ptr<prb_targetset> t;
  if (int rc = new_table("prb_targetset_create", ctx && db && db->ctx->device == ctx->device, out, t, bad_n(n))) return rc;
  t->ctx = ctx;
  t->db = db;
  t->n = n;
  t->tbase.assign(db->pages.size() + 1, 0);
  for (size_t p = 0; p < db->pages.size(); p++) t->tbase[p + 1] = t->tbase[p] + db->pages[p].nseq;
  t->merged.resize(db->pages.size());
  PRB_HIP(hipSetDevice(ctx->device));
  if (t->table.ensure(t->bytes()) != PRB_OK)
    return refuse("prb_targetset_create", "can't allocate the per-target table (" + std::to_string(t->bytes() >> 20) + " MB of HBM for " +
                                              std::to_string(t->targets()) + " targets of " + std::to_string(n) + " slots)",
                  PRB_ERR_NOMEM);
  if (int rc = t->clear()) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_search_page_targets(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *query_ids,
                            prb_targetset *ts) {
  return merge_run_page("prb_search_page_targets", kNouns.what, kNouns.finish_fn, ts, ctx, qb, db, page, opts, query_ids);
}

int prb_targetset_merge(prb_ctx *ctx, prb_targetset *dst, prb_targetset *src) {
  return merge_ranked_tables("prb_targetset_merge", kNouns, ctx, dst, src, nothing_to_carry);
}
int prb_targetset_finish(prb_ctx *ctx, prb_targetset *ts) { return finish_ranked(kNouns, ctx, ts); }

int64_t prb_targetset_size(const prb_targetset *ts) { return ts ? (int64_t)ts->recs.size() : -1; }
const prb_target_pair *prb_targetset_pairs(const prb_targetset *ts) { return ts ? ts->recs.data() : nullptr; }
void prb_targetset_counts(const prb_targetset *ts, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ts ? ts->counts[i] : 0;
}
void prb_targetset_free(prb_targetset *ts) {
  delete ts;
}

} // extern "C"
