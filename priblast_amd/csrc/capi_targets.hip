// C ABI, part 5: the per-target table of a run - the N best queries of every target (page, db_id) of one database,
// over as many batches as the caller likes (prb_targetset_*).
#include "capi_tables.hpp"

using namespace prb;

// every key, payload slot and fill count of the table back to "nothing", on its own device and stream
static int clear_target_table(prb_targetset &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, t.bytes(), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  return PRB_OK;
}

// prb_search_page_targets, per sub-batch: the pairs' records - their `query` turned into the caller's identifier -
// grouped by target (a stable sort by db_id: a target's records stay in query order; always, whatever the sub-batch
// holds) and every target's run merged into the per-target table by a wavefront, in a bracket of the "targets" timer
static int merge_targets(prb_ctx *ctx, SearchWs &w, prb_targetset *ts, int32_t page, int32_t nseq, int32_t nq, void *packed, int64_t npairs) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  const size_t NP = (size_t)npairs;
  if ((rc = ts->key.ensure(NP * 4)) || (rc = ts->keyS.ensure(NP * 4)) || (rc = ts->val.ensure(NP * 4)) || (rc = ts->valS.ensure(NP * 4)) ||
      (rc = ts->rkey.ensure(NP * sizeof(TargetKey))) || (rc = ts->head.ensure(NP)) || (rc = ts->start.ensure(NP * 4)))
    return rc;
  PRB_HIP(launch_target_ids(packed, npairs, ts->ids.as<int32_t>(), nq, ts->key.as<uint32_t>(), ts->val.as<uint32_t>(), ctx->stream));
  if ((rc = sort_target_keys(ctx->stream, ts->sortTmp, ts->key.as<uint32_t>(), ts->keyS.as<uint32_t>(), ts->val.as<uint32_t>(), ts->valS.as<uint32_t>(),
                             NP, (unsigned)bits_for(std::max(nseq - 1, 1)))))
    return rc;
  PRB_HIP(launch_target_runs(packed, npairs, ts->keyS.as<uint32_t>(), ts->valS.as<uint32_t>(), ts->rkey.as<TargetKey>(), ts->head.as<uint8_t>(),
                             ctx->stream));
  int64_t nruns = 0;
  if ((rc = select_flagged(ctx, w, nullptr, ts->head.as<uint8_t>(), ts->start.as<uint32_t>(), NP, &nruns))) return rc;
  if (nruns <= 0 || nruns > npairs || nruns > nseq) {
    set_error("per-target table: " + std::to_string(nruns) + " targets for " + std::to_string(npairs) + " pairs");
    return PRB_ERR_STATE;
  }
  PRB_HIP(launch_target_merge(packed, ts->rkey.as<TargetKey>(), ts->keyS.as<uint32_t>(), ts->start.as<uint32_t>(), nruns, npairs, page,
                              ts->tbase[(size_t)page], nseq, ts->n, ts->keys_of(ts->table.p), ts->slots_of(ts->table.p), ts->fill_of(ts->table.p),
                              ctx->stream));
  return ctx->time_end(ModeTimer::kTargets, 5);
}
int prb_targetset::take(const SubBatch &b) { return merge_targets(ctx, ws_of(ctx), this, b.page, b.nseq, b.nq, b.records, b.npairs); }

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
  if (int rc = clear_target_table(*t)) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_search_page_targets(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *query_ids,
                            prb_targetset *ts) {
  return merge_run_page("prb_search_page_targets", "per-target", "prb_targetset_finish", ts, ctx, qb, db, page, opts,
                        query_ids);
}

int prb_targetset_merge(prb_ctx *ctx, prb_targetset *dst, prb_targetset *src) {
  if (int rc = run_tables_guard("prb_targetset_merge", "per-target", ctx, dst, src, [&]() -> std::string {
        if (dst->n == src->n) return "";
        return "the per-target tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per target";
      }))
    return rc;
  return join_tables(
      "prb_targetset_merge", ModeTimer::kTargets, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_target_join(dst->keys_of(dst->table.p), dst->slots_of(dst->table.p), dst->fill_of(dst->table.p), dst->keys_of(block),
                                   dst->slots_of(block), dst->fill_of(block), dst->targets(), dst->n, ctx->stream));
        return PRB_OK;
      },
      clear_target_table);
}

// the fills scanned, the filled slots gathered by target and rank on the device, one copy
int prb_targetset_finish(prb_ctx *ctx, prb_targetset *ts) {
  if (int rc = finish_guard("prb_targetset_finish", "per-target", ctx, ts)) return rc;
  if (ts->finished) return PRB_OK; // (the records are on the host already)
  PRB_HIP(hipSetDevice(ctx->device));
  if (int rc = finish_ranked("prb_targetset_finish", ctx, ts->fill_of(ts->table.p), ts->targets(), ts->entries(), ts->pairs,
                             [&](const int64_t *off, int64_t total, void *out) {
                               return launch_target_gather(ts->keys_of(ts->table.p), ts->slots_of(ts->table.p), off, ts->targets(), ts->n, total, out,
                                                           ctx->stream);
                             }))
    return rc;
  ts->finished = true;
  ts->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_targetset_size(const prb_targetset *ts) { return ts ? (int64_t)ts->pairs.size() : -1; }
const prb_target_pair *prb_targetset_pairs(const prb_targetset *ts) { return ts ? ts->pairs.data() : nullptr; }
void prb_targetset_counts(const prb_targetset *ts, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ts ? ts->counts[i] : 0;
}
void prb_targetset_free(prb_targetset *ts) {
  delete ts;
}

} // extern "C"
