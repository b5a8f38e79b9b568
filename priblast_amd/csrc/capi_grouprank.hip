// C ABI, part 12: the group ranking table of a run - the N best queries of every group of database sequences, over as
// many batches as the caller likes (prb_grouprank_*, `ris -t -G FILE -R N`).  It is fed on the device from each batch's
// complete group table (capi_groups.hip) or from a caller's records; the kernels are in grouprank_kernels.hip, the
// ranked lists themselves the per-target table's (rank_kernels.hpp).  Every check of a call is made on the host before
// anything is enqueued: a refused call leaves the table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kWhat = "group ranking";
const char *const kFinishFn = "prb_grouprank_finish";
const char *const kBadCandidate = "a candidate merged into this group ranking table named a slot, a group, a query or an identifier outside it";

// every key, payload slot and fill count of the table back to "nothing", on its own device and stream
int clear_grouprank(prb_grouprank &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, t.bytes(), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  return PRB_OK;
}

// what both merges check of the table first
int table_guard(const char *fn, const prb_ctx *ctx, const prb_grouprank *t) {
  if (t->ctx != ctx) return refuse(fn, "the group ranking table was made with another context");
  if (t->broken) return refuse(fn, "an earlier merge into this group ranking table failed", PRB_ERR_STATE);
  if (t->bad) return refuse(fn, kBadCandidate, PRB_ERR_STATE);
  if (t->finished) return refuse(fn, std::string("the group ranking table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  return PRB_OK;
}

// behind a merge: the device's flag
int bad_guard(const char *fn, prb_ctx *ctx, prb_grouprank *t) {
  if (int rc = fetch_bad(ctx, t)) return rc;
  return t->bad ? refuse(fn, kBadCandidate, PRB_ERR_STATE) : PRB_OK;
}

} // namespace

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
  if (int rc = clear_grouprank(*t)) return rc;
  *out = t.release();
  return PRB_OK;
}

int prb_grouprank_add_groupset(prb_ctx *ctx, prb_grouprank *t, const prb_groupset *gs, const int32_t *query_ids) {
  const char *fn = "prb_grouprank_add_groupset";
  if (!ctx || !t || !gs || !query_ids) return refuse(fn, "bad argument");
  if (int rc = table_guard(fn, ctx, t)) return rc;
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
  if (int rc = run_table_guard(fn, kWhat, kFinishFn, t, ctx, t->db, 0, gs->distinct, gs->chain, query_ids, gs->nq)) return rc;
  t->broken = true; // (until the merge is whole)
  int rc;
  SearchWs &w = ws_of(ctx);
  if ((rc = upload_ids(ctx, t, query_ids, gs->nq))) return rc;
  if ((rc = w.count.ensure(16)) || (rc = t->occ.ensure((size_t)S)) || (rc = t->sel.ensure((size_t)S * 4))) return rc;
  const GroupTab tab = gs->view();
  const int32_t *ids = t->ids.as<int32_t>();
  uint32_t *bad = t->badflag.as<uint32_t>();
  if ((rc = ctx->time_begin())) return rc;
  // one linear pass over the dense slots - the flags and their compaction -, then work on the occupied ones only
  int64_t launches = 2, ncand = 0;
  PRB_HIP(launch_group_flags(tab, t->occ.as<uint8_t>(), ctx->stream));
  if ((rc = select_flagged(ctx, w, nullptr, t->occ.as<uint8_t>(), t->sel.as<uint32_t>(), (size_t)S, &ncand))) return rc;
  if (ncand < 0 || ncand > S || ncand > INT32_MAX) return refuse(fn, "bad candidate count " + std::to_string(ncand), PRB_ERR_STATE);
  if (ncand) {
    if ((rc = merge_ranked_candidates(
             ctx, w, t, kWhat, "groups", t->ngroups, ncand,
             [&](uint32_t *key, uint32_t *val) { return launch_grouprank_slot_groups(tab, t->sel.as<uint32_t>(), ncand, key, val, bad, ctx->stream); },
             [&](const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head) {
               return launch_grouprank_slot_runs(tab, ids, ncand, key, val, rkey, head, bad, ctx->stream);
             },
             [&](const GroupRankRuns &r) {
               return launch_grouprank_slot_merge(tab, ids, r, t->n, t->keys_of(t->table.p), t->slots_of(t->table.p), t->fill_of(t->table.p),
                                                  ctx->stream);
             })))
      return rc;
    launches += 5;
  }
  if ((rc = ctx->time_end(ModeTimer::kGroupRank, launches))) return rc;
  if ((rc = bad_guard(fn, ctx, t))) return rc;
  for (int i = 0; i < 3; i++) t->counts[i] += gs->counts[i];
  if (gs->distinct >= 0) t->distinct = gs->distinct;
  if (gs->chain >= 0) t->chain = gs->chain;
  t->broken = false;
  return PRB_OK;
}

int prb_grouprank_add_records(prb_ctx *ctx, prb_grouprank *t, const prb_group_pair *recs, int64_t n) {
  const char *fn = "prb_grouprank_add_records";
  if (!ctx || !t || n < 0 || n > INT32_MAX || (n && !recs)) return refuse(fn, "bad argument");
  if (int rc = table_guard(fn, ctx, t)) return rc;
  std::vector<int32_t> ids;
  try {
    std::vector<int64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const prb_group_pair &r = recs[i];
      if (r.group < 0 || r.group >= t->ngroups)
        return refuse(fn, "record " + std::to_string(i) + " names group " + std::to_string(r.group) + " (the table has " + std::to_string(t->ngroups) + ")");
      if (r.s.query < 0) return refuse(fn, "query identifier " + std::to_string(r.s.query) + " is below 0");
      keys[(size_t)i] = (int64_t)r.s.query * t->ngroups + r.group;
    }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size(); i++) {
      if (i && keys[i] == keys[i - 1])
        return refuse(fn, "query identifier " + std::to_string(keys[i] / t->ngroups) + " is given twice for group " + std::to_string(keys[i] % t->ngroups));
      const int32_t id = (int32_t)(keys[i] / t->ngroups);
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
  const size_t bytes = (size_t)n * sizeof(prb_group_pair);
  if ((rc = w.count.ensure(16)) || (rc = t->h_rec.ensure(bytes))) return rc;
  PRB_HIP(hipMemcpyAsync(t->h_rec.p, recs, bytes, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  uint32_t *bad = t->badflag.as<uint32_t>();
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = merge_ranked_candidates(
           ctx, w, t, kWhat, "groups", t->ngroups, n, [&](uint32_t *key, uint32_t *val) { return launch_grouprank_record_groups(t->h_rec.p, n, t->ngroups, key, val, bad, ctx->stream); },
           [&](const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head) {
             return launch_grouprank_record_runs(t->h_rec.p, n, t->ngroups, key, val, rkey, head, bad, ctx->stream);
           },
           [&](const GroupRankRuns &r) {
             return launch_grouprank_record_merge(t->h_rec.p, n, r, t->ngroups, t->n, t->keys_of(t->table.p), t->slots_of(t->table.p),
                                                  t->fill_of(t->table.p), ctx->stream);
           })))
    return rc;
  if ((rc = ctx->time_end(ModeTimer::kGroupRank, 5))) return rc;
  if ((rc = bad_guard(fn, ctx, t))) return rc;
  t->broken = false;
  return PRB_OK;
}

int prb_grouprank_merge(prb_ctx *ctx, prb_grouprank *dst, prb_grouprank *src) {
  const char *fn = "prb_grouprank_merge";
  if (int rc = run_tables_guard(fn, kWhat, ctx, dst, src, [&]() -> std::string {
        if (dst->ngroups != src->ngroups)
          return "the group ranking tables have " + std::to_string(dst->ngroups) + " and " + std::to_string(src->ngroups) + " groups";
        if (dst->n != src->n) return "the group ranking tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per group";
        return "";
      }))
    return rc;
  if (dst->bad || src->bad) return refuse(fn, kBadCandidate, PRB_ERR_STATE);
  return join_tables(
      fn, ModeTimer::kGroupRank, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_grouprank_join(dst->keys_of(dst->table.p), dst->slots_of(dst->table.p), dst->fill_of(dst->table.p), dst->keys_of(block),
                                      dst->slots_of(block), dst->fill_of(block), dst->ngroups, dst->n, ctx->stream));
        return PRB_OK;
      },
      clear_grouprank);
}

// the fills scanned, the filled slots gathered by group and rank on the device, one copy
int prb_grouprank_finish(prb_ctx *ctx, prb_grouprank *t) {
  if (int rc = finish_guard(kFinishFn, kWhat, ctx, t)) return rc;
  if (t->finished) return PRB_OK; // (the records are on the host already)
  if (t->bad) return refuse(kFinishFn, kBadCandidate, PRB_ERR_STATE);
  PRB_HIP(hipSetDevice(ctx->device));
  if (int rc = finish_ranked(kFinishFn, ctx, t->fill_of(t->table.p), t->ngroups, t->entries(), t->pairs,
                             [&](const int64_t *off, int64_t total, void *out) {
                               return launch_grouprank_gather(t->keys_of(t->table.p), t->slots_of(t->table.p), off, t->ngroups, t->n, total, out,
                                                              ctx->stream);
                             }))
    return rc;
  t->finished = true;
  t->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_grouprank_size(const prb_grouprank *t) { return t ? (int64_t)t->pairs.size() : -1; }
const prb_group_pair *prb_grouprank_pairs(const prb_grouprank *t) { return t ? t->pairs.data() : nullptr; }
void prb_grouprank_counts(const prb_grouprank *t, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = t ? t->counts[i] : 0;
}
void prb_grouprank_free(prb_grouprank *t) { delete t; }

} // extern "C"
