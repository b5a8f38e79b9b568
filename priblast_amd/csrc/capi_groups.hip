// C ABI, part 11: the group table of one batch - per (query, group of database sequences), the group's best member pair
// and the integer sums over its members (prb_groupset_*, `ris -t -G FILE`).  The kernels are in group_kernels.hip.  Every
// check of a call is made on the host before anything is enqueued: a refused call leaves the table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kFinishFn = "prb_groupset_finish";
const char *const kBadRecord = "a record merged into this group table named a query, a sequence, a page or a group outside it";

// a group table back to empty, on its own device and stream
int clear_group_table(prb_groupset &gs) {
  PRB_HIP(hipSetDevice(gs.ctx->device));
  PRB_HIP(launch_group_clear(gs.view(), gs.ctx->stream));
  PRB_HIP(hipStreamSynchronize(gs.ctx->stream));
  return PRB_OK;
}

} // namespace

// prb_search_page_groups (per sub-batch) and prb_groupset_add_pairs: the records folded into their slots, in a bracket of
// the "group" timer
static int merge_group_pairs(prb_ctx *ctx, prb_groupset *gs, int32_t page, const void *packed, int64_t npairs) {
  int rc;
  if (page < 0 || (size_t)page >= gs->map_dev.size()) return refuse("prb_search_page_groups", "page out of range", PRB_ERR_STATE);
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_group_fold(packed, npairs, gs->view(), gs->page_view((size_t)page), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kGroup, 3))) return rc;
  if ((rc = fetch_bad(ctx, gs))) return rc;
  if (gs->bad) return refuse("prb_search_page_groups", kBadRecord, PRB_ERR_STATE);
  return PRB_OK;
}
int prb_groupset::take(const SubBatch &b) { return merge_group_pairs(ctx, this, b.page, b.records, b.npairs); }

// prb_groupset_finish (and prb_gnullset_create, which keeps the records on the device): the occupied slots selected on the
// device - with n > 0 each query's n lowest keys among them -, their records gathered there and copied once
int prb::finish_groupset(const char *fn, prb_ctx *ctx, prb_groupset *gs, int32_t n, prb_gnullset *keep) {
  if (int rc = finish_guard(fn, "group", ctx, gs)) return rc;
  if (gs->finished) return PRB_OK; // (the records are on the host already)
  if (gs->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (n < 0 || n > kTopMaxN) return refuse(fn, "need 0 <= n <= " + std::to_string(kTopMaxN) + " (got " + std::to_string(n) + ")");
  gs->pairs.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  const int64_t S = gs->slots();
  if (S > 0) {
    int rc;
    SearchWs &w = ws_of(ctx);
    if ((rc = gs->occ.ensure((size_t)S)) || (rc = gs->sel.ensure((size_t)S * 4)) || (rc = w.count.ensure(16))) return rc;
    if ((rc = ctx->time_begin())) return rc;
    int64_t launches = 2, nsel = 0;
    PRB_HIP(launch_group_flags(gs->view(), gs->occ.as<uint8_t>(), ctx->stream));
    if ((rc = select_flagged(ctx, w, nullptr, gs->occ.as<uint8_t>(), gs->sel.as<uint32_t>(), (size_t)S, &nsel))) return rc;
    if (nsel < 0 || nsel > S) return refuse(fn, "bad record count " + std::to_string(nsel), PRB_ERR_STATE);
    const uint32_t *idx = gs->sel.as<uint32_t>(), *top = nullptr;
    if (nsel && n > 0) {
      // each query's n lowest keys: top[q * n + r]; the ranks in use selected in (query, rank) order into occ's place
      const size_t T = (size_t)gs->nq * (size_t)n;
      if ((rc = gs->top.ensure(T * 4)) || (rc = gs->keep.ensure(T)) || (rc = gs->out.ensure(T * 4))) return rc;
      PRB_HIP(launch_group_select(gs->view(), gs->sel.as<uint32_t>(), nsel, n, gs->top.as<uint32_t>(), gs->keep.as<uint8_t>(), ctx->stream));
      if ((rc = select_flagged(ctx, w, nullptr, gs->keep.as<uint8_t>(), gs->out.as<uint32_t>(), T, &nsel))) return rc;
      if (nsel < 0 || nsel > (int64_t)T) return refuse(fn, "bad record count " + std::to_string(nsel), PRB_ERR_STATE);
      std::swap(gs->sel, gs->out); // (sel = the kept ranks; out is free for the records)
      idx = gs->sel.as<uint32_t>();
      top = gs->top.as<uint32_t>();
      launches += 2;
    }
    if (nsel) {
      try {
        gs->pairs.resize((size_t)nsel);
      } catch (const std::exception &e) {
        return refuse(fn, e.what(), PRB_ERR_NOMEM);
      }
      const size_t bytes = (size_t)nsel * sizeof(prb_group_pair);
      if ((rc = gs->out.ensure(bytes))) return rc;
      PRB_HIP(launch_group_gather(gs->view(), idx, nsel, top, n, gs->out.p, ctx->stream));
      PRB_HIP(hipMemcpyAsync(gs->pairs.data(), gs->out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
      launches++;
    }
    if ((rc = ctx->time_end(ModeTimer::kGroup, launches))) return rc; // (synchronises: the copy is over)
    if ((rc = fetch_bad(ctx, gs))) return rc;
    if (gs->bad) {
      gs->pairs.clear();
      return refuse(fn, "a selected slot lies outside the group table", PRB_ERR_STATE);
    }
  }
  if (keep)
    if (int rc = keep_group_records(ctx, keep, gs, gs->pairs.empty() ? nullptr : gs->out.p, (int64_t)gs->pairs.size())) return rc;
  gs->finished = true;
  gs->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

extern "C" {

int prb_groupset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, const int32_t *const *group_of_page, int32_t ngroups,
                        prb_groupset **out) {
  const char *fn = "prb_groupset_create";
  std::unique_ptr<prb_groupset> gs;
  const bool args_ok = ctx && qb && db && group_of_page && qb->ctx->device == ctx->device && db->ctx->device == ctx->device;
  int64_t nseq_all = 0;
  if (args_ok)
    for (const DbPage &pg : db->pages) nseq_all += pg.nseq;
  if (int rc = new_table(fn, args_ok, out, gs,
                         ngroups < 1 || ngroups > nseq_all
                             ? "need 1 <= ngroups <= " + std::to_string(nseq_all) + ", the sequences of the database (got " + std::to_string(ngroups) + ")"
                             : ""))
    return rc;
  try {
    gs->map.resize(db->pages.size());
    for (size_t p = 0; p < db->pages.size(); p++) {
      const int32_t nseq = db->pages[p].nseq;
      if (nseq && !group_of_page[p]) return refuse(fn, "no group map for page " + std::to_string(p));
      for (int32_t i = 0; i < nseq; i++)
        if (group_of_page[p][i] < 0 || group_of_page[p][i] >= ngroups)
          return refuse(fn, "the group of sequence " + std::to_string(i) + " of page " + std::to_string(p) + " is " + std::to_string(group_of_page[p][i]) +
                                " (the table has " + std::to_string(ngroups) + " groups)");
      gs->map[p].assign(group_of_page[p], group_of_page[p] + nseq);
    }
    gs->merged.assign(db->pages.size(), 0);
    gs->qlen = qb->len;
    gs->map_dev.resize(db->pages.size());
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  gs->nq = qb->nq;
  gs->ngroups = ngroups;
  if (gs->slots() > (int64_t)UINT32_MAX)
    return refuse(fn, "the batch and the map have " + std::to_string(gs->slots()) + " (query, group) slots (at most 2^32 - 1)");
  gs->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  gs->db = db;
  gs->qb = qb;
  PRB_HIP(hipSetDevice(ctx->device));
  bool ok = gs->table.ensure(std::max<size_t>(gs->bytes(), 16)) == PRB_OK && gs->badflag.ensure(16) == PRB_OK;
  for (size_t p = 0; ok && p < gs->map.size(); p++) ok = gs->map_dev[p].ensure(std::max<size_t>(gs->map[p].size() * 4, 16)) == PRB_OK;
  if (!ok)
    return refuse(fn, "can't allocate the group table (" + std::to_string(gs->bytes() >> 20) + " MB of HBM for " + std::to_string(gs->nq) + " queries x " +
                          std::to_string(ngroups) + " groups)",
                  PRB_ERR_NOMEM);
  PRB_HIP(hipMemsetAsync(gs->badflag.p, 0, 16, ctx->stream));
  for (size_t p = 0; p < gs->map.size(); p++)
    if (!gs->map[p].empty())
      PRB_HIP(hipMemcpyAsync(gs->map_dev[p].p, gs->map[p].data(), gs->map[p].size() * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(launch_group_clear(gs->view(), ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  *out = gs.release();
  return PRB_OK;
}

int prb_search_page_groups(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_groupset *gs) {
  const char *fn = "prb_search_page_groups";
  if (gs && gs->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  return merge_page(fn, "group", kFinishFn, gs, ctx, qb, db, page, opts);
}

int prb_groupset_add_pairs(prb_ctx *ctx, prb_groupset *gs, int32_t page, const prb_pair_summary *pairs, int64_t n) {
  const char *fn = "prb_groupset_add_pairs";
  if (!ctx || !gs || n < 0 || n > INT32_MAX || (n && !pairs)) return refuse(fn, "bad argument");
  if (gs->ctx != ctx) return refuse(fn, "the group table was made with another context");
  if (gs->broken) return refuse(fn, "an earlier merge into this group table failed", PRB_ERR_STATE);
  if (gs->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (gs->finished) return refuse(fn, std::string("the group table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  if (page < 0 || (size_t)page >= gs->merged.size())
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(gs->merged.size()) + ")");
  if (gs->merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged into this group table");
  if (int rc = records_guard(fn, (int64_t)gs->map[(size_t)page].size(), gs->nq, pairs, n)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  gs->merged[(size_t)page] = 1;
  if (!n) return PRB_OK;
  gs->broken = true; // (until the merge is whole)
  if (int rc = upload_records(ctx, gs->h_rec, pairs, n)) return rc;
  if (int rc = merge_group_pairs(ctx, gs, page, gs->h_rec.p, n)) return rc;
  gs->broken = false;
  return PRB_OK;
}

int prb_groupset_merge(prb_ctx *ctx, prb_groupset *dst, prb_groupset *src) {
  const char *fn = "prb_groupset_merge";
  if (int rc = merge_tables_guard(fn, "group", ctx, dst, src)) return rc;
  if (dst->bad || src->bad) return refuse(fn, kBadRecord, PRB_ERR_STATE);
  if (dst->ngroups != src->ngroups || dst->map != src->map) return refuse(fn, "the group tables were made with different group maps");
  const prb_db *db = src->db;
  const size_t npages = src->merged.size();
  const int rc = join_tables(
      fn, ModeTimer::kGroup, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *slots) -> int {
        PRB_HIP(launch_group_join(dst->view(), static_cast<const GroupSlot *>(slots), ctx->stream));
        return PRB_OK;
      },
      clear_group_table);
  // (src stays a table of its database, with no page merged: it can be finished to zero records)
  src->db = db;
  src->merged.assign(npages, 0);
  return rc;
}

int prb_groupset_finish(prb_ctx *ctx, prb_groupset *gs, int32_t n) { return finish_groupset(kFinishFn, ctx, gs, n, nullptr); }

int64_t prb_groupset_size(const prb_groupset *gs) { return gs ? (int64_t)gs->pairs.size() : -1; }
const prb_group_pair *prb_groupset_pairs(const prb_groupset *gs) { return gs ? gs->pairs.data() : nullptr; }
void prb_groupset_counts(const prb_groupset *gs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = gs ? gs->counts[i] : 0;
}
void prb_groupset_free(prb_groupset *gs) { delete gs; }

} // extern "C"
