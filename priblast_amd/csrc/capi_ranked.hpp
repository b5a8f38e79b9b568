// The protocol of the three ranked run tables, each step once (capi_targets.hip, capi_grouprank.hip, capi_featrank.hip;
// RankedTable, search_host.hpp; the kernels: ranked_kernels.hip): a merge's candidates into the lists, a caller's records
// checked and merged, two tables into one, and the finish.  The per-table files keep their create, the feed that is
// theirs alone - a search's sub-batches, a batch's group table, a batch's feature table - with its own checks of the
// source, and the entry points.  Every check of a call is made on the host before anything is enqueued: a refused call
// leaves the table as it was.
#pragma once
#include "capi_tables.hpp"

namespace prb {

// a table's nouns in the messages, and its stage timer
struct RankedNouns {
  const char *what;          // "group ranking": the table
  const char *list, *lists;  // "group", "groups": what it ranks for
  const char *owner;         // "table", "annotation": what has the lists, where a caller's record names one outside
  const char *candidates;    // "candidates", "pairs": what is merged
  const char *finish_fn;     // "prb_grouprank_finish"
  const char *bad_candidate; // the refusal behind the device's `bad` flag (a table without one: unused)
  ModeTimer timer;
};

// ---- a merge's candidates into the ranked lists
// The ncand candidates of `feed` (search_kernels.hpp), which name nlists lists, grouped by list and merged into the table
// `t` (inside the caller's bracket of the table's timer): their lists as sort keys, the stable sort, their rank keys and
// the heads of the lists' runs, the heads' places, and every run into its list; 5 launches
template <class T, class Feed> int merge_ranked_candidates(prb_ctx *ctx, T *t, const RankedNouns &nn, const Feed &feed, int32_t nlists, int64_t ncand) {
  int rc;
  SearchWs &w = ws_of(ctx);
  const size_t NC = (size_t)ncand;
  if ((rc = w.count.ensure(16)) || (rc = t->key.ensure(NC * 4)) || (rc = t->keyS.ensure(NC * 4)) || (rc = t->val.ensure(NC * 4)) ||
      (rc = t->valS.ensure(NC * 4)) || (rc = t->rkey.ensure(NC * sizeof(TargetKey))) || (rc = t->head.ensure(NC)) || (rc = t->start.ensure(NC * 4)))
    return rc;
  uint32_t *const keyS = t->keyS.template as<uint32_t>(), *const valS = t->valS.template as<uint32_t>();
  PRB_HIP(launch_ranked_lists(feed, t->key.template as<uint32_t>(), t->val.template as<uint32_t>(), ctx->stream));
  if ((rc = sort_target_keys(ctx->stream, t->sortTmp, t->key.template as<uint32_t>(), keyS, t->val.template as<uint32_t>(), valS, NC,
                             (unsigned)bits_for(std::max(nlists - 1, 1)))))
    return rc;
  PRB_HIP(launch_ranked_runs(feed, keyS, valS, t->rkey.template as<TargetKey>(), t->head.template as<uint8_t>(), ctx->stream));
  int64_t nruns = 0;
  if ((rc = select_flagged(ctx, w, nullptr, t->head.template as<uint8_t>(), t->start.template as<uint32_t>(), NC, &nruns))) return rc;
  if (nruns <= 0 || nruns > ncand || nruns > nlists) {
    set_error(std::string(nn.what) + " table: " + std::to_string(nruns) + " " + nn.lists + " for " + std::to_string(ncand) + " " + nn.candidates);
    return PRB_ERR_STATE;
  }
  PRB_HIP(launch_ranked_merge(feed, RankedRuns{t->rkey.template as<TargetKey>(), keyS, t->start.template as<uint32_t>(), nruns, ncand},
                              t->lists_of(t->table.p), ctx->stream));
  return PRB_OK;
}

// ---- prb_grouprank_add_* / prb_featrank_add_*
// what both merges check of the table first
template <class T> int ranked_guard(const char *fn, const RankedNouns &nn, const prb_ctx *ctx, const T *t) {
  const std::string table = std::string("the ") + nn.what + " table";
  if (t->ctx != ctx) return refuse(fn, table + " was made with another context");
  if (t->broken) return refuse(fn, std::string("an earlier merge into this ") + nn.what + " table failed", PRB_ERR_STATE);
  if (t->bad) return refuse(fn, nn.bad_candidate, PRB_ERR_STATE);
  if (t->finished) return refuse(fn, table + " is finished (" + nn.finish_fn + ")", PRB_ERR_STATE);
  return PRB_OK;
}
// behind a merge: the device's flag
template <class T> int ranked_bad_guard(const char *fn, const RankedNouns &nn, prb_ctx *ctx, T *t) {
  if (int rc = fetch_bad(ctx, t)) return rc;
  return t->bad ? refuse(fn, nn.bad_candidate, PRB_ERR_STATE) : PRB_OK;
}
// `feed`'s ncand candidates (none: nothing is done) merged into `t` in a bracket of its timer - `launches` more than
// the merge's own are booked -, then the device's flag.  A failure leaves the table unusable.
template <class T, class Feed>
int feed_ranked(const char *fn, const RankedNouns &nn, prb_ctx *ctx, T *t, const Feed &feed, int64_t ncand, int64_t launches = 0) {
  int rc;
  if (ncand) {
    if ((rc = merge_ranked_candidates(ctx, t, nn, feed, (int32_t)t->targets(), ncand))) return rc;
    launches += 5;
  }
  if ((rc = ctx->time_end(nn.timer, launches))) return rc;
  return ranked_bad_guard(fn, nn, ctx, t);
}
// A caller's n records merged: list_of(r) is the list that record r names and id_of(r) its query identifier.  Every
// list lies in the table, every identifier is >= 0, no (identifier, list) comes twice, and no identifier was merged before.
template <class T, class ListOf, class IdOf>
int add_ranked_records(const char *fn, const RankedNouns &nn, prb_ctx *ctx, T *t, const typename T::Payload *recs, int64_t n, ListOf list_of,
                       IdOf id_of) {
  using Payload = typename T::Payload;
  if (!ctx || !t || n < 0 || n > INT32_MAX || (n && !recs)) return refuse(fn, "bad argument");
  if (int rc = ranked_guard(fn, nn, ctx, t)) return rc;
  const int64_t L = t->targets();
  std::vector<int32_t> ids;
  try {
    std::vector<int64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const int32_t l = list_of(recs[i]), id = id_of(recs[i]);
      if (l < 0 || l >= L)
        return refuse(fn, "record " + std::to_string(i) + " names " + nn.list + " " + std::to_string(l) + " (the " + nn.owner + " has " +
                              std::to_string(L) + ")");
      if (id < 0) return refuse(fn, "query identifier " + std::to_string(id) + " is below 0");
      keys[(size_t)i] = (int64_t)id * L + l;
    }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size(); i++) {
      if (i && keys[i] == keys[i - 1])
        return refuse(fn, "query identifier " + std::to_string(keys[i] / L) + " is given twice for " + nn.list + " " + std::to_string(keys[i] % L));
      const int32_t id = (int32_t)(keys[i] / L);
      if (ids.empty() || ids.back() != id) ids.push_back(id);
    }
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  // (the last check: a call that passes has its identifiers marked as merged)
  if (int rc = run_table_guard(fn, nn.what, nn.finish_fn, t, ctx, t->db, 0, -1, -1, ids.data(), (int32_t)ids.size())) return rc;
  if (!n) return PRB_OK;
  t->broken = true; // (until the merge is whole)
  int rc;
  const size_t bytes = (size_t)n * sizeof(Payload);
  if ((rc = t->h_rec.ensure(bytes))) return rc;
  PRB_HIP(hipMemcpyAsync(t->h_rec.p, recs, bytes, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = feed_ranked(fn, nn, ctx, t, RecordFeed<Payload>{t->h_rec.p, n, (int32_t)L, t->badflag.template as<uint32_t>()}, n))) return rc;
  t->broken = false;
  return PRB_OK;
}

// ---- prb_*_merge: two unfinished ranked tables over disjoint (page, identifier) sets into one
// carry(dst, src): what the table has beside its lists, from src to dst (called once src's lists are enqueued)
template <class T, class Carry> int merge_ranked_tables(const char *fn, const RankedNouns &nn, prb_ctx *ctx, T *dst, T *src, Carry carry) {
  const std::string tables = std::string("the ") + nn.what + " tables";
  if (int rc = run_tables_guard(fn, nn.what, ctx, dst, src, [&]() -> std::string {
        if (!dst->db && dst->targets() != src->targets()) // (lists of the tables' own: else a database's, which run_tables_guard compares)
          return tables + " have " + std::to_string(dst->targets()) + " and " + std::to_string(src->targets()) + " " + nn.lists;
        if (dst->n != src->n) return tables + " keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per " + nn.list;
        return "";
      }))
    return rc;
  if (dst->bad || src->bad) return refuse(fn, nn.bad_candidate, PRB_ERR_STATE);
  return join_tables(
      fn, nn.timer, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *block) -> int {
        PRB_HIP(launch_ranked_join<typename T::Payload>(dst->lists_of(dst->table.p), dst->lists_of(block), ctx->stream));
        carry(dst, src);
        return PRB_OK;
      },
      [](T &t) { return t.clear(); });
}
inline void nothing_to_carry(const void *, const void *) {}

// ---- prb_*_finish: the ranked lists to the host
// The fills (L + 1 values, the last one 0) scanned, the filled slots gathered by list and rank on the device, one copy
// to t->recs; then only the host records are needed, and the device memory is released
template <class T> int finish_ranked(const RankedNouns &nn, prb_ctx *ctx, T *t) {
  using Payload = typename T::Payload;
  const char *fn = nn.finish_fn;
  if (int rc = finish_guard(fn, nn.what, ctx, t)) return rc;
  if (t->finished) return PRB_OK; // (the records are on the host already)
  if (t->bad) return refuse(fn, nn.bad_candidate, PRB_ERR_STATE);
  PRB_HIP(hipSetDevice(ctx->device));
  const RankedLists l = t->lists_of(t->table.p);
  int rc;
  ScratchBuf off, out, tmp;
  if ((rc = off.ensure(((size_t)l.nlists + 1) * 8))) return rc;
  auto fills = rocprim::make_transform_iterator(static_cast<const int32_t *>(l.fill), ToI64());
  if ((rc = with_temp(tmp, "rocprim::exclusive_scan", [&](void *p, size_t &b) {
         return rocprim::exclusive_scan(p, b, fills, off.as<int64_t>(), (int64_t)0, (size_t)l.nlists + 1, rocprim::plus<int64_t>(), ctx->stream);
       })))
    return rc;
  int64_t total = 0;
  PRB_HIP(hipMemcpyAsync(&total, off.as<int64_t>() + l.nlists, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if (total < 0 || (uint64_t)total > (uint64_t)t->entries()) return refuse(fn, "bad record count " + std::to_string(total), PRB_ERR_STATE);
  t->recs.clear();
  if (total) {
    try {
      t->recs.resize((size_t)total);
    } catch (const std::exception &e) {
      return refuse(fn, e.what(), PRB_ERR_NOMEM);
    }
    if ((rc = out.ensure((size_t)total * sizeof(Payload)))) return rc;
    PRB_HIP(launch_ranked_gather<Payload>(l, off.as<int64_t>(), total, out.p, ctx->stream));
    PRB_HIP(hipMemcpyAsync(t->recs.data(), out.p, (size_t)total * sizeof(Payload), hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
  }
  t->finished = true;
  t->release();
  return PRB_OK;
}

} // namespace prb
