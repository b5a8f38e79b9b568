// C ABI, part 4: the two top-N tables of a batch - the N best pairs per query (prb_topset_*) and the N best final hits
// per query with their base pairs (prb_tophits_*).
#include <cstring>

#include "capi_tables.hpp"

using namespace prb;

// a top table back to empty, on its own device and stream
template <class Slot> static int clear_top_table(TopTable<Slot> &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, std::max<size_t>(t.bytes(), 1), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  return PRB_OK;
}

// prb_topset_create / prb_tophits_create: an empty table of n slots per query of the batch
template <class T> static int create_top_table(const char *fn_name, prb_ctx *ctx, const prb_qbatch *qb, int32_t n, T **out) {
  std::unique_ptr<T> t;
  if (int rc = new_table(fn_name, ctx && qb, out, t, bad_n(n))) return rc;
  t->ctx = ctx;
  t->qb = qb;
  t->nq = qb->nq;
  t->qlen = qb->len;
  t->n = n;
  PRB_HIP(hipSetDevice(ctx->device));
  if (int rc = t->table.ensure(std::max<size_t>(t->bytes(), 1))) return rc;
  if (int rc = clear_top_table(*t)) return rc;
  *out = t.release();
  return PRB_OK;
}

// prb_topset_merge / prb_tophits_merge: what is checked before either table is touched
template <class T> static int top_tables_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const T *dst, const T *src) {
  if (int rc = merge_tables_guard(fn_name, what, ctx, dst, src)) return rc;
  if (dst->n != src->n)
    return refuse(fn_name, std::string("the ") + what + " tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per query");
  return PRB_OK;
}

// prb_topset_finish / prb_tophits_finish: the slots and fill counts to the host (one block: one copy, enqueued after
// `also_copy` has enqueued whatever else the table holds), then each(q, r, slot) for every slot in use, by query, then
// rank - the order of the host records
template <class Slot, class AlsoCopy, class Each>
static int download_slots(const char *fn_name, prb_ctx *ctx, const TopTable<Slot> &t, AlsoCopy also_copy, Each each) {
  const std::string fn = fn_name;
  try {
    std::vector<char> host(t.bytes());
    PRB_HIP(hipSetDevice(ctx->device));
    if (int rc = also_copy()) return rc;
    if (!host.empty()) PRB_HIP(hipMemcpyAsync(host.data(), t.table.p, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> fill((size_t)t.nq);
    std::memcpy(fill.data(), host.data() + t.slots_bytes(), fill.size() * sizeof(int32_t));
    for (int32_t q = 0; q < t.nq; q++) {
      if (fill[q] < 0 || fill[q] > t.n) return refuse(fn, "query " + std::to_string(q) + " has " + std::to_string(fill[q]) + " slots in use", PRB_ERR_STATE);
      for (int32_t r = 0; r < fill[q]; r++) {
        Slot x;
        std::memcpy(&x, host.data() + ((size_t)q * t.n + r) * sizeof(Slot), sizeof x);
        x.rank = r;
        if (int rc = each(q, r, x)) return rc;
      }
    }
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  return PRB_OK;
}

// What follows a merge into the top-N hit table, of a sub-batch (prb_tophits::take) or of another table (prb_tophits_merge):
// the pair counts of the slots in use, their exclusive scan, and the kept hits' base-pair lists gathered in table order
// into a second pool of exactly the scanned size, which becomes the table's.  A newcomer's bp_offset is `split` (the
// table's pool_pairs) + the place of its list in `fresh`.  `fn` names the entry point in the messages.  Synchronises.
static int regather_tophits(const char *fn, prb_ctx *ctx, prb_tophits *th, const int32_t *fresh) {
  int rc;
  const int64_t nslots = (int64_t)th->nq * th->n;
  const size_t NS = (size_t)nslots + 1;
  if ((rc = th->cnt.ensure(NS * 4)) || (rc = th->off.ensure(NS * 8))) return rc;
  PRB_HIP(launch_tophits_counts(th->table.p, th->fill(), th->n, nslots, th->cnt.as<int32_t>(), ctx->stream));
  auto counts = rocprim::make_transform_iterator(th->cnt.as<int32_t>(), ToI64());
  if ((rc = with_temp(th->scanTmp, "rocprim::exclusive_scan", [&](void *t, size_t &b) {
         return rocprim::exclusive_scan(t, b, counts, th->off.as<int64_t>(), (int64_t)0, NS, rocprim::plus<int64_t>(), ctx->stream);
       })))
    return rc;
  int64_t total = 0;
  PRB_HIP(hipMemcpyAsync(&total, th->off.as<int64_t>() + nslots, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if (total < 0) {
    set_error("top-N hit table: bad base-pair total");
    return PRB_ERR_STATE;
  }
  if (th->pool2.ensure((size_t)std::max<int64_t>(total, 1) * 8) != PRB_OK)
    return refuse(fn, "can't allocate the pool of the kept hits' base pairs (" + std::to_string(total) + " pairs)", PRB_ERR_NOMEM);
  PRB_HIP(launch_tophits_gather(th->table.p, th->fill(), th->n, nslots, th->off.as<int64_t>(), th->pool_pairs, th->pool.as<int32_t>(), fresh,
                                th->pool2.as<int32_t>(), ctx->stream));
  std::swap(th->pool, th->pool2);
  th->pool_pairs = total;
  return PRB_OK;
}

// prb_search_page_top, per sub-batch: the npairs pair records at `packed` (of the queries [q0, q1) against `page`) merged
// into the top-N table, in a bracket of the "top" timer
static int merge_top(prb_ctx *ctx, prb_topset *ts, int32_t page, int32_t q0, int32_t q1, const void *packed, int64_t npairs) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_top_merge(packed, npairs, q0, q1, page, ts->n, ts->table.p, ts->fill(), ctx->stream));
  return ctx->time_end(ModeTimer::kTop, 1);
}
int prb_topset::take(const SubBatch &b) { return merge_top(ctx, this, b.page, b.q0, b.q1, b.records, b.npairs); }

// prb_search_page_tophits, per sub-batch: the hits' records merged into the top-N hit table, then the kept hits'
// base-pair lists gathered in table order - survivors from the table's pool, newcomers from this sub-batch's pairs
// (regather_tophits) -, in a bracket of the "tophits" timer
int prb_tophits::take(const SubBatch &b) {
  int rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_tophits_merge(b.records, b.nfin, b.q0, b.q1, b.page, n, table.p, fill(), ctx->stream));
  if ((rc = regather_tophits("prb_search_page_tophits", ctx, this, b.fresh_bp))) return rc;
  return ctx->time_end(ModeTimer::kTopHits, 4);
}

extern "C" {

int prb_topset_create(prb_ctx *ctx, const prb_qbatch *qb, int32_t n, prb_topset **out) {
  return create_top_table("prb_topset_create", ctx, qb, n, out);
}

int prb_search_page_top(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_topset *ts) {
  return merge_page("prb_search_page_top", "top-N", "prb_topset_finish", ts, ctx, qb, db, page, opts);
}

int prb_topset_finish(prb_ctx *ctx, prb_topset *ts) {
  if (int rc = finish_guard("prb_topset_finish", "top-N", ctx, ts)) return rc;
  if (ts->finished) return PRB_OK; // (the records are on the host already)
  ts->pairs.clear();
  const int rc = download_slots("prb_topset_finish", ctx, *ts, nothing_more, [&](int32_t, int32_t, const prb_top_pair &p) -> int {
    ts->pairs.push_back(p);
    return PRB_OK;
  });
  if (rc) return rc;
  ts->finished = true;
  ts->table.release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int prb_topset_merge(prb_ctx *ctx, prb_topset *dst, prb_topset *src) {
  if (int rc = top_tables_guard("prb_topset_merge", "top-N", ctx, dst, src)) return rc;
  return join_tables(
      "prb_topset_merge", ModeTimer::kTop, 1, ctx, dst, src, src->bytes(), nothing_more,
      [&](void *slots) -> int {
        PRB_HIP(launch_top_join(dst->table.p, dst->fill(), slots, reinterpret_cast<const int32_t *>(static_cast<char *>(slots) + src->slots_bytes()),
                                dst->nq, dst->n, ctx->stream));
        return PRB_OK;
      },
      clear_top_table<prb_top_pair>);
}

int64_t prb_topset_size(const prb_topset *ts) { return ts ? (int64_t)ts->pairs.size() : -1; }
const prb_top_pair *prb_topset_pairs(const prb_topset *ts) { return ts ? ts->pairs.data() : nullptr; }
void prb_topset_counts(const prb_topset *ts, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ts ? ts->counts[i] : 0;
}
void prb_topset_free(prb_topset *ts) {
  delete ts;
}

int prb_tophits_create(prb_ctx *ctx, const prb_qbatch *qb, int32_t n, prb_tophits **out) {
  return create_top_table("prb_tophits_create", ctx, qb, n, out);
}

int prb_search_page_tophits(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_tophits *th) {
  // (with the other checks' guarantee: a refused call leaves the table as it was)
  if (th && opts && th->style >= 0 && opts->output_style != th->style)
    return refuse("prb_search_page_tophits", "the top-N hit table holds pages searched with output_style " + std::to_string(th->style) +
                                                 " (this call: " + std::to_string(opts->output_style) + ")");
  const int rc = merge_page("prb_search_page_tophits", "top-N hit", "prb_tophits_finish", th, ctx, qb, db, page, opts);
  if (rc == PRB_OK) th->style = opts->output_style;
  return rc;
}

// the table's slots and fill counts are one block, the pool another: one copy each
int prb_tophits_finish(prb_ctx *ctx, prb_tophits *th) {
  if (int rc = finish_guard("prb_tophits_finish", "top-N hit", ctx, th)) return rc;
  if (th->finished) return PRB_OK; // (the records are on the host already)
  th->hits.clear();
  int64_t next = 0; // the lists lie in table order without gaps: in record order
  const int rc = download_slots(
      "prb_tophits_finish", ctx, *th,
      [&]() -> int {
        th->bp.assign((size_t)th->pool_pairs * 2, 0);
        if (!th->bp.empty()) PRB_HIP(hipMemcpyAsync(th->bp.data(), th->pool.p, th->bp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        return PRB_OK;
      },
      [&](int32_t q, int32_t r, const prb_top_hit &x) -> int {
        if (x.h.bp_offset != next || x.h.bp_count < 0)
          return refuse("prb_tophits_finish", "the base pairs of query " + std::to_string(q) + ", rank " + std::to_string(r) + " are out of place",
                        PRB_ERR_STATE);
        next += x.h.bp_count;
        th->hits.push_back(x);
        return PRB_OK;
      });
  if (rc) return rc;
  if (next != th->pool_pairs)
    return refuse("prb_tophits_finish", std::to_string(th->pool_pairs) + " base pairs in the pool, " + std::to_string(next) + " in the records",
                  PRB_ERR_STATE);
  th->finished = true;
  th->release(); // (only the host copies are needed from here on)
  return PRB_OK;
}

// the records as prb_topset_merge merges them, src's lists addressed behind dst's pool; then the scan and the gather of
// prb_search_page_tophits with src's pool as the newcomers' source
int prb_tophits_merge(prb_ctx *ctx, prb_tophits *dst, prb_tophits *src) {
  if (dst && src && dst->style >= 0 && src->style >= 0 && dst->style != src->style)
    return refuse("prb_tophits_merge", "the top-N hit tables hold pages searched with output_style " + std::to_string(dst->style) + " and " +
                                           std::to_string(src->style));
  if (int rc = top_tables_guard("prb_tophits_merge", "top-N hit", ctx, dst, src)) return rc;
  ScratchBuf pool_copy;
  void *pool = nullptr;
  const int rc = join_tables(
      "prb_tophits_merge", ModeTimer::kTopHits, 4, ctx, dst, src, src->bytes(),
      [&]() -> int { return on_device_of(ctx, src->ctx, src->pool.p, (size_t)src->pool_pairs * 8, pool_copy, &pool); },
      [&](void *slots) -> int {
        PRB_HIP(launch_tophits_join(dst->table.p, dst->fill(), slots, reinterpret_cast<const int32_t *>(static_cast<char *>(slots) + src->slots_bytes()),
                                    dst->nq, dst->n, dst->pool_pairs, ctx->stream));
        return regather_tophits("prb_tophits_merge", ctx, dst, static_cast<const int32_t *>(pool));
      },
      clear_top_table<prb_top_hit>);
  if (rc) return rc;
  if (dst->style < 0) dst->style = src->style;
  src->style = -1;
  src->pool_pairs = 0;
  return PRB_OK;
}

int64_t prb_tophits_size(const prb_tophits *th) { return th ? (int64_t)th->hits.size() : -1; }
const prb_top_hit *prb_tophits_hits(const prb_tophits *th) { return th ? th->hits.data() : nullptr; }
const int32_t *prb_tophits_basepairs(const prb_tophits *th, int64_t *npairs) {
  if (!th) return nullptr;
  if (npairs) *npairs = (int64_t)th->bp.size() / 2;
  return th->bp.data();
}
void prb_tophits_counts(const prb_tophits *th, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = th ? th->counts[i] : 0;
}
void prb_tophits_free(prb_tophits *th) {
  delete th;
}

} // extern "C"
