// C ABI, part 4: the tables and record sets a search fills - the top-N table (prb_topset_*), the top-N hit table
// (prb_tophits_*), the per-position profile (prb_profset_*), the per-target table (prb_targetset_*), the per-target
// coverage table (prb_covset_*), per-pair records (prb_pairset_*), hit sets (prb_hitset_*).
#include <algorithm>
#include <cstring>
#include <functional>

#include "search_host.hpp"

using namespace prb;

namespace {
// a slot of the profile table that some final hit covers (prb_profset_finish: `hits` holds the scanned counts)
struct ProfCovered {
  const int64_t *hits;
  __host__ __device__ bool operator()(const uint32_t &p) const { return hits[p] > 0; }
};
// a fill count as what the scan of prb_targetset_finish adds up
struct FillToI64 {
  __host__ __device__ int64_t operator()(const int32_t &x) const { return (int64_t)x; }
};
// the first slot of a region of the coverage table at depth D (prb_covset_finish: `queries` holds the scanned counts; a
// sequence's separator slot has none, so the slot in front of a sequence's first one is always below D)
struct CovHead {
  const int32_t *queries;
  int32_t D;
  __host__ __device__ bool operator()(const uint32_t &p) const { return queries[p] >= D && (p == 0 || queries[p - 1] < D); }
};
// the caller's current device, put back on every way out of a call that visits another table's device
struct DeviceScope {
  int prev = -1;
  DeviceScope() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
// device / pinned memory that lives as long as one call
struct ScratchBuf : DevBuf {
  ~ScratchBuf() { release(); }
};
struct ScratchPin : PinnedBuf {
  ~ScratchPin() { release(); }
};
} // namespace

// prb_search_page_top / prb_search_page_profile / prb_search_page_tophits: page `page` searched and merged into the table `t` - `what` in the
// messages, finished by `finish_fn`.  Every check comes before the table is touched: a refused call leaves it as it was.
static int merge_page(const char *fn_name, const char *what, const char *finish_fn, SearchMode mode, MergeTable *t, prb_ctx *ctx,
                      prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts) {
  const std::string fn = fn_name, table = std::string(what) + " table";
  if (!t) {
    set_error(fn + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (int rc = check_search_args(fn_name, ctx, qb, db, page, opts, 3)) return rc;
  if (t->ctx != ctx || t->qb != qb || t->nq != qb->nq) {
    set_error(fn + ": the " + table + " was made for another context or query batch (" + std::to_string(t->nq) +
              " queries; this batch has " + std::to_string(qb->nq) + ")");
    return PRB_ERR_ARG;
  }
  if (t->db && t->db != db) {
    set_error(fn + ": the " + table + " holds pages of another database");
    return PRB_ERR_ARG;
  }
  if (t->broken) {
    set_error(fn + ": an earlier merge into this " + table + " failed");
    return PRB_ERR_STATE;
  }
  if (t->finished) {
    set_error(fn + ": the " + table + " is finished (" + finish_fn + ")");
    return PRB_ERR_STATE;
  }
  if (t->distinct >= 0 && opts->distinct_sites != t->distinct) {
    set_error(fn + ": the " + table + " holds pages searched with distinct_sites " + std::to_string(t->distinct) + " (this call: " +
              std::to_string(opts->distinct_sites) + ")");
    return PRB_ERR_ARG;
  }
  if (!t->db) {
    t->db = db;
    t->merged.assign(db->pages.size(), 0);
  }
  if (t->merged[(size_t)page]) {
    set_error(fn + ": page " + std::to_string(page) + " is already merged into this " + table);
    return PRB_ERR_ARG;
  }
  t->merged[(size_t)page] = 1;
  prb_hitset *hs = nullptr;
  const int rc = search_page(ctx, qb, db, page, opts, 3, mode, &hs, t);
  if (rc != PRB_OK) {
    t->broken = true;
    return rc;
  }
  for (int i = 0; i < 3; i++) t->counts[i] += hs->counts[i];
  t->distinct = opts->distinct_sites;
  delete hs;
  return PRB_OK;
}

// prb_topset_create / prb_tophits_create: an empty table of n slots per query of the batch
template <class T> static int create_top_table(const char *fn_name, prb_ctx *ctx, const prb_qbatch *qb, int32_t n, T **out) {
  const std::string fn = fn_name;
  if (!ctx || !qb || !out) {
    set_error(fn + ": bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  if (n < 1 || n > kTopMaxN) {
    set_error(fn + ": need 1 <= n <= " + std::to_string(kTopMaxN) + " (got " + std::to_string(n) + ")");
    return PRB_ERR_ARG;
  }
  std::unique_ptr<T> t(new (std::nothrow) T());
  if (!t) {
    set_error(fn + ": out of host memory");
    return PRB_ERR_NOMEM;
  }
  t->ctx = ctx;
  t->qb = qb;
  t->nq = qb->nq;
  t->qlen = qb->len;
  t->n = n;
  PRB_HIP(hipSetDevice(ctx->device));
  const size_t bytes = std::max<size_t>(t->slots_bytes() + (size_t)qb->nq * sizeof(int32_t), 1);
  if (int rc = t->table.ensure(bytes)) return rc;
  PRB_HIP(hipMemsetAsync(t->table.p, 0, bytes, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  *out = t.release();
  return PRB_OK;
}

// What every prb_*_finish starts with: the table `t` - `what` in the messages - belongs to ctx and no merge into it failed
static int finish_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const MergeTable *t) {
  if (!ctx || !t || t->ctx != ctx) {
    set_error(std::string(fn_name) + ": bad argument (the table belongs to another context)");
    return PRB_ERR_ARG;
  }
  if (t->broken) {
    set_error(std::string(fn_name) + ": an earlier merge into this " + what + " table failed");
    return PRB_ERR_STATE;
  }
  return PRB_OK;
}

// ---- prb_topset_merge / prb_tophits_merge / prb_profset_merge: two unfinished tables over disjoint page sets into one
// What the three check before either table is touched: `dst` - `what` in the messages - belongs to ctx, both are
// unfinished and whole, made for the same queries, and no page is in both.
static int merge_tables_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const MergeTable *dst, const MergeTable *src) {
  const std::string fn = fn_name, tables = std::string(what) + " tables";
  auto refuse = [&](const std::string &why) {
    set_error(fn + ": " + why);
    return PRB_ERR_ARG;
  };
  if (!ctx || !dst || !src || dst == src) return refuse("bad argument");
  if (dst->ctx != ctx) return refuse("the table to merge into belongs to another context");
  if (dst->broken || src->broken) return refuse("an earlier merge into one of the " + tables + " failed");
  if (dst->finished || src->finished) return refuse("one of the " + tables + " is finished");
  if (dst->nq != src->nq) return refuse("the " + tables + " were made for " + std::to_string(dst->nq) + " and " + std::to_string(src->nq) + " queries");
  if (dst->qlen != src->qlen) return refuse("the " + tables + " were made for queries of different lengths");
  if (dst->distinct >= 0 && src->distinct >= 0 && dst->distinct != src->distinct)
    return refuse("the " + tables + " hold pages searched with distinct_sites " + std::to_string(dst->distinct) + " and " +
                  std::to_string(src->distinct));
  if (dst->db && src->db) {
    if (dst->merged.size() != src->merged.size())
      return refuse("the " + tables + " hold pages of databases of " + std::to_string(dst->merged.size()) + " and " +
                    std::to_string(src->merged.size()) + " pages");
    for (size_t p = 0; p < dst->merged.size(); p++)
      if (dst->merged[p] && src->merged[p]) return refuse("page " + std::to_string(p) + " is merged into both " + tables);
  }
  return PRB_OK;
}
// after the merge: dst's page set is the union and its counts the sums; src has merged nothing
static void move_pages(MergeTable *dst, MergeTable *src) {
  if (src->db) {
    if (!dst->db) {
      dst->db = src->db;
      dst->merged = src->merged;
    } else {
      for (size_t p = 0; p < dst->merged.size(); p++) dst->merged[p] |= src->merged[p];
    }
  }
  for (int i = 0; i < 3; i++) {
    dst->counts[i] += src->counts[i];
    src->counts[i] = 0;
  }
  if (dst->distinct < 0) dst->distinct = src->distinct;
  src->distinct = -1;
  src->db = nullptr;
  src->merged.clear();
}
// `bytes` at p on device `from` into `scratch` on ctx's device (the current one), complete on return or in order on
// ctx's stream: a peer copy where the devices allow it, else through pinned host memory
static int fetch_remote(prb_ctx *ctx, int from, const void *p, size_t bytes, DevBuf &scratch) {
  if (int rc = scratch.ensure(std::max<size_t>(bytes, 1))) return rc;
  if (!bytes) return PRB_OK;
  int peer = 0;
  if (hipDeviceCanAccessPeer(&peer, ctx->device, from) != hipSuccess) {
    (void)hipGetLastError();
    peer = 0;
  }
  if (peer) {
    PRB_HIP(hipMemcpyPeerAsync(scratch.p, ctx->device, p, from, bytes, ctx->stream));
    return PRB_OK;
  }
  ScratchPin pin;
  if (int rc = pin.ensure(bytes)) return rc;
  PRB_HIP(hipSetDevice(from));
  PRB_HIP(hipMemcpy(pin.p, p, bytes, hipMemcpyDeviceToHost));
  PRB_HIP(hipSetDevice(ctx->device));
  PRB_HIP(hipMemcpy(scratch.p, pin.p, bytes, hipMemcpyHostToDevice));
  return PRB_OK;
}
// `bytes` at p of a table of context `owner`, once that context's work is done, where ctx's device reads them: in place,
// or a copy in `scratch`
static int on_device_of(prb_ctx *ctx, const prb_ctx *owner, void *p, size_t bytes, DevBuf &scratch, void **out) {
  PRB_HIP(hipStreamSynchronize(owner->stream));
  *out = p;
  if (owner->device == ctx->device || !p) return PRB_OK;
  if (int rc = fetch_remote(ctx, owner->device, p, bytes, scratch)) return rc;
  *out = scratch.p;
  return PRB_OK;
}
// a top table back to empty, on its own device and stream
template <class Slot> static int clear_top_table(TopTable<Slot> &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, std::max<size_t>(t.slots_bytes() + (size_t)t.nq * sizeof(int32_t), 1), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  return PRB_OK;
}
// The two top tables: src's slots (and what `more` fetches) where dst's device reads them, join(slots, fill) enqueued
// in the bracket of `timer`, then src emptied.  A failure from the first launch on leaves dst unusable.
template <class T, class More, class Join>
static int merge_top_tables(const char *fn_name, const char *what, StageTimer prb_ctx::*timer, int64_t launches, prb_ctx *ctx, T *dst, T *src,
                            More more, Join join) {
  if (int rc = merge_tables_guard(fn_name, what, ctx, dst, src)) return rc;
  if (dst->n != src->n) {
    set_error(std::string(fn_name) + ": the " + what + " tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per query");
    return PRB_ERR_ARG;
  }
  DeviceScope restore;
  ScratchBuf copy;
  PRB_HIP(hipSetDevice(ctx->device));
  void *slots = nullptr;
  int rc;
  if ((rc = on_device_of(ctx, src->ctx, src->table.p, src->slots_bytes() + (size_t)src->nq * sizeof(int32_t), copy, &slots))) return rc;
  if ((rc = more())) return rc;
  dst->broken = true; // (until the merge is whole)
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = join(slots, reinterpret_cast<const int32_t *>(static_cast<char *>(slots) + src->slots_bytes())))) return rc;
  if ((rc = ctx->time_end(ctx->*timer, launches))) return rc; // (synchronises: src is read no more)
  dst->broken = false;
  move_pages(dst, src);
  return clear_top_table(*src);
}

// prb_topset_finish / prb_tophits_finish: the slots and fill counts to the host (one block: one copy, enqueued after
// `also_copy` has enqueued whatever else the table holds), then each(q, r, slot) for every slot in use, by query, then
// rank - the order of the host records
template <class Slot, class AlsoCopy, class Each>
static int download_slots(const char *fn_name, prb_ctx *ctx, const TopTable<Slot> &t, AlsoCopy also_copy, Each each) {
  const std::string fn = fn_name;
  try {
    std::vector<char> host(t.slots_bytes() + (size_t)t.nq * sizeof(int32_t));
    PRB_HIP(hipSetDevice(ctx->device));
    if (int rc = also_copy()) return rc;
    if (!host.empty()) PRB_HIP(hipMemcpyAsync(host.data(), t.table.p, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> fill((size_t)t.nq);
    std::memcpy(fill.data(), host.data() + t.slots_bytes(), fill.size() * sizeof(int32_t));
    for (int32_t q = 0; q < t.nq; q++) {
      if (fill[q] < 0 || fill[q] > t.n) {
        set_error(fn + ": query " + std::to_string(q) + " has " + std::to_string(fill[q]) + " slots in use");
        return PRB_ERR_STATE;
      }
      for (int32_t r = 0; r < fill[q]; r++) {
        Slot x;
        std::memcpy(&x, host.data() + ((size_t)q * t.n + r) * sizeof(Slot), sizeof x);
        x.rank = r;
        if (int rc = each(q, r, x)) return rc;
      }
    }
  } catch (const std::exception &e) {
    set_error(fn + ": " + e.what());
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}

extern "C" {

int prb_topset_create(prb_ctx *ctx, const prb_qbatch *qb, int32_t n, prb_topset **out) {
  return create_top_table("prb_topset_create", ctx, qb, n, out);
}

int prb_search_page_top(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_topset *ts) {
  return merge_page("prb_search_page_top", "top-N", "prb_topset_finish", SearchMode::kTop, ts, ctx, qb, db, page, opts);
}

int prb_topset_finish(prb_ctx *ctx, prb_topset *ts) {
  if (int rc = finish_guard("prb_topset_finish", "top-N", ctx, ts)) return rc;
  if (ts->finished) return PRB_OK; // (the records are on the host already)
  ts->pairs.clear();
  const int rc = download_slots(
      "prb_topset_finish", ctx, *ts, []() -> int { return PRB_OK; },
      [&](int32_t, int32_t, const prb_top_pair &p) -> int {
        ts->pairs.push_back(p);
        return PRB_OK;
      });
  if (rc) return rc;
  ts->finished = true;
  ts->table.release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int prb_topset_merge(prb_ctx *ctx, prb_topset *dst, prb_topset *src) {
  return merge_top_tables(
      "prb_topset_merge", "top-N", &prb_ctx::top_timer, 1, ctx, dst, src, []() -> int { return PRB_OK; },
      [&](const void *slots, const int32_t *fill) -> int {
        PRB_HIP(launch_top_join(dst->table.p, dst->fill(), slots, fill, dst->nq, dst->n, ctx->stream));
        return PRB_OK;
      });
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
  if (th && opts && th->style >= 0 && opts->output_style != th->style) {
    set_error("prb_search_page_tophits: the top-N hit table holds pages searched with output_style " + std::to_string(th->style) +
              " (this call: " + std::to_string(opts->output_style) + ")");
    return PRB_ERR_ARG;
  }
  const int rc = merge_page("prb_search_page_tophits", "top-N hit", "prb_tophits_finish", SearchMode::kTopHits, th, ctx, qb, db, page, opts);
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
        if (x.h.bp_offset != next || x.h.bp_count < 0) {
          set_error("prb_tophits_finish: the base pairs of query " + std::to_string(q) + ", rank " + std::to_string(r) + " are out of place");
          return PRB_ERR_STATE;
        }
        next += x.h.bp_count;
        th->hits.push_back(x);
        return PRB_OK;
      });
  if (rc) return rc;
  if (next != th->pool_pairs) {
    set_error("prb_tophits_finish: " + std::to_string(th->pool_pairs) + " base pairs in the pool, " + std::to_string(next) + " in the records");
    return PRB_ERR_STATE;
  }
  th->finished = true;
  th->release(); // (only the host copies are needed from here on)
  return PRB_OK;
}

// the records as prb_topset_merge merges them, src's lists addressed behind dst's pool; then the scan and the gather of
// prb_search_page_tophits with src's pool as the newcomers' source
int prb_tophits_merge(prb_ctx *ctx, prb_tophits *dst, prb_tophits *src) {
  if (dst && src && dst->style >= 0 && src->style >= 0 && dst->style != src->style) {
    set_error("prb_tophits_merge: the top-N hit tables hold pages searched with output_style " + std::to_string(dst->style) + " and " +
              std::to_string(src->style));
    return PRB_ERR_ARG;
  }
  ScratchBuf pool_copy;
  void *pool = nullptr;
  const int rc = merge_top_tables(
      "prb_tophits_merge", "top-N hit", &prb_ctx::tophits_timer, 4, ctx, dst, src,
      [&]() -> int { return on_device_of(ctx, src->ctx, src->pool.p, (size_t)src->pool_pairs * 8, pool_copy, &pool); },
      [&](const void *slots, const int32_t *fill) -> int {
        PRB_HIP(launch_tophits_join(dst->table.p, dst->fill(), slots, fill, dst->nq, dst->n, dst->pool_pairs, ctx->stream));
        return regather_tophits("prb_tophits_merge", ctx, dst, static_cast<const int32_t *>(pool));
      });
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

// every slot of the table back to "no hit" (the current device is the table's); its stream is idle on return
static int clear_profile_table(prb_profset &ps) {
  hipStream_t stream = ps.ctx->stream;
  const size_t P = (size_t)ps.slots();
  const prb::ProfTab t = ps.view();
  PRB_HIP(hipMemsetAsync(ps.table.p, 0, ps.bytes(), stream));
  PRB_HIP(hipMemsetAsync(t.key, 0xFF, 3 * P * 8, stream)); // key, tie, skey: none yet
  PRB_HIP(hipMemsetAsync(t.stie, 0xFF, P * 4, stream));
  PRB_HIP(hipMemcpyAsync(ps.table.p, ps.off.data(), ps.off.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipStreamSynchronize(stream));
  return PRB_OK;
}

int prb_profset_create(prb_ctx *ctx, const prb_qbatch *qb, prb_profset **out) {
  if (!ctx || !qb || !out) {
    set_error("prb_profset_create: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  std::unique_ptr<prb_profset> ps(new (std::nothrow) prb_profset());
  if (!ps) {
    set_error("prb_profset_create: out of host memory");
    return PRB_ERR_NOMEM;
  }
  ps->ctx = ctx;
  ps->qb = qb;
  ps->nq = qb->nq;
  ps->qlen = qb->len;
  ps->off.assign((size_t)qb->nq + 1, 0);
  for (int32_t q = 0; q < qb->nq; q++) ps->off[(size_t)q + 1] = ps->off[(size_t)q] + qb->len[(size_t)q] + 1;
  PRB_HIP(hipSetDevice(ctx->device));
  const size_t P = (size_t)ps->slots();
  if (ps->table.ensure(ps->bytes()) != PRB_OK) {
    set_error("prb_profset_create: can't allocate the per-position table (" + std::to_string(ps->bytes() >> 20) + " MB of HBM for " +
              std::to_string(P) + " query positions)");
    return PRB_ERR_NOMEM;
  }
  if (int rc = clear_profile_table(*ps)) return rc;
  *out = ps.release();
  return PRB_OK;
}

int prb_profset_merge(prb_ctx *ctx, prb_profset *dst, prb_profset *src) {
  if (int rc = merge_tables_guard("prb_profset_merge", "profile", ctx, dst, src)) return rc;
  DeviceScope restore;
  ScratchBuf copy;
  PRB_HIP(hipSetDevice(ctx->device));
  void *block = nullptr;
  int rc;
  if ((rc = on_device_of(ctx, src->ctx, src->table.p, src->bytes(), copy, &block))) return rc;
  dst->broken = true; // (until the merge is whole)
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_prof_join(dst->view(), dst->view_of(static_cast<char *>(block)), dst->slots(), ctx->stream));
  if ((rc = ctx->time_end(ctx->profile_timer, 1))) return rc; // (synchronises: src is read no more)
  dst->broken = false;
  move_pages(dst, src);
  PRB_HIP(hipSetDevice(src->ctx->device));
  return clear_profile_table(*src);
}

int prb_search_page_profile(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_profset *ps) {
  return merge_page("prb_search_page_profile", "profile", "prb_profset_finish", SearchMode::kProfile, ps, ctx, qb, db, page, opts);
}

// the covered positions selected on the device (Hits > 0 after the scans), their rows built there and copied once
int prb_profset_finish(prb_ctx *ctx, prb_profset *ps) {
  if (int rc = finish_guard("prb_profset_finish", "profile", ctx, ps)) return rc;
  if (ps->finished) return PRB_OK; // (the rows are on the host already)
  const size_t P = (size_t)ps->slots();
  ps->rows.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (P > 0) {
    int rc;
    if ((rc = ctx->time_begin())) return rc;
    const prb::ProfTab t = ps->view();
    // counts: hits into skey's slots, targets into stie's (the scratch is free once every page is merged)
    int64_t *hits = reinterpret_cast<int64_t *>(t.skey);
    int32_t *targets = reinterpret_cast<int32_t *>(t.stie);
    if ((rc = ps->valA.ensure(P * 4)) || (rc = ps->keyA.ensure(16))) return rc;
    // (the three share ps->sortTmp: all are sized before the first is enqueued)
    const ProfCovered covered{hits};
    auto scan_hits = [&](void *tmp, size_t &bytes) {
      return rocprim::inclusive_scan(tmp, bytes, reinterpret_cast<const int64_t *>(t.hdiff), hits, P, rocprim::plus<int64_t>(), ctx->stream);
    };
    auto scan_targets = [&](void *tmp, size_t &bytes) {
      return rocprim::inclusive_scan(tmp, bytes, t.tdiff, targets, P, rocprim::plus<int32_t>(), ctx->stream);
    };
    auto select_covered = [&](void *tmp, size_t &bytes) {
      return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), ps->valA.as<uint32_t>(), ps->keyA.as<size_t>(), P, covered,
                             ctx->stream);
    };
    size_t tmp_h = 0, tmp_t = 0, tmp_s = 0;
    PRB_HIP(scan_hits(nullptr, tmp_h));
    PRB_HIP(scan_targets(nullptr, tmp_t));
    PRB_HIP(select_covered(nullptr, tmp_s));
    if ((rc = ps->sortTmp.ensure(std::max<size_t>({tmp_h, tmp_t, tmp_s, 1})))) return rc;
    PRB_HIP(scan_hits(ps->sortTmp.p, tmp_h));
    PRB_HIP(scan_targets(ps->sortTmp.p, tmp_t));
    PRB_HIP(select_covered(ps->sortTmp.p, tmp_s));
    size_t nsel = 0;
    uint32_t bad = 0;
    PRB_HIP(hipMemcpyAsync(&nsel, ps->keyA.p, sizeof nsel, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipMemcpyAsync(&bad, t.bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    if (bad || nsel > P) {
      set_error("prb_profset_finish: " + std::string(bad ? "a final hit's span lies outside its query" : "bad row count"));
      return PRB_ERR_STATE;
    }
    if (nsel) {
      try {
        ps->rows.resize(nsel);
      } catch (const std::exception &e) {
        set_error(std::string("prb_profset_finish: ") + e.what());
        return PRB_ERR_NOMEM;
      }
      if ((rc = ps->span.ensure(nsel * sizeof(prb_profile_pos)))) return rc;
      PRB_HIP(launch_prof_rows(t, ps->valA.as<uint32_t>(), (int64_t)nsel, hits, targets, ps->span.p, ctx->stream));
      PRB_HIP(hipMemcpyAsync(ps->rows.data(), ps->span.p, nsel * sizeof(prb_profile_pos), hipMemcpyDeviceToHost, ctx->stream));
      PRB_HIP(hipStreamSynchronize(ctx->stream));
    }
    if ((rc = ctx->time_end(ctx->profile_timer, nsel ? 4 : 3))) return rc;
  }
  ps->finished = true;
  ps->release(); // (only the host rows are needed from here on)
  return PRB_OK;
}

int64_t prb_profset_size(const prb_profset *ps) { return ps ? (int64_t)ps->rows.size() : -1; }
const prb_profile_pos *prb_profset_rows(const prb_profset *ps) { return ps ? ps->rows.data() : nullptr; }
void prb_profset_counts(const prb_profset *ps, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ps ? ps->counts[i] : 0;
}
void prb_profset_free(prb_profset *ps) {
  delete ps;
}

// ---- the per-target table (prb_targetset_*) ----
// every key, payload slot and fill count of the table back to "nothing", on its own device and stream
static int clear_target_table(prb_targetset &t) {
  PRB_HIP(hipSetDevice(t.ctx->device));
  PRB_HIP(hipMemsetAsync(t.table.p, 0, t.bytes(), t.ctx->stream));
  PRB_HIP(hipStreamSynchronize(t.ctx->stream));
  return PRB_OK;
}

int prb_targetset_create(prb_ctx *ctx, prb_db *db, int32_t n, prb_targetset **out) {
  if (!ctx || !db || !out || db->ctx->device != ctx->device) {
    set_error("prb_targetset_create: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  if (n < 1 || n > kTopMaxN) {
    set_error("prb_targetset_create: need 1 <= n <= " + std::to_string(kTopMaxN) + " (got " + std::to_string(n) + ")");
    return PRB_ERR_ARG;
  }
  std::unique_ptr<prb_targetset> t(new (std::nothrow) prb_targetset());
  if (!t) {
    set_error("prb_targetset_create: out of host memory");
    return PRB_ERR_NOMEM;
  }
  t->ctx = ctx;
  t->db = db;
  t->n = n;
  t->tbase.assign(db->pages.size() + 1, 0);
  for (size_t p = 0; p < db->pages.size(); p++) t->tbase[p + 1] = t->tbase[p] + db->pages[p].nseq;
  t->merged.resize(db->pages.size());
  PRB_HIP(hipSetDevice(ctx->device));
  if (t->table.ensure(t->bytes()) != PRB_OK) {
    set_error("prb_targetset_create: can't allocate the per-target table (" + std::to_string(t->bytes() >> 20) + " MB of HBM for " +
              std::to_string(t->targets()) + " targets of " + std::to_string(n) + " slots)");
    return PRB_ERR_NOMEM;
  }
  if (int rc = clear_target_table(*t)) return rc;
  *out = t.release();
  return PRB_OK;
}

// prb_search_page_targets / prb_search_page_coverage / prb_covset_add_hits: what is checked of the run table `t` - `what`
// in the messages, finished by `finish_fn` - before a batch of nq queries named query_ids is merged into it for `page`
// (distinct < 0: the call has no options).  Every check comes before the table is touched: a refused call leaves it as
// it was; a call that passes has its identifiers marked as merged.
static int run_table_guard(const std::string &fn, const char *what, const char *finish_fn, RunTable *t, const prb_ctx *ctx, const prb_db *db,
                           int32_t page, int32_t distinct, const int32_t *query_ids, int32_t nq) {
  const std::string table = std::string(what) + " table";
  auto refuse = [&](const std::string &why, int code = PRB_ERR_ARG) {
    set_error(fn + ": " + why);
    return code;
  };
  if (t->ctx != ctx || t->db != db) return refuse("the " + table + " was made with another context or for another database");
  if (t->broken) return refuse("an earlier merge into this " + table + " failed", PRB_ERR_STATE);
  if (t->finished) return refuse("the " + table + " is finished (" + finish_fn + ")", PRB_ERR_STATE);
  if (t->distinct >= 0 && distinct >= 0 && distinct != t->distinct)
    return refuse("the " + table + " holds pages searched with distinct_sites " + std::to_string(t->distinct) + " (this call: " +
                  std::to_string(distinct) + ")");
  try {
    std::vector<int32_t> sorted(query_ids, query_ids + nq);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size(); i++) {
      if (sorted[i] < 0) return refuse("query identifier " + std::to_string(sorted[i]) + " is below 0");
      if (i && sorted[i] == sorted[i - 1]) return refuse("query identifier " + std::to_string(sorted[i]) + " is given twice");
      if (t->has((size_t)page, sorted[i]))
        return refuse("query identifier " + std::to_string(sorted[i]) + " is already merged for page " + std::to_string(page));
    }
    for (int32_t id : sorted) t->set((size_t)page, id);
  } catch (const std::exception &e) {
    return refuse(e.what(), PRB_ERR_NOMEM);
  }
  return PRB_OK;
}
// the identifiers of the batch being merged into t, on the device (the current one)
static int upload_ids(prb_ctx *ctx, RunTable *t, const int32_t *query_ids, int32_t nq) {
  if (int rc = t->ids.ensure(std::max<size_t>((size_t)nq * 4, 4))) return rc;
  PRB_HIP(hipMemcpyAsync(t->ids.p, query_ids, (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  return PRB_OK;
}

int prb_search_page_targets(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *query_ids,
                            prb_targetset *ts) {
  const std::string fn = "prb_search_page_targets";
  if (!ts || !query_ids) {
    set_error(fn + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (int rc = check_search_args(fn.c_str(), ctx, qb, db, page, opts, 3)) return rc;
  if (int rc = run_table_guard(fn, "per-target", "prb_targetset_finish", ts, ctx, db, page, opts->distinct_sites, query_ids, qb->nq)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  ts->broken = true; // (until the merge is whole)
  int rc;
  if ((rc = upload_ids(ctx, ts, query_ids, qb->nq))) return rc;
  prb_hitset *hs = nullptr;
  if ((rc = search_page(ctx, qb, db, page, opts, 3, SearchMode::kTargets, &hs, ts))) return rc;
  for (int i = 0; i < 3; i++) ts->counts[i] += hs->counts[i];
  ts->distinct = opts->distinct_sites;
  ts->broken = false;
  delete hs;
  return PRB_OK;
}

// prb_targetset_merge / prb_covset_merge: what is checked before either run table - `what` in the messages - is touched;
// `more` (may be empty) = a refusal of the caller's own, or "", asked once both are known to be whole and unfinished
static int run_tables_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const RunTable *dst, const RunTable *src,
                            const std::function<std::string()> &more) {
  const std::string tables = std::string(what) + " tables";
  auto refuse = [&](const std::string &why) {
    set_error(std::string(fn_name) + ": " + why);
    return PRB_ERR_ARG;
  };
  if (!ctx || !dst || !src || dst == src) return refuse("bad argument");
  if (dst->ctx != ctx) return refuse("the table to merge into belongs to another context");
  if (dst->broken || src->broken) return refuse("an earlier merge into one of the " + tables + " failed");
  if (dst->finished || src->finished) return refuse("one of the " + tables + " is finished");
  if (more)
    if (const std::string why = more(); !why.empty()) return refuse(why);
  if (dst->tbase != src->tbase) return refuse("the " + tables + " were made for different databases");
  if (dst->distinct >= 0 && src->distinct >= 0 && dst->distinct != src->distinct)
    return refuse("the " + tables + " hold pages searched with distinct_sites " + std::to_string(dst->distinct) + " and " +
                  std::to_string(src->distinct));
  for (size_t p = 0; p < dst->merged.size(); p++) {
    const std::vector<uint64_t> &a = dst->merged[p], &b = src->merged[p];
    for (size_t k = 0; k < std::min(a.size(), b.size()); k++)
      if (a[k] & b[k]) return refuse("a query identifier is merged for page " + std::to_string(p) + " into both " + tables);
  }
  return PRB_OK;
}
// after the merge: dst's identifier sets are the unions and its counts the sums; src has merged nothing
static int move_ids(const char *fn_name, RunTable *dst, RunTable *src) {
  try {
    for (size_t p = 0; p < dst->merged.size(); p++) {
      std::vector<uint64_t> &a = dst->merged[p], &b = src->merged[p];
      if (a.size() < b.size()) a.resize(b.size(), 0);
      for (size_t k = 0; k < b.size(); k++) a[k] |= b[k];
      b.clear();
    }
  } catch (const std::exception &e) {
    dst->broken = true;
    set_error(std::string(fn_name) + ": " + e.what());
    return PRB_ERR_NOMEM;
  }
  for (int i = 0; i < 3; i++) {
    dst->counts[i] += src->counts[i];
    src->counts[i] = 0;
  }
  if (dst->distinct < 0) dst->distinct = src->distinct;
  src->distinct = -1;
  return PRB_OK;
}

int prb_targetset_merge(prb_ctx *ctx, prb_targetset *dst, prb_targetset *src) {
  if (int rc = run_tables_guard("prb_targetset_merge", "per-target", ctx, dst, src, [&]() -> std::string {
        if (dst->n == src->n) return "";
        return "the per-target tables keep " + std::to_string(dst->n) + " and " + std::to_string(src->n) + " records per target";
      }))
    return rc;
  DeviceScope restore;
  ScratchBuf copy;
  PRB_HIP(hipSetDevice(ctx->device));
  void *block = nullptr;
  int rc;
  if ((rc = on_device_of(ctx, src->ctx, src->table.p, src->bytes(), copy, &block))) return rc;
  dst->broken = true; // (until the merge is whole)
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_target_join(dst->keys_of(dst->table.p), dst->slots_of(dst->table.p), dst->fill_of(dst->table.p), dst->keys_of(block),
                             dst->slots_of(block), dst->fill_of(block), dst->targets(), dst->n, ctx->stream));
  if ((rc = ctx->time_end(ctx->targets_timer, 1))) return rc; // (synchronises: src is read no more)
  dst->broken = false;
  if ((rc = move_ids("prb_targetset_merge", dst, src))) return rc;
  return clear_target_table(*src);
}

// the fills scanned, the filled slots gathered by target and rank on the device, one copy
int prb_targetset_finish(prb_ctx *ctx, prb_targetset *ts) {
  if (!ctx || !ts || ts->ctx != ctx) {
    set_error("prb_targetset_finish: bad argument (the table belongs to another context)");
    return PRB_ERR_ARG;
  }
  if (ts->broken) {
    set_error("prb_targetset_finish: an earlier merge into this per-target table failed");
    return PRB_ERR_STATE;
  }
  if (ts->finished) return PRB_OK; // (the records are on the host already)
  ts->pairs.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  const int64_t T = ts->targets();
  if (T > 0) {
    int rc;
    ScratchBuf off, out, tmp;
    if ((rc = off.ensure(((size_t)T + 1) * 8))) return rc;
    auto fills = rocprim::make_transform_iterator(ts->fill_of(ts->table.p), FillToI64());
    if ((rc = with_temp(tmp, "rocprim::exclusive_scan", [&](void *t, size_t &b) {
           return rocprim::exclusive_scan(t, b, fills, off.as<int64_t>(), (int64_t)0, (size_t)T + 1, rocprim::plus<int64_t>(), ctx->stream);
         })))
      return rc;
    int64_t total = 0;
    PRB_HIP(hipMemcpyAsync(&total, off.as<int64_t>() + T, 8, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    if (total < 0 || (uint64_t)total > (uint64_t)ts->entries()) {
      set_error("prb_targetset_finish: bad record count " + std::to_string(total));
      return PRB_ERR_STATE;
    }
    if (total) {
      try {
        ts->pairs.resize((size_t)total);
      } catch (const std::exception &e) {
        set_error(std::string("prb_targetset_finish: ") + e.what());
        return PRB_ERR_NOMEM;
      }
      if ((rc = out.ensure((size_t)total * sizeof(prb_target_pair)))) return rc;
      PRB_HIP(launch_target_gather(ts->keys_of(ts->table.p), ts->slots_of(ts->table.p), off.as<int64_t>(), T, ts->n, total, out.p, ctx->stream));
      PRB_HIP(hipMemcpyAsync(ts->pairs.data(), out.p, (size_t)total * sizeof(prb_target_pair), hipMemcpyDeviceToHost, ctx->stream));
      PRB_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
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

// ---- the per-target coverage table (prb_covset_*) ----
// every slot of the table back to "no hit", on its own device and stream; its stream is idle on return
static int clear_coverage_table(prb_covset &cs) {
  hipStream_t stream = cs.ctx->stream;
  const size_t P = (size_t)cs.slots();
  const prb::CovTab t = cs.view();
  PRB_HIP(hipSetDevice(cs.ctx->device));
  PRB_HIP(hipMemsetAsync(cs.table.p, 0, cs.bytes(), stream));
  if (P) PRB_HIP(hipMemsetAsync(t.key, 0xFF, 4 * P * 8, stream)); // key, tie, skey, stie: none yet
  PRB_HIP(hipMemcpyAsync(cs.table.p, cs.seq_lo.data(), cs.seq_lo.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipMemcpyAsync(cs.table.as<int64_t>() + cs.seq_lo.size(), cs.tbase.data(), cs.tbase.size() * 8, hipMemcpyHostToDevice, stream));
  PRB_HIP(hipStreamSynchronize(stream));
  return PRB_OK;
}

int prb_covset_create(prb_ctx *ctx, prb_db *db, prb_covset **out) {
  if (!ctx || !db || !out || db->ctx->device != ctx->device) {
    set_error("prb_covset_create: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  std::unique_ptr<prb_covset> cs(new (std::nothrow) prb_covset());
  if (!cs) {
    set_error("prb_covset_create: out of host memory");
    return PRB_ERR_NOMEM;
  }
  cs->ctx = ctx;
  cs->db = db;
  try {
    cs->tbase.assign(db->pages.size() + 1, 0);
    cs->slot0.assign(db->pages.size() + 1, 0);
    for (size_t p = 0; p < db->pages.size(); p++) {
      const DbPage &pg = db->pages[p];
      cs->tbase[p + 1] = cs->tbase[p] + pg.nseq;
      for (int32_t i = 0; i < pg.nseq; i++) cs->seq_lo.push_back(cs->slot0[p] + pg.start_pos[(size_t)i]);
      cs->slot0[p + 1] = cs->slot0[p] + (int64_t)pg.seqs.size(); // (the text: every sequence and the separator behind it)
    }
    cs->seq_lo.push_back(cs->slot0.back());
    cs->merged.resize(db->pages.size());
  } catch (const std::exception &e) {
    set_error(std::string("prb_covset_create: ") + e.what());
    return PRB_ERR_NOMEM;
  }
  if (cs->slots() > (int64_t)UINT32_MAX) {
    set_error("prb_covset_create: the database has " + std::to_string(cs->slots()) + " positions (at most 2^32 - 1)");
    return PRB_ERR_ARG;
  }
  PRB_HIP(hipSetDevice(ctx->device));
  if (cs->table.ensure(cs->bytes()) != PRB_OK) {
    set_error("prb_covset_create: can't allocate the coverage table (" + std::to_string(cs->bytes() >> 20) + " MB of HBM for " +
              std::to_string(cs->slots()) + " positions of " + std::to_string(cs->targets()) + " targets)");
    return PRB_ERR_NOMEM;
  }
  if (int rc = clear_coverage_table(*cs)) return rc;
  *out = cs.release();
  return PRB_OK;
}

int prb_search_page_coverage(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *query_ids,
                             prb_covset *cs) {
  const std::string fn = "prb_search_page_coverage";
  if (!cs || !query_ids) {
    set_error(fn + ": bad argument");
    return PRB_ERR_ARG;
  }
  if (int rc = check_search_args(fn.c_str(), ctx, qb, db, page, opts, 3)) return rc;
  if (int rc = run_table_guard(fn, "coverage", "prb_covset_finish", cs, ctx, db, page, opts->distinct_sites, query_ids, qb->nq)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  cs->broken = true; // (until the merge is whole)
  int rc;
  if ((rc = upload_ids(ctx, cs, query_ids, qb->nq))) return rc;
  prb_hitset *hs = nullptr;
  if ((rc = search_page(ctx, qb, db, page, opts, 3, SearchMode::kCoverage, &hs, cs))) return rc;
  for (int i = 0; i < 3; i++) cs->counts[i] += hs->counts[i];
  cs->distinct = opts->distinct_sites;
  cs->broken = false;
  delete hs;
  return PRB_OK;
}

// the caller's list checked on the host - a refused call leaves the table as it was -, then as columns to the device and
// through the merge of a sub-batch
int prb_covset_add_hits(prb_ctx *ctx, prb_covset *cs, int32_t page, const int32_t *query_ids, int32_t nq, const prb_hit *hits, int64_t nhits,
                        const int32_t *basepairs, int64_t npairs) {
  const std::string fn = "prb_covset_add_hits";
  auto refuse = [&](const std::string &why, int code = PRB_ERR_ARG) {
    set_error(fn + ": " + why);
    return code;
  };
  if (!ctx || !cs || nq < 0 || (nq && !query_ids) || nhits < 0 || nhits > INT32_MAX || npairs < 0 || (nhits && (!hits || !basepairs)))
    return refuse("bad argument");
  if (page < 0 || (size_t)page >= cs->merged.size()) return refuse("page " + std::to_string(page) + " out of range");
  const prb::CovPage pg = cs->page_view((size_t)page);
  std::vector<int32_t> query, db_id, ends;
  std::vector<double> e_tot;
  try {
    query.resize((size_t)nhits);
    db_id.resize((size_t)nhits);
    e_tot.resize((size_t)nhits);
    ends.resize((size_t)nhits * 4);
  } catch (const std::exception &e) {
    return refuse(e.what(), PRB_ERR_NOMEM);
  }
  for (int64_t i = 0; i < nhits; i++) {
    const prb_hit &x = hits[i];
    if (x.query < 0 || x.query >= nq || (i && x.query < hits[i - 1].query) || x.db_id < 0 || x.db_id >= pg.nseq || x.bp_count < 1 ||
        x.bp_offset < 0 || x.bp_offset + x.bp_count > npairs)
      return refuse("hit record " + std::to_string(i) + " is inconsistent");
    const int32_t *first = basepairs + 2 * x.bp_offset, *last = basepairs + 2 * (x.bp_offset + x.bp_count - 1);
    const int64_t lo = std::min(first[1], last[1]), hi = std::max(first[1], last[1]);
    const int64_t s0 = cs->seq_lo[(size_t)(pg.target0 + x.db_id)] - pg.slot0, sep = cs->seq_lo[(size_t)(pg.target0 + x.db_id) + 1] - pg.slot0 - 1;
    if (lo < s0 || hi >= sep) return refuse("the span of hit record " + std::to_string(i) + " leaves its sequence", PRB_ERR_STATE);
    query[(size_t)i] = x.query;
    db_id[(size_t)i] = x.db_id;
    e_tot[(size_t)i] = x.e_tot;
    ends[4 * (size_t)i] = first[0], ends[4 * (size_t)i + 1] = first[1], ends[4 * (size_t)i + 2] = last[0], ends[4 * (size_t)i + 3] = last[1];
  }
  if (int rc = run_table_guard(fn, "coverage", "prb_covset_finish", cs, ctx, cs->db, page, -1, query_ids, nq)) return rc;
  if (!nhits) return PRB_OK;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  cs->broken = true; // (until the merge is whole)
  int rc;
  const size_t N = (size_t)nhits;
  if ((rc = upload_ids(ctx, cs, query_ids, nq))) return rc;
  if ((rc = cs->h_query.ensure(N * 4)) || (rc = cs->h_db_id.ensure(N * 4)) || (rc = cs->h_e_tot.ensure(N * 8)) || (rc = cs->h_ends.ensure(N * 16)))
    return rc;
  PRB_HIP(hipMemcpyAsync(cs->h_query.p, query.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_db_id.p, db_id.data(), N * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_e_tot.p, e_tot.data(), N * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(cs->h_ends.p, ends.data(), N * 16, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the vectors go)
  if ((rc = merge_coverage(ctx, cs, page, prb::CovHits{nhits, cs->h_query.as<int32_t>(), cs->h_db_id.as<int32_t>(), cs->h_e_tot.as<double>(),
                                                      cs->h_ends.as<int32_t>()},
                           nq)))
    return rc;
  cs->broken = false;
  return PRB_OK;
}

int prb_covset_merge(prb_ctx *ctx, prb_covset *dst, prb_covset *src) {
  if (int rc = run_tables_guard("prb_covset_merge", "coverage", ctx, dst, src, [&]() -> std::string {
        return dst->seq_lo == src->seq_lo ? "" : "the coverage tables were made for different databases";
      }))
    return rc;
  DeviceScope restore;
  ScratchBuf copy;
  PRB_HIP(hipSetDevice(ctx->device));
  void *block = nullptr;
  int rc;
  if ((rc = on_device_of(ctx, src->ctx, src->table.p, src->bytes(), copy, &block))) return rc;
  dst->broken = true; // (until the merge is whole)
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_cov_join(dst->view(), dst->view_of(static_cast<char *>(block)), dst->slots(), ctx->stream));
  if ((rc = ctx->time_end(ctx->coverage_timer, 1))) return rc; // (synchronises: src is read no more)
  dst->broken = false;
  if ((rc = move_ids("prb_covset_merge", dst, src))) return rc;
  return clear_coverage_table(*src);
}

// the counts scanned into the scratch columns, the regions' first slots selected, a wavefront per region, one copy
int prb_covset_finish(prb_ctx *ctx, prb_covset *cs, int32_t min_queries) {
  if (!ctx || !cs || cs->ctx != ctx) {
    set_error("prb_covset_finish: bad argument (the table belongs to another context)");
    return PRB_ERR_ARG;
  }
  if (cs->broken) {
    set_error("prb_covset_finish: an earlier merge into this coverage table failed");
    return PRB_ERR_STATE;
  }
  if (cs->finished) return PRB_OK; // (the records are on the host already)
  if (min_queries < 1 || min_queries > 1000000) {
    set_error("prb_covset_finish: need 1 <= min_queries <= 1000000 (got " + std::to_string(min_queries) + ")");
    return PRB_ERR_ARG;
  }
  const size_t P = (size_t)cs->slots();
  cs->regions.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  if (P > 0) {
    int rc;
    if ((rc = ctx->time_begin())) return rc;
    const prb::CovTab t = cs->view();
    // the scratch is free once everything is merged: hits into skey's slots, queries into the first half of stie's, the
    // regions' first slots (at most one for two slots) into the second half
    int64_t *hits = reinterpret_cast<int64_t *>(t.skey);
    int32_t *queries = reinterpret_cast<int32_t *>(t.stie);
    uint32_t *first = reinterpret_cast<uint32_t *>(t.stie) + P;
    if ((rc = cs->keyA.ensure(16))) return rc;
    // (the three share cs->sortTmp: all are sized before the first is enqueued)
    const CovHead head{queries, min_queries};
    auto scan_hits = [&](void *tmp, size_t &bytes) {
      return rocprim::inclusive_scan(tmp, bytes, reinterpret_cast<const int64_t *>(t.hdiff), hits, P, rocprim::plus<int64_t>(), ctx->stream);
    };
    auto scan_queries = [&](void *tmp, size_t &bytes) {
      return rocprim::inclusive_scan(tmp, bytes, t.qdiff, queries, P, rocprim::plus<int32_t>(), ctx->stream);
    };
    auto select_heads = [&](void *tmp, size_t &bytes) {
      return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), first, cs->keyA.as<size_t>(), P, head, ctx->stream);
    };
    size_t tmp_h = 0, tmp_q = 0, tmp_s = 0;
    PRB_HIP(scan_hits(nullptr, tmp_h));
    PRB_HIP(scan_queries(nullptr, tmp_q));
    PRB_HIP(select_heads(nullptr, tmp_s));
    if ((rc = cs->sortTmp.ensure(std::max<size_t>({tmp_h, tmp_q, tmp_s, 1})))) return rc;
    PRB_HIP(scan_hits(cs->sortTmp.p, tmp_h));
    PRB_HIP(scan_queries(cs->sortTmp.p, tmp_q));
    PRB_HIP(select_heads(cs->sortTmp.p, tmp_s));
    size_t nreg = 0;
    uint32_t bad = 0;
    PRB_HIP(hipMemcpyAsync(&nreg, cs->keyA.p, sizeof nreg, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipMemcpyAsync(&bad, t.bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    if (bad || nreg > (P + 1) / 2) {
      set_error("prb_covset_finish: " + std::string(bad ? "a final hit's span leaves its sequence" : "bad region count"));
      return PRB_ERR_STATE;
    }
    if (nreg) {
      try {
        cs->regions.resize(nreg);
      } catch (const std::exception &e) {
        set_error(std::string("prb_covset_finish: ") + e.what());
        return PRB_ERR_NOMEM;
      }
      if ((rc = cs->span.ensure(nreg * sizeof(prb_target_region)))) return rc;
      PRB_HIP(launch_cov_regions(t, cs->tbase_dev(), (int32_t)cs->merged.size(), cs->targets(), first, (int64_t)nreg, hits, queries, min_queries,
                                 cs->span.p, ctx->stream));
      PRB_HIP(hipMemcpyAsync(cs->regions.data(), cs->span.p, nreg * sizeof(prb_target_region), hipMemcpyDeviceToHost, ctx->stream));
      PRB_HIP(hipStreamSynchronize(ctx->stream));
      // (the slots run along the page's text, which holds the sequences reversed: a target's regions arrive by start
      // descending)
      for (size_t i = 0, j; i < nreg; i = j) {
        for (j = i + 1; j < nreg && cs->regions[j].page == cs->regions[i].page && cs->regions[j].db_id == cs->regions[i].db_id;) j++;
        std::reverse(cs->regions.begin() + (ptrdiff_t)i, cs->regions.begin() + (ptrdiff_t)j);
      }
    }
    if ((rc = ctx->time_end(ctx->coverage_timer, nreg ? 4 : 3))) return rc;
  }
  cs->finished = true;
  cs->release(); // (only the host records are needed from here on)
  return PRB_OK;
}

int64_t prb_covset_size(const prb_covset *cs) { return cs ? (int64_t)cs->regions.size() : -1; }
const prb_target_region *prb_covset_regions(const prb_covset *cs) { return cs ? cs->regions.data() : nullptr; }
void prb_covset_counts(const prb_covset *cs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = cs ? cs->counts[i] : 0;
}
void prb_covset_free(prb_covset *cs) {
  delete cs;
}

int64_t prb_pairset_size(const prb_pairset *ps) { return ps ? (int64_t)ps->pairs.size() : -1; }
const prb_pair_summary *prb_pairset_pairs(const prb_pairset *ps) { return ps ? ps->pairs.data() : nullptr; }
void prb_pairset_counts(const prb_pairset *ps, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = ps ? ps->counts[i] : 0;
}
void prb_pairset_free(prb_pairset *ps) { delete ps; }

int64_t prb_hitset_size(const prb_hitset *hs) { return !hs ? -1 : hs->ext_hits ? hs->ext_nhits : (int64_t)hs->hits.size(); }
const prb_hit *prb_hitset_hits(const prb_hitset *hs) { return !hs ? nullptr : hs->ext_hits ? hs->ext_hits : hs->hits.data(); }
const int32_t *prb_hitset_basepairs(const prb_hitset *hs, int64_t *count) {
  if (!hs) return nullptr;
  if (count) *count = (hs->ext_hits ? hs->ext_bp_ints : (int64_t)hs->bp.size()) / 2;
  return hs->ext_hits ? hs->ext_bp : hs->bp.data();
}
void prb_hitset_counts(const prb_hitset *hs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = hs ? hs->counts[i] : 0;
}
void prb_hitset_free(prb_hitset *hs) { delete hs; }

} // extern "C"
