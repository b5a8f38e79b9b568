// The protocol of the thirteen result tables, each step once (capi_top.hip, capi_targets.hip, capi_spans.hip, capi_null.hip,
// capi_groups.hip, capi_grouprank.hip, capi_gnull.hip, capi_eval.hip, capi_features.hip, capi_fnull.hip, capi_featrank.hip): what a prb_*_create starts with, what is checked before a page, a
// caller's list, a batch of decoys or another table is merged, the search of a page into a table, the uploads of a
// caller's arrays, the device's `bad` flag, the merge of one table into another across contexts and devices, and what
// every prb_*_finish starts with.  `fn_name` is the entry point and `what` the table's noun in the messages.  Every check
// comes before a table is touched: a refused call leaves it as it was.  The per-table files keep what is theirs alone:
// their own state checks, their kernels' launches and their create and finish.  What the three ranked run tables share
// beyond this - their merges and their finish - is in capi_ranked.hpp.
#pragma once
#include <algorithm>
#include <string>

#include "search_host.hpp"

namespace prb {

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

inline int refuse(const std::string &fn, const std::string &why, int code = PRB_ERR_ARG) {
  set_error(fn + ": " + why);
  return code;
}

// ---- prb_*_create
// What the create functions start with (args_ok: the caller's test of its other arguments): *out = nullptr, the
// caller's own refusal if it has one (bad_n), and an empty table in `t`
template <class T> int new_table(const char *fn_name, bool args_ok, T **out, std::unique_ptr<T> &t, const std::string &why = "") {
  if (!args_ok || !out) return refuse(fn_name, "bad argument");
  *out = nullptr;
  if (!why.empty()) return refuse(fn_name, why);
  t.reset(new (std::nothrow) T());
  if (!t) return refuse(fn_name, "out of host memory", PRB_ERR_NOMEM);
  return PRB_OK;
}
// the refusal of a number of slots per query or target that no table takes ("": n is fine)
inline std::string bad_n(int32_t n) {
  return n < 1 || n > kTopMaxN ? "need 1 <= n <= " + std::to_string(kTopMaxN) + " (got " + std::to_string(n) + ")" : "";
}

// ---- prb_*_finish
// What every prb_*_finish starts with: the table belongs to ctx and no merge into it failed
inline int finish_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const TableState *t) {
  if (!ctx || !t || t->ctx != ctx) return refuse(fn_name, "bad argument (the table belongs to another context)");
  if (t->broken) return refuse(fn_name, std::string("an earlier merge into this ") + what + " table failed", PRB_ERR_STATE);
  return PRB_OK;
}

// ---- one selection per table
// A table holds pages of one selection: why pages searched with (distinct_sites, chain_sites) = (distinct, chain) do
// not go with the ones `t` holds, or "" (a value below 0: none yet, or the call has no options).  The message names the
// field; `holds` = "holds" or "hold", other_open / other_close = what stands around the second value.
inline std::string selection_clash(const std::string &tables, const char *holds, const TableState *t, int32_t distinct, int32_t chain,
                                   const char *other_open, const char *other_close) {
  if (t->distinct >= 0 && distinct >= 0 && distinct != t->distinct)
    return "the " + tables + " " + holds + " pages searched with distinct_sites " + std::to_string(t->distinct) + other_open +
           std::to_string(distinct) + other_close;
  if (t->chain >= 0 && chain >= 0 && chain != t->chain)
    return "the " + tables + " " + holds + " pages searched with chain_sites " + std::to_string(t->chain) + other_open + std::to_string(chain) +
           other_close;
  return "";
}

// the options of a page search against the selection of the table it goes into (`table`: "null table", "evalset", ...)
inline int selection_guard(const std::string &fn, const char *table, const TableState *t, const prb_ris_opts *opts) {
  if (const std::string why = selection_clash(table, "holds", t, opts->distinct_sites, opts->chain_sites, " (this call: ", ")"); !why.empty())
    return refuse(fn, why);
  return PRB_OK;
}
// opts->allowed_pairs belongs to this search (what search_page would refuse only once the call is under way)
inline int mask_guard(const std::string &fn, const prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, const prb_ris_opts *opts) {
  const prb_pairmask *pm = opts->allowed_pairs;
  if (pm && (pm->qb != qb || pm->db != db || pm->nq != qb->nq || pm->tbase.size() != db->pages.size() + 1 || pm->ctx->device != ctx->device))
    return refuse(fn, "allowed_pairs was made for another query batch, another database or on another device");
  return PRB_OK;
}

// ---- every prb_search_page_* of a table, behind its guards
// Page `page` searched with every sub-batch's final hits taken by `t` (TableState::take), the three stage counts of the
// search added to `counts` (t->counts, or the table's other set), and - unless the batch is not the table's own
// (record_selection = false: the null table's decoys) - the options' selection recorded as the table's
inline int search_into_table(TableState *t, prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, int64_t counts[3],
                             bool record_selection = true) {
  prb_hitset *hs = nullptr;
  if (int rc = search_page(ctx, qb, db, page, opts, 3, SearchMode::kTable, &hs, t)) return rc;
  for (int i = 0; i < 3; i++) counts[i] += hs->counts[i];
  if (record_selection) {
    t->distinct = opts->distinct_sites;
    t->chain = opts->chain_sites;
  }
  delete hs;
  return PRB_OK;
}

// ---- prb_search_page_top / _profile / _tophits / _groups: a page searched and merged into a batch table
// What is checked of the table `t`, finished by `finish_fn`, before `page` is searched and merged into it; a call that
// passes has the page marked as merged (also prb_search_page_scored, which searches the page into its evalset and hands
// the sub-batches on to `t`)
inline int merge_page_guard(const char *fn_name, const char *what, const char *finish_fn, MergeTable *t, prb_ctx *ctx, prb_qbatch *qb, prb_db *db,
                            int32_t page, const prb_ris_opts *opts) {
  const std::string fn = fn_name, table = std::string(what) + " table";
  if (!t) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn_name, ctx, qb, db, page, opts, 3)) return rc;
  if (t->ctx != ctx || t->qb != qb || t->nq != qb->nq)
    return refuse(fn, "the " + table + " was made for another context or query batch (" + std::to_string(t->nq) + " queries; this batch has " +
                          std::to_string(qb->nq) + ")");
  if (t->db && t->db != db) return refuse(fn, "the " + table + " holds pages of another database");
  if (t->broken) return refuse(fn, "an earlier merge into this " + table + " failed", PRB_ERR_STATE);
  if (t->finished) return refuse(fn, "the " + table + " is finished (" + finish_fn + ")", PRB_ERR_STATE);
  if (const std::string why = selection_clash(table, "holds", t, opts->distinct_sites, opts->chain_sites, " (this call: ", ")"); !why.empty())
    return refuse(fn, why);
  if (!t->db) {
    t->db = db;
    t->merged.assign(db->pages.size(), 0);
  }
  if (t->merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged into this " + table);
  t->merged[(size_t)page] = 1;
  return PRB_OK;
}
// Page `page` searched and merged into the table `t`, finished by `finish_fn`
inline int merge_page(const char *fn_name, const char *what, const char *finish_fn, MergeTable *t, prb_ctx *ctx, prb_qbatch *qb, prb_db *db,
                      int32_t page, const prb_ris_opts *opts) {
  if (int rc = merge_page_guard(fn_name, what, finish_fn, t, ctx, qb, db, page, opts)) return rc;
  const int rc = search_into_table(t, ctx, qb, db, page, opts, t->counts);
  if (rc != PRB_OK) t->broken = true;
  return rc;
}

// ---- prb_search_page_targets / _coverage / prb_covset_add_hits: a batch merged into a run table
// What is checked of the run table `t`, finished by `finish_fn`, before a batch of nq queries named query_ids is merged
// into it for `page` (distinct, chain < 0: the call has no options).  A call that passes has its identifiers marked as merged.
inline int run_table_guard(const std::string &fn, const char *what, const char *finish_fn, RunTable *t, const prb_ctx *ctx, const prb_db *db,
                           int32_t page, int32_t distinct, int32_t chain, const int32_t *query_ids, int32_t nq) {
  const std::string table = std::string(what) + " table";
  if (t->ctx != ctx || t->db != db) return refuse(fn, "the " + table + " was made with another context or for another database");
  if (t->broken) return refuse(fn, "an earlier merge into this " + table + " failed", PRB_ERR_STATE);
  if (t->finished) return refuse(fn, "the " + table + " is finished (" + finish_fn + ")", PRB_ERR_STATE);
  if (const std::string why = selection_clash(table, "holds", t, distinct, chain, " (this call: ", ")"); !why.empty()) return refuse(fn, why);
  try {
    std::vector<int32_t> sorted(query_ids, query_ids + nq);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size(); i++) {
      if (sorted[i] < 0) return refuse(fn, "query identifier " + std::to_string(sorted[i]) + " is below 0");
      if (i && sorted[i] == sorted[i - 1]) return refuse(fn, "query identifier " + std::to_string(sorted[i]) + " is given twice");
      if (t->has((size_t)page, sorted[i]))
        return refuse(fn, "query identifier " + std::to_string(sorted[i]) + " is already merged for page " + std::to_string(page));
    }
    for (int32_t id : sorted) t->set((size_t)page, id);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  return PRB_OK;
}
// the identifiers of the batch being merged into t, on the device (the current one)
inline int upload_ids(prb_ctx *ctx, RunTable *t, const int32_t *query_ids, int32_t nq) {
  if (int rc = t->ids.ensure(std::max<size_t>((size_t)nq * 4, 4))) return rc;
  PRB_HIP(hipMemcpyAsync(t->ids.p, query_ids, (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  return PRB_OK;
}
// Page `page` searched and merged into the run table `t` under the caller's identifiers.  A failure from the upload on
// leaves the table unusable.
inline int merge_run_page(const char *fn_name, const char *what, const char *finish_fn, RunTable *t, prb_ctx *ctx, prb_qbatch *qb, prb_db *db,
                          int32_t page, const prb_ris_opts *opts, const int32_t *query_ids) {
  if (!t || !query_ids) return refuse(fn_name, "bad argument");
  if (int rc = check_search_args(fn_name, ctx, qb, db, page, opts, 3)) return rc;
  if (int rc = run_table_guard(fn_name, what, finish_fn, t, ctx, db, page, opts->distinct_sites, opts->chain_sites, query_ids, qb->nq)) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  t->broken = true; // (until the merge is whole)
  int rc;
  if ((rc = upload_ids(ctx, t, query_ids, qb->nq))) return rc;
  if ((rc = search_into_table(t, ctx, qb, db, page, opts, t->counts))) return rc;
  t->broken = false;
  return PRB_OK;
}

// ---- prb_*_add_pairs / prb_nullset_observe: a caller's list of pair records merged like a page's
// The list against a page of nseq sequences and a batch of nq queries: every record within those ranges and with a hit,
// and no (query, db_id) twice
inline int records_guard(const std::string &fn, int64_t nseq, int64_t nq, const prb_pair_summary *pairs, int64_t n) {
  try {
    std::vector<int64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const prb_pair_summary &r = pairs[i];
      if (r.query < 0 || r.query >= nq || r.db_id < 0 || r.db_id >= nseq || r.hits < 1)
        return refuse(fn, "pair record " + std::to_string(i) + " is out of range (query " + std::to_string(r.query) + " of " + std::to_string(nq) +
                              ", db_id " + std::to_string(r.db_id) + " of " + std::to_string(nseq) + ", hits " + std::to_string(r.hits) + ")");
      keys[(size_t)i] = (int64_t)r.query * nseq + r.db_id;
    }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 1; i < keys.size(); i++)
      if (keys[i] == keys[i - 1])
        return refuse(fn, "the pair (query " + std::to_string(keys[i] / nseq) + ", db_id " + std::to_string(keys[i] % nseq) + ") has two records");
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  return PRB_OK;
}
// ... and on the device (the current one), in the table's `h_rec`
inline int upload_records(prb_ctx *ctx, DevBuf &h_rec, const prb_pair_summary *pairs, int64_t n) {
  const size_t bytes = (size_t)n * sizeof(prb_pair_summary);
  if (int rc = h_rec.ensure(std::max<size_t>(bytes, 8))) return rc;
  if (!n) return PRB_OK;
  PRB_HIP(hipMemcpyAsync(h_rec.p, pairs, bytes, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's array may go)
  return PRB_OK;
}

// ---- a batch of decoys merged into a table that keeps a bit per decoy (DecoySet, search_host.hpp)
// The ndq decoys decoy[i] of the queries owner[i], their bits counted from bit0 on: every owner and decoy number lies in
// its range, and no (owner, decoy) comes twice - before (`already`: how that message ends), or in the call
inline int decoys_guard(const std::string &fn, const DecoySet *t, int64_t bit0, const int32_t *owner, const int32_t *decoy, int32_t ndq,
                        const std::string &already) {
  try {
    std::vector<int64_t> bits((size_t)ndq);
    for (int32_t i = 0; i < ndq; i++) {
      if (owner[i] < 0 || owner[i] >= t->nq)
        return refuse(fn, "owner[" + std::to_string(i) + "] = " + std::to_string(owner[i]) + " is out of range (the batch has " +
                              std::to_string(t->nq) + " queries)");
      if (decoy[i] < 0 || decoy[i] >= t->ndecoys)
        return refuse(fn, "decoy[" + std::to_string(i) + "] = " + std::to_string(decoy[i]) + " is out of range (the table has " +
                              std::to_string(t->ndecoys) + " decoys per query)");
      bits[(size_t)i] = t->bit_of(bit0, owner[i], decoy[i]);
      if ((t->merged[(size_t)(bits[(size_t)i] >> 6)] >> (bits[(size_t)i] & 63)) & 1)
        return refuse(fn, "decoy " + std::to_string(decoy[i]) + " of query " + std::to_string(owner[i]) + already);
    }
    std::sort(bits.begin(), bits.end());
    for (size_t i = 1; i < bits.size(); i++)
      if (bits[i] == bits[i - 1])
        return refuse(fn, "decoy " + std::to_string((bits[i] - bit0) % t->ndecoys) + " of query " + std::to_string((bits[i] - bit0) / t->ndecoys) +
                              " is given twice");
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  return PRB_OK;
}
// ... behind the guard: their bits set
inline void mark_decoys(DecoySet *t, int64_t bit0, const int32_t *owner, const int32_t *decoy, int32_t ndq) {
  for (int32_t i = 0; i < ndq; i++) {
    const int64_t b = t->bit_of(bit0, owner[i], decoy[i]);
    t->merged[(size_t)(b >> 6)] |= 1ull << (b & 63);
  }
  t->nmerged += ndq;
}
// ... and their owners and decoy numbers on the device (the current one)
inline int upload_owners(prb_ctx *ctx, DecoySet *t, const int32_t *owner, const int32_t *decoy, int32_t ndq) {
  if (int rc = t->own.ensure(std::max<size_t>((size_t)ndq * 8, 8))) return rc;
  t->ndq = ndq;
  if (!ndq) return PRB_OK;
  PRB_HIP(hipMemcpyAsync(t->own.p, owner, (size_t)ndq * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(t->own.as<int32_t>() + ndq, decoy, (size_t)ndq * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's arrays may go)
  return PRB_OK;
}

// ---- the device's `bad` flag to the host, in t->bad (the stream is drained: every merge of such a table ends with this)
inline int fetch_bad(prb_ctx *ctx, TableState *t) {
  uint32_t flag = 0;
  PRB_HIP(hipMemcpyAsync(&flag, t->badflag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  t->bad = flag != 0;
  return PRB_OK;
}

// ---- prb_*_merge: two unfinished tables over disjoint page or (page, identifier) sets into one
// What they all check first: `dst` belongs to ctx, both are unfinished and whole, own() has no refusal of the table's
// own ("" = none; asked once both are known to be whole and unfinished), and both were searched with one distinct_sites and one chain_sites
template <class Own>
int merge_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const TableState *dst, const TableState *src, Own own) {
  const std::string tables = std::string(what) + " tables";
  if (!ctx || !dst || !src || dst == src) return refuse(fn_name, "bad argument");
  if (dst->ctx != ctx) return refuse(fn_name, "the table to merge into belongs to another context");
  if (dst->broken || src->broken) return refuse(fn_name, "an earlier merge into one of the " + tables + " failed");
  if (dst->finished || src->finished) return refuse(fn_name, "one of the " + tables + " is finished");
  if (const std::string why = own(); !why.empty()) return refuse(fn_name, why);
  if (const std::string why = selection_clash(tables, "hold", dst, src->distinct, src->chain, " and ", ""); !why.empty())
    return refuse(fn_name, why);
  return PRB_OK;
}
// ... of two batch tables: made for the same queries, and no page is in both
inline int merge_tables_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const MergeTable *dst, const MergeTable *src) {
  const std::string tables = std::string(what) + " tables";
  if (int rc = merge_guard(fn_name, what, ctx, dst, src, [&]() -> std::string {
        if (dst->nq != src->nq) return "the " + tables + " were made for " + std::to_string(dst->nq) + " and " + std::to_string(src->nq) + " queries";
        if (dst->qlen != src->qlen) return "the " + tables + " were made for queries of different lengths";
        return "";
      }))
    return rc;
  if (dst->db && src->db) {
    if (dst->merged.size() != src->merged.size())
      return refuse(fn_name, "the " + tables + " hold pages of databases of " + std::to_string(dst->merged.size()) + " and " +
                                 std::to_string(src->merged.size()) + " pages");
    for (size_t p = 0; p < dst->merged.size(); p++)
      if (dst->merged[p] && src->merged[p]) return refuse(fn_name, "page " + std::to_string(p) + " is merged into both " + tables);
  }
  return PRB_OK;
}
// ... of two run tables: more() has no refusal of the table's own, they were made for databases of one shape, and no
// (page, identifier) is in both
template <class More>
int run_tables_guard(const char *fn_name, const char *what, const prb_ctx *ctx, const RunTable *dst, const RunTable *src, More more) {
  const std::string tables = std::string(what) + " tables";
  if (int rc = merge_guard(fn_name, what, ctx, dst, src, [&]() -> std::string {
        if (const std::string why = more(); !why.empty()) return why;
        return dst->tbase != src->tbase ? "the " + tables + " were made for different databases" : "";
      }))
    return rc;
  for (size_t p = 0; p < dst->merged.size(); p++) {
    const std::vector<uint64_t> &a = dst->merged[p], &b = src->merged[p];
    for (size_t k = 0; k < std::min(a.size(), b.size()); k++)
      if (a[k] & b[k]) return refuse(fn_name, "a query identifier is merged for page " + std::to_string(p) + " into both " + tables);
  }
  return PRB_OK;
}

// after the merge: dst's counts are the sums and its distinct_sites / chain_sites the merged pages'; src has merged nothing
inline void move_counts(TableState *dst, TableState *src) {
  for (int i = 0; i < 3; i++) {
    dst->counts[i] += src->counts[i];
    src->counts[i] = 0;
  }
  if (dst->distinct < 0) dst->distinct = src->distinct;
  if (dst->chain < 0) dst->chain = src->chain;
  src->distinct = src->chain = -1;
}
// ... and dst's page set is the union
inline void move_merged(MergeTable *dst, MergeTable *src) {
  if (src->db) {
    if (!dst->db) {
      dst->db = src->db;
      dst->merged = src->merged;
    } else {
      for (size_t p = 0; p < dst->merged.size(); p++) dst->merged[p] |= src->merged[p];
    }
  }
  move_counts(dst, src);
  src->db = nullptr;
  src->merged.clear();
}
// ... and dst's identifier sets are the unions
inline void move_merged(RunTable *dst, RunTable *src) {
  for (size_t p = 0; p < dst->merged.size(); p++) {
    std::vector<uint64_t> &a = dst->merged[p], &b = src->merged[p];
    if (a.size() < b.size()) a.resize(b.size(), 0);
    for (size_t k = 0; k < b.size(); k++) a[k] |= b[k];
    b.clear();
  }
  move_counts(dst, src);
}

// `bytes` at p on device `from` into `scratch` on ctx's device (the current one), complete on return or in order on
// ctx's stream: a peer copy where the devices allow it, else through pinned host memory
inline int fetch_remote(prb_ctx *ctx, int from, const void *p, size_t bytes, DevBuf &scratch) {
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
inline int on_device_of(prb_ctx *ctx, const prb_ctx *owner, void *p, size_t bytes, DevBuf &scratch, void **out) {
  PRB_HIP(hipStreamSynchronize(owner->stream));
  *out = p;
  if (owner->device == ctx->device || !p) return PRB_OK;
  if (int rc = fetch_remote(ctx, owner->device, p, bytes, scratch)) return rc;
  *out = scratch.p;
  return PRB_OK;
}

// The merge proper, behind the table's guard: src's block of `bytes` (and what `more` fetches) where dst's device reads
// it, join(block) enqueued in the bracket of `timer` with its `launches`, dst's book-keeping, then src emptied on its
// own device by `clear`.  A failure from the first launch on leaves dst unusable.
template <class T, class More, class Join, class Clear>
int join_tables(const char *fn_name, ModeTimer timer, int64_t launches, prb_ctx *ctx, T *dst, T *src, size_t bytes, More more,
                Join join, Clear clear) {
  DeviceScope restore;
  ScratchBuf copy;
  PRB_HIP(hipSetDevice(ctx->device));
  void *block = nullptr;
  int rc;
  if ((rc = on_device_of(ctx, src->ctx, src->table.p, bytes, copy, &block))) return rc;
  if ((rc = more())) return rc;
  dst->broken = true; // (until the merge is whole)
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = join(block))) return rc;
  if ((rc = ctx->time_end(timer, launches))) return rc; // (synchronises: src is read no more)
  dst->broken = false;
  try {
    move_merged(dst, src);
  } catch (const std::exception &e) { // (a page set that could not grow)
    dst->broken = true;
    return refuse(fn_name, e.what(), PRB_ERR_NOMEM);
  }
  return clear(*src);
}
inline int nothing_more() { return PRB_OK; }

} // namespace prb
