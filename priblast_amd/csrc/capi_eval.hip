// C ABI, part 12: the evalset of one batch - the energy keys of its final hits and of its decoys', pooled per query over
// the whole database, and per real hit the E-value and the FDR q-value that they give (prb_evalset_*, `ris -k N -E M`).
// The kernels are in eval_kernels.hip.  Every check of a call is made on the host before anything is enqueued: a refused
// call leaves the table as it was.
#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kCloseFn = "prb_evalset_close";
const char *const kBadWhy = "a record merged into this evalset named a query, an owner or a decoy outside it, or a key was looked up that it does not hold";
constexpr int64_t kEvalMaxKeys = (int64_t)UINT32_MAX; // per list: both factors of a cross-multiplication stay below 2^32

// What every call on the table checks of it first
int eval_guard(const std::string &fn, const prb_ctx *ctx, const prb_evalset *es) {
  if (!ctx || !es) return refuse(fn, "bad argument");
  if (es->ctx != ctx) return refuse(fn, "the evalset was made with another context");
  if (es->broken) return refuse(fn, "an earlier merge into this evalset failed", PRB_ERR_STATE);
  if (es->bad) return refuse(fn, kBadWhy, PRB_ERR_STATE);
  return PRB_OK;
}
// ... and every call that appends to it
int open_guard(const std::string &fn, const prb_ctx *ctx, const prb_evalset *es) {
  if (int rc = eval_guard(fn, ctx, es)) return rc;
  if (es->finished) return refuse(fn, std::string("the evalset is closed (") + kCloseFn + ")", PRB_ERR_STATE);
  return PRB_OK;
}
int page_guard(const std::string &fn, const prb_evalset *es, int32_t page) {
  if (page < 0 || page >= es->npages)
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(es->npages) + ")");
  return PRB_OK;
}

// room for `more` entries behind the list's end; what it holds moves along.  `fn` names the entry point.
int reserve(const char *fn, prb_ctx *ctx, prb_evalset::List &l, int64_t more) {
  if (more > kEvalMaxKeys - l.n)
    return refuse(fn, "a list of the evalset would hold " + std::to_string(l.n + more) + " keys (at most 2^32 - 1)", PRB_ERR_STATE);
  if (l.n + more <= l.cap) return PRB_OK;
  const int64_t cap = std::min(kEvalMaxKeys, std::max<int64_t>({2 * l.cap, l.n + more, 1 << 16}));
  DevBuf key, own;
  if (key.ensure((size_t)cap * 8) != PRB_OK || own.ensure((size_t)cap * 4) != PRB_OK) {
    key.release();
    own.release();
    return refuse(fn, "can't allocate a list of the evalset (" + std::to_string(((size_t)cap * 12) >> 20) + " MB of HBM for " + std::to_string(cap) + " keys)",
                  PRB_ERR_NOMEM);
  }
  if (l.n) {
    PRB_HIP(hipMemcpyAsync(key.p, l.key.p, (size_t)l.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PRB_HIP(hipMemcpyAsync(own.p, l.own.p, (size_t)l.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
  }
  try {
    if (l.key.p) l.retired.push_back(l.key);
    if (l.own.p) l.retired.push_back(l.own);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  l.key = key;
  l.own = own;
  l.cap = cap;
  return PRB_OK;
}

// a caller's (identifier, energy) list on the device
int upload_list(prb_ctx *ctx, prb_evalset *es, const int32_t *ids, const double *energy, int64_t n) {
  int rc;
  if ((rc = es->h_ids.ensure(std::max<size_t>((size_t)n * 4, 8))) || (rc = es->h_energy.ensure(std::max<size_t>((size_t)n * 8, 8)))) return rc;
  if (!n) return PRB_OK;
  PRB_HIP(hipMemcpyAsync(es->h_ids.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipMemcpyAsync(es->h_energy.p, energy, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the caller's arrays may go)
  return PRB_OK;
}

} // namespace

// prb_search_page_scored / _null_hits (per sub-batch) and prb_evalset_add_keys: n keys behind the end of the real list
// or - under the owners of the batch being merged (mapped), or under ids themselves - of the decoy list, in a bracket of
// the "eval" timer
static int append_eval_keys(const char *fn, prb_ctx *ctx, prb_evalset *es, bool to_decoys, bool mapped, const int32_t *ids, const double *energy,
                            int64_t n) {
  prb_evalset::List &l = to_decoys ? es->dec : es->real;
  int rc;
  if ((rc = reserve(fn, ctx, l, n))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_eval_append(ids, energy, n, mapped ? es->own.as<int32_t>() : nullptr, mapped ? es->own.as<int32_t>() + es->ndq : nullptr,
                             es->ndq, es->nq, es->ndecoys, l.key.as<unsigned long long>() + l.n, l.own.as<uint32_t>() + l.n,
                             es->badflag.as<uint32_t>(), ctx->stream));
  l.n += n;
  if ((rc = ctx->time_end(ModeTimer::kEval, 1))) return rc;
  return fetch_bad(ctx, es);
}
// a sub-batch of the batch being searched: a decoy batch's while prb_search_page_null_hits says so, else the real one's -
// which goes on to the top-N hit table of prb_search_page_scored as it came
int prb_evalset::take(const SubBatch &b) {
  if (decoy_phase) return append_eval_keys("prb_search_page_null_hits", ctx, this, true, true, b.F.query, b.F.e_tot, b.nfin);
  if (int rc = append_eval_keys("prb_search_page_scored", ctx, this, false, false, b.F.query, b.F.e_tot, b.nfin)) return rc;
  return tee ? tee->take(b) : PRB_OK;
}

// prb_evalset_close, per list: the entries into (query, key) order - a stable sort by key, then one by query - and the
// queries' segment sizes counted into cnt[nq].  The sorts are capi_search.hip's (search_host.hpp: no sort is instantiated
// here).  Scratch, sized by the caller for the longer list: keyB [n], idx [3 n], q2 [n]; the sorts' temporary storage: one
// buffer each, so that neither grows under the other's work.
static int sort_eval_list(prb_ctx *ctx, prb_evalset *es, prb_evalset::List &l, DevBuf &keyB, DevBuf &idx, DevBuf &q2, DevBuf &tmp64, DevBuf &tmp32,
                          uint32_t *cnt, int64_t *launches) {
  const int64_t n = l.n;
  if (!n) return PRB_OK;
  const size_t N = (size_t)n;
  int rc;
  uint32_t *iota = idx.as<uint32_t>(), *by_key = iota + N, *by_query = by_key + N, *bad = es->badflag.as<uint32_t>();
  unsigned long long *key = l.key.as<unsigned long long>();
  uint32_t *own = l.own.as<uint32_t>();
  PRB_HIP(launch_eval_count(own, n, es->nq, cnt, bad, ctx->stream));
  PRB_HIP(launch_eval_iota(iota, n, ctx->stream));
  if ((rc = with_temp(tmp64, "rocprim::radix_sort_pairs", [&](void *t, size_t &b) {
         return sort_span_keys(t, b, reinterpret_cast<uint64_t *>(key), keyB.as<uint64_t>(), iota, by_key, N, 64, ctx->stream);
       })))
    return rc;
  PRB_HIP(launch_eval_gather32(own, by_key, q2.as<uint32_t>(), n, bad, ctx->stream));
  // (own <- the queries in order; by_query[k] = the place in key order of the entry that comes k-th)
  if ((rc = sort_target_keys(ctx->stream, tmp32, q2.as<uint32_t>(), own, iota, by_query, N, (unsigned)bits_for(std::max(0, es->nq - 1))))) return rc;
  PRB_HIP(launch_eval_gather64(keyB.as<unsigned long long>(), by_query, key, n, bad, ctx->stream));
  *launches += 6;
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (the next list shares the scratch, and a temporary buffer that grows is freed)
  return PRB_OK;
}

extern "C" {

int prb_evalset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t ndecoys, prb_evalset **out) {
  const char *fn = "prb_evalset_create";
  std::unique_ptr<prb_evalset> es;
  const bool args_ok = ctx && qb && db && qb->ctx->device == ctx->device && db->ctx->device == ctx->device;
  if (int rc = new_table(fn, args_ok, out, es,
                         ndecoys < 1 || ndecoys > 100000 ? "need 1 <= ndecoys <= 100000 (got " + std::to_string(ndecoys) + ")" : ""))
    return rc;
  try {
    es->nq = qb->nq;
    es->ndecoys = ndecoys;
    es->npages = (int32_t)db->pages.size();
    es->real_merged.assign(db->pages.size(), 0);
    es->merged.assign((size_t)((es->triples() + 63) / 64), 0);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  es->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  es->db = db;
  es->qb = qb;
  PRB_HIP(hipSetDevice(ctx->device));
  if (int rc = es->badflag.ensure(16)) return rc;
  PRB_HIP(hipMemsetAsync(es->badflag.p, 0, 16, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  *out = es.release();
  return PRB_OK;
}

int prb_search_page_scored(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_tophits *th, prb_evalset *es) {
  const char *fn = "prb_search_page_scored";
  if (!es) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, qb, db, page, opts, 3)) return rc;
  if (es->qb != qb || es->nq != qb->nq || es->db != db) return refuse(fn, "the evalset was made for another query batch or another database");
  if (int rc = open_guard(fn, ctx, es)) return rc;
  if (int rc = page_guard(fn, es, page)) return rc;
  if (int rc = selection_guard(fn, "evalset", es, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, qb, db, opts)) return rc;
  if (es->real_merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged into this evalset");
  if (th) { // (its own refusals last: the guard marks the page as merged)
    if (th->style >= 0 && opts->output_style != th->style)
      return refuse(fn, "the top-N hit table holds pages searched with output_style " + std::to_string(th->style) + " (this call: " +
                            std::to_string(opts->output_style) + ")");
    if (int rc = merge_page_guard(fn, "top-N hit", "prb_tophits_finish", th, ctx, qb, db, page, opts)) return rc;
  }
  PRB_HIP(hipSetDevice(ctx->device));
  es->real_merged[(size_t)page] = 1;
  es->nreal_merged++;
  es->searched = true;
  es->broken = true; // (until the merge is whole)
  if (th) th->broken = true;
  int64_t got[3] = {0, 0, 0};
  es->tee = th;
  const int rc = search_into_table(es, ctx, qb, db, page, opts, got);
  es->tee = nullptr;
  if (rc) return rc;
  for (int i = 0; i < 3; i++) es->counts[i] += got[i];
  es->broken = false;
  if (th) {
    for (int i = 0; i < 3; i++) th->counts[i] += got[i];
    th->distinct = opts->distinct_sites;
    th->chain = opts->chain_sites;
    th->style = opts->output_style;
    th->broken = false;
  }
  return PRB_OK;
}

int prb_search_page_null_hits(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *owner,
                              const int32_t *decoy, prb_evalset *es) {
  const char *fn = "prb_search_page_null_hits";
  if (!es || !owner || !decoy) return refuse(fn, "bad argument");
  if (int rc = check_search_args(fn, ctx, dqb, db, page, opts, 3)) return rc;
  if (es->db != db) return refuse(fn, "the evalset was made for another database");
  if (int rc = open_guard(fn, ctx, es)) return rc;
  if (int rc = page_guard(fn, es, page)) return rc;
  if (int rc = selection_guard(fn, "evalset", es, opts)) return rc;
  if (int rc = mask_guard(fn, ctx, dqb, db, opts)) return rc;
  if (int rc = decoys_guard(fn, es, es->bit0(page), owner, decoy, dqb->nq, " is already merged for page " + std::to_string(page))) return rc;
  PRB_HIP(hipSetDevice(ctx->device));
  es->broken = true; // (until the merge is whole)
  es->searched = true;
  mark_decoys(es, es->bit0(page), owner, decoy, dqb->nq);
  if (int rc = upload_owners(ctx, es, owner, decoy, dqb->nq)) return rc;
  es->decoy_phase = true;
  const int rc = search_into_table(es, ctx, dqb, db, page, opts, es->decoy_counts, false);
  es->decoy_phase = false;
  if (rc) return rc;
  es->broken = false;
  return PRB_OK;
}

int prb_evalset_add_keys(prb_ctx *ctx, prb_evalset *es, int32_t is_decoy, const int32_t *query_or_owner, const double *energy, int64_t n) {
  const char *fn = "prb_evalset_add_keys";
  if (n < 0 || n > INT32_MAX || (n && (!query_or_owner || !energy))) return refuse(fn, "bad argument");
  if (int rc = open_guard(fn, ctx, es)) return rc;
  if (!n) return PRB_OK;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  es->broken = true; // (until the merge is whole)
  if (int rc = upload_list(ctx, es, query_or_owner, energy, n)) return rc;
  if (int rc = append_eval_keys(fn, ctx, es, is_decoy != 0, false, es->h_ids.as<int32_t>(), es->h_energy.as<double>(), n)) return rc;
  es->broken = false;
  return PRB_OK;
}

int prb_evalset_close(prb_ctx *ctx, prb_evalset *es) {
  const char *fn = kCloseFn;
  if (int rc = eval_guard(fn, ctx, es)) return rc;
  if (es->finished) return PRB_OK;
  if (es->searched && (es->nreal_merged != es->npages || es->nmerged != es->triples()))
    return refuse(fn, std::to_string(es->nreal_merged) + " of " + std::to_string(es->npages) + " pages of the real batch and " + std::to_string(es->nmerged) +
                          " of " + std::to_string(es->triples()) +
                          " (query, decoy, page) searches are merged: every page, and every decoy of every query against every page, comes first",
                  PRB_ERR_STATE);
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  const size_t NQ = (size_t)es->nq, NR = (size_t)std::max<int64_t>(es->real.n, 1);
  int rc;
  ScratchBuf keyB, idx, q2, tmp64, tmp32, cnt;
  const size_t NM = (size_t)std::max<int64_t>({es->real.n, es->dec.n, 1});
  if ((rc = keyB.ensure(NM * 8)) || (rc = idx.ensure(3 * NM * 4)) || (rc = q2.ensure(NM * 4))) return rc;
  if ((rc = cnt.ensure(std::max<size_t>(2 * NQ * 4, 8))) || (rc = es->off.ensure(2 * (NQ + 1) * 8)) || (rc = es->null_le.ensure(NR * 4)) ||
      (rc = es->rank.ensure(NR * 4)) || (rc = es->qnum.ensure(NR * 4)) || (rc = es->qden.ensure(NR * 4)))
    return rc;
  es->broken = true; // (until the close is whole)
  int64_t launches = 0;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(hipMemsetAsync(cnt.p, 0, std::max<size_t>(2 * NQ * 4, 8), ctx->stream));
  if ((rc = sort_eval_list(ctx, es, es->real, keyB, idx, q2, tmp64, tmp32, cnt.as<uint32_t>(), &launches))) return rc;
  if ((rc = sort_eval_list(ctx, es, es->dec, keyB, idx, q2, tmp64, tmp32, cnt.as<uint32_t>() + NQ, &launches))) return rc;
  // the segments' bounds from the counts: a prefix sum of nq numbers per list, on the host
  try {
    std::vector<uint32_t> c(2 * NQ);
    std::vector<int64_t> off(2 * (NQ + 1), 0);
    if (NQ) PRB_HIP(hipMemcpyAsync(c.data(), cnt.p, 2 * NQ * 4, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t l = 0; l < 2; l++)
      for (size_t q = 0; q < NQ; q++) off[l * (NQ + 1) + q + 1] = off[l * (NQ + 1) + q] + (int64_t)c[l * NQ + q];
    if (off[NQ] != es->real.n || off[2 * NQ + 1] != es->dec.n)
      return refuse(fn, "the segments hold " + std::to_string(off[NQ]) + " and " + std::to_string(off[2 * NQ + 1]) + " keys, the lists " +
                            std::to_string(es->real.n) + " and " + std::to_string(es->dec.n),
                    PRB_ERR_STATE);
    PRB_HIP(hipMemcpyAsync(es->off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory)
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  PRB_HIP(launch_eval_rank(es->view(), ctx->stream));
  PRB_HIP(launch_eval_qmin(es->view(), ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kEval, launches + 2))) return rc;
  if ((rc = fetch_bad(ctx, es))) return rc;
  if (es->bad) return refuse(fn, "an index of the close lies outside its list", PRB_ERR_STATE);
  // (only the sorted keys and the real entries' figures are needed from here on)
  es->drop_retired();
  for (DevBuf *b : {&es->real.own, &es->dec.own, &es->own}) b->release();
  es->broken = false;
  es->finished = true;
  return PRB_OK;
}

int prb_evalset_score(prb_ctx *ctx, prb_evalset *es, const int32_t *query, const double *energy, int64_t n, prb_eval_score *out) {
  const char *fn = "prb_evalset_score";
  if (n < 0 || n > INT32_MAX || (n && (!query || !energy || !out))) return refuse(fn, "bad argument");
  if (int rc = eval_guard(fn, ctx, es)) return rc;
  if (!es->finished) return refuse(fn, std::string("the evalset is not closed yet (") + kCloseFn + ")", PRB_ERR_STATE);
  if (!n) return PRB_OK;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = upload_list(ctx, es, query, energy, n)) || (rc = es->out.ensure((size_t)n * sizeof(prb_eval_score)))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  PRB_HIP(launch_eval_lookup(es->view(), es->h_ids.as<int32_t>(), es->h_energy.as<double>(), n, es->out.p, ctx->stream));
  PRB_HIP(hipMemcpyAsync(out, es->out.p, (size_t)n * sizeof(prb_eval_score), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = ctx->time_end(ModeTimer::kEval, 1))) return rc; // (synchronises: the copy is over)
  if ((rc = fetch_bad(ctx, es))) return rc;
  if (es->bad) return refuse(fn, "a query is out of range, or a key is not among its query's real hits", PRB_ERR_STATE);
  return PRB_OK;
}

void prb_evalset_sizes(const prb_evalset *es, int64_t *nreal, int64_t *ndecoy) {
  if (nreal) *nreal = es ? es->real.n : -1;
  if (ndecoy) *ndecoy = es ? es->dec.n : -1;
}
void prb_evalset_counts(const prb_evalset *es, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = es ? es->counts[i] : 0;
}
void prb_evalset_decoy_counts(const prb_evalset *es, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = es ? es->decoy_counts[i] : 0;
}
void prb_evalset_free(prb_evalset *es) { delete es; }

} // extern "C"
