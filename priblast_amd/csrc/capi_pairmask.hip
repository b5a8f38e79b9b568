// C ABI, part 9: the pair mask - the (query, target) pairs a search is restricted to (prb_pairmask_*,
// prb_ris_opts::allowed_pairs; `ris -L`).  The bits live on the host until the first search that uses the mask, which
// uploads them once; the kernels that read them are in seed_kernels.hip and ungapped_kernels.hip.  A mask of a null
// table's live pairs (prb_pairmask_create_live, `ris -t -z N -H H`) is made on the device instead and never changes.
#include "capi_tables.hpp"

using namespace prb;

int prb::use_pairmask(const char *fn, prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page, const prb_pairmask *pm,
                      AllowDev *view) {
  if (pm->qb != qb || pm->db != db || pm->nq != qb->nq || pm->tbase.size() != db->pages.size() + 1) {
    set_error(std::string(fn) + ": allowed_pairs was made for another query batch or another database");
    return PRB_ERR_ARG;
  }
  if (pm->ctx->device != ctx->device) {
    set_error(std::string(fn) + ": allowed_pairs was made on another device");
    return PRB_ERR_ARG;
  }
  prb_pairmask *m = const_cast<prb_pairmask *>(pm); // (the upload is not a change a caller can see)
  std::lock_guard<std::mutex> lk(m->first_use);       // two searches may meet at a mask's first use
  if (!m->used) {
    const size_t bytes = std::max<size_t>(m->bits.size() * sizeof(uint32_t), 16);
    if (int rc = m->dev.ensure(bytes)) return rc;
    if (!m->bits.empty()) PRB_HIP(hipMemcpy(m->dev.p, m->bits.data(), m->bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    m->used = true;
  }
  *view = AllowDev{m->dev.as<uint32_t>(), m->row_words, m->tbase[(size_t)page]};
  return PRB_OK;
}

extern "C" {

int prb_pairmask_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, prb_pairmask **out) {
  if (!ctx || !qb || !db || !out || qb->ctx->device != ctx->device || db->ctx->device != ctx->device) {
    set_error("prb_pairmask_create: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  try {
    std::unique_ptr<prb_pairmask> m(new prb_pairmask());
    m->ctx = ctx;
    m->qb = qb;
    m->db = db;
    m->nq = qb->nq;
    m->tbase.assign(db->pages.size() + 1, 0);
    for (size_t p = 0; p < db->pages.size(); p++) m->tbase[p + 1] = m->tbase[p] + db->pages[p].nseq;
    m->row_words = (m->tbase.back() + 31) / 32;
    m->bits.assign((size_t)m->nq * (size_t)m->row_words, 0u);
    *out = m.release();
  } catch (const std::exception &e) {
    set_error(std::string("prb_pairmask_create: ") + e.what());
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}

int prb_pairmask_allow(prb_pairmask *pm, int64_t n, const int32_t *query, const int32_t *page, const int32_t *db_id) {
  if (!pm || n < 0 || (n > 0 && (!query || !page || !db_id))) {
    set_error("prb_pairmask_allow: bad argument");
    return PRB_ERR_ARG;
  }
  if (pm->used) {
    set_error("prb_pairmask_allow: the mask has been used by a search; pairs are allowed before its first use only");
    return PRB_ERR_STATE;
  }
  const int32_t npages = (int32_t)pm->tbase.size() - 1;
  for (int64_t i = 0; i < n; i++) { // all of the call, or nothing
    const bool q_ok = query[i] >= -1 && query[i] < pm->nq, p_ok = page[i] >= 0 && page[i] < npages;
    if (q_ok && p_ok && db_id[i] >= 0 && db_id[i] < pm->tbase[(size_t)page[i] + 1] - pm->tbase[(size_t)page[i]]) continue;
    set_error("prb_pairmask_allow: entry " + std::to_string(i) + " is out of range (query " + std::to_string(query[i]) + " of " +
              std::to_string(pm->nq) + ", page " + std::to_string(page[i]) + " of " + std::to_string(npages) + ", db_id " +
              std::to_string(db_id[i]) + ")");
    return PRB_ERR_ARG;
  }
  for (int64_t i = 0; i < n; i++) {
    const int64_t t = pm->tbase[(size_t)page[i]] + db_id[i];
    const int32_t q0 = query[i] < 0 ? 0 : query[i], q1 = query[i] < 0 ? pm->nq : query[i] + 1;
    for (int32_t q = q0; q < q1; q++) {
      uint32_t &w = pm->bits[(size_t)q * (size_t)pm->row_words + (size_t)(t >> 5)];
      const uint32_t b = 1u << (t & 31);
      pm->count += !(w & b);
      w |= b;
    }
  }
  return PRB_OK;
}

// The mask of a decoy batch from a null table's live pairs: made on the device (k_null_live_mask, null_kernels.hip) in a
// bracket of the "allow" timer, and born used - its bits never exist on the host
int prb_pairmask_create_live(prb_ctx *ctx, prb_nullset *ns, const prb_qbatch *dqb, const int32_t *owner, int32_t ndq, prb_pairmask **out) {
  const char *fn = "prb_pairmask_create_live";
  if (!ctx || !ns || !dqb || !out || ndq < 0 || (ndq && !owner) || dqb->ctx->device != ctx->device) return refuse(fn, "bad argument");
  *out = nullptr;
  if (ns->ctx != ctx) return refuse(fn, "the null table was made with another context");
  if (ns->broken) return refuse(fn, "an earlier merge into this null table failed", PRB_ERR_STATE);
  if (ns->bad) return refuse(fn, "a record merged into this null table named a query, a sequence, an owner or a decoy outside it", PRB_ERR_STATE);
  if (ns->finished) return refuse(fn, "the null table is finished (prb_nullset_finish)", PRB_ERR_STATE);
  if (ndq != dqb->nq) return refuse(fn, "the decoy batch has " + std::to_string(dqb->nq) + " queries (owner[] has " + std::to_string(ndq) + ")");
  for (int32_t k = 0; k < ndq; k++)
    if (owner[k] < 0 || owner[k] >= ns->nq)
      return refuse(fn, "owner[" + std::to_string(k) + "] = " + std::to_string(owner[k]) + " is out of range (the batch has " + std::to_string(ns->nq) +
                            " queries)");
  std::unique_ptr<prb_pairmask> m;
  std::vector<int32_t> lists; // uowner[nown], rowoff[nown + 1], rows[ndq]
  int32_t nown = 0;
  try {
    m.reset(new prb_pairmask());
    m->ctx = ctx;
    m->qb = dqb;
    m->db = ns->db;
    m->nq = ndq;
    m->tbase = ns->tbase;
    m->row_words = (m->tbase.back() + 31) / 32;
    // the batch's rows by owner (stable: an owner's rows ascending)
    std::vector<int32_t> rows((size_t)ndq);
    for (int32_t k = 0; k < ndq; k++) rows[(size_t)k] = k;
    std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) { return owner[a] < owner[b]; });
    std::vector<int32_t> uowner, rowoff;
    for (int32_t i = 0; i < ndq; i++)
      if (!i || owner[rows[(size_t)i]] != owner[rows[(size_t)i - 1]]) uowner.push_back(owner[rows[(size_t)i]]), rowoff.push_back(i);
    rowoff.push_back(ndq);
    nown = (int32_t)uowner.size();
    lists = uowner;
    lists.insert(lists.end(), rowoff.begin(), rowoff.end());
    lists.insert(lists.end(), rows.begin(), rows.end());
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  const size_t words = (size_t)ndq * (size_t)m->row_words;
  ScratchBuf dl, dc;
  int rc;
  if ((rc = m->dev.ensure(std::max<size_t>(words * sizeof(uint32_t), 16))) || (rc = dl.ensure(lists.size() * 4)) || (rc = dc.ensure(16))) return rc;
  m->used = true;
  if (words) {
    PRB_HIP(hipMemcpyAsync(dl.p, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    PRB_HIP(hipMemsetAsync(dc.p, 0, 8, ctx->stream));
    if ((rc = ctx->time_begin())) return rc;
    const LiveMaskRows r{dl.as<int32_t>(), dl.as<int32_t>() + nown, dl.as<int32_t>() + 2 * nown + 1, nown};
    PRB_HIP(launch_null_live_mask(ns->view(), r, m->dev.as<uint32_t>(), m->row_words, dc.as<unsigned long long>(), ctx->stream));
    unsigned long long count = 0;
    PRB_HIP(hipMemcpyAsync(&count, dc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kAllow, 1))) return rc; // (synchronises: the lists and the count are done with)
    m->count = (int64_t)count;
  }
  *out = m.release();
  return PRB_OK;
}

int64_t prb_pairmask_count(const prb_pairmask *pm) { return pm ? pm->count : -1; }
int64_t prb_pairmask_row_words(const prb_pairmask *pm) { return pm ? pm->row_words : -1; }
// the words as a search reads them: the device's once the mask is used, the host's before
int prb_pairmask_words(const prb_pairmask *pm, uint32_t *out, int64_t n) {
  const char *fn = "prb_pairmask_words";
  if (!pm || n < 0 || (n && !out)) return refuse(fn, "bad argument");
  const int64_t have = (int64_t)pm->nq * pm->row_words;
  if (n > have) return refuse(fn, "the mask has " + std::to_string(have) + " words (asked for " + std::to_string(n) + ")");
  if (!n) return PRB_OK;
  if (!pm->used) {
    std::copy(pm->bits.begin(), pm->bits.begin() + n, out);
    return PRB_OK;
  }
  DeviceScope restore;
  PRB_HIP(hipSetDevice(pm->ctx->device));
  PRB_HIP(hipMemcpy(out, pm->dev.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PRB_OK;
}
void prb_pairmask_free(prb_pairmask *pm) { delete pm; }

} // extern "C"
