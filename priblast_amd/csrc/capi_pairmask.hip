// C ABI, part 9: the pair mask - the (query, target) pairs a search is restricted to (prb_pairmask_*,
// prb_ris_opts::allowed_pairs; `ris -L`).  The bits live on the host until the first search that uses the mask, which
// uploads them once; the kernels that read them are in seed_kernels.hip and ungapped_kernels.hip.
#include "search_host.hpp"

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

int64_t prb_pairmask_count(const prb_pairmask *pm) { return pm ? pm->count : -1; }
void prb_pairmask_free(prb_pairmask *pm) { delete pm; }

} // extern "C"
