// C ABI, part 2: database pages on the device (resident or streamed), query batches, and the seed search proper
// that runs ahead of a page's search on host threads.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "search_host.hpp"
#include "cpu_budget.hpp"
#include "encoder.hpp"
#include "suffix_array.hpp"

using namespace prb;

namespace prb {
int run_accessibility(prb_ctx *ctx, int32_t nseq, const char *seqs, const int64_t *in_off, const int32_t *lens,
                      const int64_t *out_off, int W, int delta, float *d_acc, float *d_cond);

// An explicit count, because launchers such as torchrun export OMP_NUM_THREADS=1 (cpu_budget.hpp for the default)
int host_threads(int work_items) {
  static const int cap = [] {
    const char *e = getenv("PRB_HOST_THREADS");
    int n = e ? atoi(e) : default_host_threads();
    return std::max(1, n);
  }();
  return std::max(1, std::min(cap, work_items));
}
} // namespace prb

extern "C" {

int prb_search_const_upload(prb_ctx *ctx) {
  auto *m = new SearchConstMem();
  ctx->search_const = m;
  const EnergyParams &p = ctx->params;
  std::vector<int32_t> ints;
  auto add = [&](const int *src, size_t n) {
    size_t at = ints.size();
    ints.insert(ints.end(), src, src + n);
    return at;
  };
  const size_t o_stack = add(&p.stack37[0][0], 49), o_int = add(p.internal37, 31), o_mm = add(&p.mismatchI37[0][0][0], 175),
               o_11 = add(&p.int11_37[0][0][0][0], 1600), o_21 = add(&p.int21_37[0][0][0][0][0], 8000),
               o_22 = add(&p.int22_37[0][0][0][0][0][0], 40000), o_d5 = add(&p.dangle5_37[0][0], 40),
               o_d3 = add(&p.dangle3_37[0][0], 40);
  {
    using T = SearchTab;
    if (o_stack != T::kStack || o_int != T::kInternal || o_mm != T::kMismatchI || o_11 != T::kInt11 || o_21 != T::kInt21 ||
        o_22 != T::kInt22 || o_d5 != T::kDangle5 || o_d3 != T::kDangle3) {
      set_error("internal error: SearchTab layout");
      return PRB_ERR_STATE;
    }
    add(p.bulge37, 31);
    int tau[8] = {0, 0, 0, p.terminal_au, p.terminal_au, p.terminal_au, p.terminal_au, 0};
    add(tau, 8);
    int zero = 0;
    add(&zero, 1);
  }
  std::vector<double> bulge(64);
  for (int u = 0; u < 64; u++) // gapped_extension.cpp:439
    bulge[u] = u <= 30 ? (double)p.bulge37[u] : p.bulge37[30] + p.lxc37 * std::log(u / 30.);
  int rc;
  if ((rc = m->ints.ensure(ints.size() * 4))) return rc;
  if ((rc = m->bulge.ensure(bulge.size() * 8))) return rc;
  PRB_HIP(hipMemcpy(m->ints.p, ints.data(), ints.size() * 4, hipMemcpyHostToDevice));
  PRB_HIP(hipMemcpy(m->bulge.p, bulge.data(), bulge.size() * 8, hipMemcpyHostToDevice));
  for (int t = 0; t < 7; t++)
    if (p.rtype[t] != (t == 0 ? 0 : ((t - 1) ^ 1) + 1)) {
      set_error("parameter file: rtype is not the expected pair-type involution");
      return PRB_ERR_ARG;
    }
  const int32_t *b = m->ints.as<int32_t>();
  SearchConst &v = m->view;
  v.tab = b;
  v.stack37 = b + o_stack;
  v.internal37 = b + o_int;
  v.mismatchI37 = b + o_mm;
  v.int11 = b + o_11;
  v.int21 = b + o_21;
  v.int22 = b + o_22;
  v.dangle5 = b + o_d5;
  v.dangle3 = b + o_d3;
  v.bulge = m->bulge.as<double>();
  v.bp_rows = 0;
  for (int a = 1; a < 5; a++)
    for (int c = 0; c < 5; c++) v.bp_rows |= (uint64_t)(p.bp_pair[a][c] & 7) << (15 * (a - 1) + 3 * c);
  v.terminal_au = p.terminal_au;
  for (int a = 0; a < 5; a++)
    for (int c = 0; c < 5; c++) v.bp_pair[a * 5 + c] = (unsigned char)p.bp_pair[a][c];
  v.pair_mask = v.wobble_mask = 0;
  for (int a = 0; a < 5; a++)
    for (int c = 0; c < 5; c++) {
      if (p.bp_pair[a][c] != 0) v.pair_mask |= 1u << (a * 5 + c);
      if (p.bp_pair[a][c] == 3 || p.bp_pair[a][c] == 4) v.wobble_mask |= 1u << (a * 5 + c);
    }
  return PRB_OK;
}

void prb_search_const_free(prb_ctx *ctx) {
  if (ctx->search_const) {
    auto *m = static_cast<SearchConstMem *>(ctx->search_const);
    m->ints.release();
    m->bulge.release();
    delete m;
    ctx->search_const = nullptr;
  }
  if (ctx->search_ws) {
    auto *w = static_cast<SearchWs *>(ctx->search_ws);
    w->release();
    delete w;
    ctx->search_ws = nullptr;
  }
}

} // extern "C"

namespace prb {
// ------------------------------------------------------------------------ database
static int upload_page(const DbPage &pg, PageMem &m, hipStream_t stream) {
  int rc;
  auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
    if ((rc = b.ensure(std::max<size_t>(bytes, 16)))) return rc;
    if (bytes) PRB_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, stream));
    return PRB_OK;
  };
  if ((rc = up(m.seqs, pg.seqs.data(), pg.seqs.size()))) return rc;
  if ((rc = up(m.sa, pg.sa.data(), pg.sa.size() * 4))) return rc;
  if ((rc = up(m.start_pos, pg.start_pos.data(), pg.start_pos.size() * 4))) return rc;
  if ((rc = up(m.seq_length, pg.seq_length.data(), pg.seq_length.size() * 4))) return rc;
  if ((rc = up(m.acc, pg.acc.data(), pg.acc.size() * 4))) return rc;
  if ((rc = up(m.cond, pg.cond.data(), pg.cond.size() * 4))) return rc;
  if ((rc = m.sa_seq.ensure(std::max<size_t>(pg.sa.size() * 4, 16)))) return rc;
  if ((rc = m.blk_seq.ensure((size_t)blk_seq_entries((int64_t)pg.seqs.size()) * 4))) return rc;
  m.view.seqs = m.seqs.as<uint8_t>();
  m.view.sa = m.sa.as<int32_t>();
  m.view.sa_seq = m.sa_seq.as<int32_t>();
  m.view.blk_seq = m.blk_seq.as<int32_t>();
  m.view.start_pos = m.start_pos.as<int32_t>();
  m.view.seq_length = m.seq_length.as<int32_t>();
  m.view.acc = m.acc.as<float>();
  m.view.cond = m.cond.as<float>();
  m.view.nchars = (int32_t)pg.seqs.size();
  m.view.nseq = pg.nseq;
  PRB_HIP(launch_sa_seq(m.view, m.sa_seq.as<int32_t>(), stream));
  PRB_HIP(launch_blk_seq(m.view, m.blk_seq.as<int32_t>(), stream));
  return PRB_OK;
}

// Page `page` on the device: its slot, uploaded now if need be (on `stream`; the slot's event is recorded behind
// the upload).  `keep` = a page whose slot must not be taken (the one being searched), or -1.
int page_slot(prb_ctx *user, prb_db *db, int page, int keep, hipStream_t stream, int *slot_out) {
  int slot = db->slot_of_page[page];
  if (slot < 0) {
    // a free slot, else the least recently used one
    for (size_t k = 0; k < db->page_in_slot.size() && slot < 0; k++)
      if (db->page_in_slot[k] < 0) slot = (int)k;
    if (slot < 0) {
      for (size_t k = 0; k < db->page_in_slot.size(); k++)
        if (db->page_in_slot[k] != keep && (slot < 0 || db->slot_used[k] < db->slot_used[(size_t)slot])) slot = (int)k;
      if (slot < 0) return PRB_ERR_STATE;
      // what still reads the slot's old page (a search on the context's stream, an earlier upload) must be over
      PRB_HIP(hipStreamSynchronize(user->stream));
      PRB_HIP(hipEventSynchronize(db->slot_ready[(size_t)slot]));
      db->slot_of_page[(size_t)db->page_in_slot[(size_t)slot]] = -1;
    }
    int rc = upload_page(db->pages[(size_t)page], db->mem[(size_t)slot], stream);
    if (rc) return rc;
    PRB_HIP(hipEventRecord(db->slot_ready[(size_t)slot], stream));
    db->page_in_slot[(size_t)slot] = page;
    db->slot_of_page[(size_t)page] = slot;
    db->uploads++;
  }
  db->slot_used[(size_t)slot] = ++db->clock;
  *slot_out = slot;
  return PRB_OK;
}
} // namespace prb

extern "C" {

int prb_db_open_streaming(prb_ctx *ctx, const char *prefix, int32_t max_resident_pages, prb_db **out) {
  if (!ctx || !prefix || !out || max_resident_pages < 0) return PRB_ERR_ARG;
  *out = nullptr;
  auto *db = new prb_db();
  db->ctx = ctx;
  std::string err;
  try {
    err = read_db(prefix, db->hdr, db->pages);
  } catch (const std::exception &e) { // (no exception leaves the C ABI)
    err = std::string("Error: cannot load the database: ") + e.what();
  }
  if (!err.empty()) {
    set_error(err);
    delete db;
    return PRB_ERR_IO;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) {
    delete db;
    return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
  }
  const size_t np = db->pages.size();
  const size_t nslots = max_resident_pages == 0 ? np : std::min<size_t>(np, (size_t)max_resident_pages);
  db->mem.resize(nslots);
  db->page_in_slot.assign(nslots, -1);
  db->slot_used.assign(nslots, 0);
  db->slot_of_page.assign(np, -1);
  db->slot_ready.assign(nslots, nullptr);
  int rc = PRB_OK;
  for (size_t k = 0; k < nslots && rc == PRB_OK; k++)
    if (hipEventCreateWithFlags(&db->slot_ready[k], hipEventDisableTiming) != hipSuccess) rc = PRB_ERR_HIP;
  if (rc == PRB_OK && nslots < np) {
    // streaming: uploads of the next page run beside the search on a stream of their own, from page-locked memory
    if (hipStreamCreateWithFlags(&db->copy_stream, hipStreamNonBlocking) != hipSuccess) rc = PRB_ERR_HIP;
    for (DbPage &pg : db->pages) {
      if (rc != PRB_OK) break;
      auto pin = [&](void *p, size_t bytes) {
        if (bytes && hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) rc = PRB_ERR_HIP;
      };
      pin(pg.seqs.data(), pg.seqs.size());
      pin(pg.sa.data(), pg.sa.size() * 4);
      pin(pg.acc.data(), pg.acc.size() * 4);
      pin(pg.cond.data(), pg.cond.size() * 4);
    }
    db->pinned = rc == PRB_OK;
    if (rc != PRB_OK) set_error("prb_db_open: cannot set up page streaming (stream / page-locked host memory)");
  }
  // the first pages are resident from the start
  for (size_t i = 0; i < nslots && rc == PRB_OK; i++) {
    int slot = -1;
    rc = page_slot(ctx, db, (int)i, -1, ctx->stream, &slot);
  }
  if (rc == PRB_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PRB_ERR_HIP;
  if (rc != PRB_OK) {
    prb_db_close(db);
    return rc;
  }
  db->tabs.resize(np);
  for (size_t i = 0; i < np; i++) {
    const DbPage &pg = db->pages[i];
    db->tabs[i] = SeqTable{pg.names, pg.seq_length, pg.seq_length_rep, pg.start_pos};
  }
  *out = db;
  return PRB_OK;
}

int prb_db_open(prb_ctx *ctx, const char *prefix, prb_db **out) {
  const char *e = getenv("PRB_DB_RESIDENT_PAGES"); // 0 / unset: every page resident
  return prb_db_open_streaming(ctx, prefix, e ? std::max(0, atoi(e)) : 0, out);
}

int64_t prb_db_page_uploads(const prb_db *db) { return db ? db->uploads : -1; }

void prb_db_close(prb_db *db) {
  if (!db) return;
  (void)hipSetDevice(db->ctx->device);
  (void)hipStreamSynchronize(db->ctx->stream);
  if (db->copy_stream) {
    (void)hipStreamSynchronize(db->copy_stream);
    (void)hipStreamDestroy(db->copy_stream);
  }
  for (hipEvent_t e : db->slot_ready)
    if (e) (void)hipEventDestroy(e);
  if (db->pinned)
    for (DbPage &pg : db->pages) {
      if (!pg.seqs.empty()) (void)hipHostUnregister(pg.seqs.data());
      if (!pg.sa.empty()) (void)hipHostUnregister(pg.sa.data());
      if (!pg.acc.empty()) (void)hipHostUnregister(pg.acc.data());
      if (!pg.cond.empty()) (void)hipHostUnregister(pg.cond.data());
    }
  for (auto &m : db->mem)
    for (DevBuf *b : {&m.seqs, &m.sa, &m.sa_seq, &m.blk_seq, &m.start_pos, &m.seq_length, &m.acc, &m.cond}) b->release();
  delete db;
}

int prb_db_info(const prb_db *db, int32_t *hash_size, int32_t *repeat_flag, int32_t *maximal_span,
                int32_t *min_accessible_length, int32_t *npages) {
  if (!db) return PRB_ERR_ARG;
  if (hash_size) *hash_size = db->hdr.hash_size;
  if (repeat_flag) *repeat_flag = db->hdr.repeat_flag;
  if (maximal_span) *maximal_span = db->hdr.maximal_span;
  if (min_accessible_length) *min_accessible_length = db->hdr.min_accessible_length;
  if (npages) *npages = (int32_t)db->pages.size();
  return PRB_OK;
}

int prb_db_page_info(const prb_db *db, int32_t page, int32_t *nseq, int64_t *nchars) {
  if (!db || page < 0 || page >= (int32_t)db->pages.size()) return PRB_ERR_ARG;
  if (nseq) *nseq = db->pages[page].nseq;
  if (nchars) *nchars = (int64_t)db->pages[page].seqs.size();
  return PRB_OK;
}

const char *prb_db_seq_name(const prb_db *db, int32_t page, int32_t id) {
  if (!db || page < 0 || page >= (int32_t)db->pages.size()) return nullptr;
  const DbPage &pg = db->pages[page];
  if (id < 0 || id >= pg.nseq) return nullptr;
  return pg.names[id].c_str();
}

int prb_db_seq_lengths(const prb_db *db, int32_t page, int32_t id, int32_t *length, int32_t *length_unmasked,
                       int32_t *start_pos) {
  if (!db || page < 0 || page >= (int32_t)db->pages.size()) return PRB_ERR_ARG;
  const DbPage &pg = db->pages[page];
  if (id < 0 || id >= pg.nseq) return PRB_ERR_ARG;
  if (length) *length = pg.seq_length[id];
  if (length_unmasked) *length_unmasked = pg.seq_length_rep[id];
  if (start_pos) *start_pos = pg.start_pos[id];
  return PRB_OK;
}

// DbConstruction::Run (db_construction.cpp:37-83) as a tool: accessibilities on the GPU
// (the same Raccess kernels as for queries), suffix array and k-mer table on the host.
int prb_db_build(prb_ctx *ctx, const char *prefix, int32_t nseq, const char *const *names, const char *seqs,
                 const int64_t *offsets, int32_t repeat_flag, int32_t hash_size, int32_t maximal_span,
                 int32_t min_accessible_length, int32_t page_size) {
  if (!ctx || !prefix || nseq <= 0 || !names || !seqs || !offsets || repeat_flag < 0 || repeat_flag > 2 ||
      hash_size < 1 || hash_size > 12 || page_size < 1) {
    set_error("prb_db_build: bad argument");
    return PRB_ERR_ARG;
  }
  const int64_t total = offsets[nseq] - offsets[0];
  std::vector<float> acc((size_t)std::max<int64_t>(total, 1)), cond((size_t)std::max<int64_t>(total, 1));
  int rc = prb_accessibility(ctx, nseq, seqs, offsets, maximal_span, min_accessible_length, acc.data(), cond.data());
  if (rc) return rc;
  DbHeader hdr{hash_size, repeat_flag, maximal_span, min_accessible_length};
  DbWriter w;
  std::string err = w.open(prefix, hdr);
  if (!err.empty()) {
    set_error(err);
    return PRB_ERR_IO;
  }
  Encoder enc(repeat_flag);
  for (int32_t first = 0; first < nseq; first += page_size) {
    const int32_t n = std::min(page_size, nseq - first);
    DbPage pg;
    pg.nseq = n;
    int64_t t = 0;
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = first + k;
      const int64_t L = offsets[i + 1] - offsets[i];
      pg.seq_length.push_back((int32_t)L);
      pg.start_pos.push_back((int32_t)t);
      t += L + 1;
      enc.append_db(seqs + offsets[i], L, pg.seqs);
      pg.names.push_back(names[i]);
      // the file stores cond[0..delta) = 0 and the conditional value of window i at i+delta
      // (raccess.cpp:462-480): the in-memory layout of stage 1 already has that shape
      pg.acc.insert(pg.acc.end(), acc.begin() + (offsets[i] - offsets[0]), acc.begin() + (offsets[i + 1] - offsets[0]));
      pg.cond.insert(pg.cond.end(), cond.begin() + (offsets[i] - offsets[0]), cond.begin() + (offsets[i + 1] - offsets[0]));
    }
    if (t > INT32_MAX) {
      set_error("database page exceeds 2^31 characters: use a smaller page size");
      return PRB_ERR_ARG;
    }
    pg.sa.resize(pg.seqs.size());
    suffix_array(pg.seqs.data(), (int32_t)pg.seqs.size(), pg.sa.data());
    build_kmer_table(pg.seqs, pg.sa, hash_size, pg.start_hash, pg.end_hash);
    err = w.append_page(pg, min_accessible_length);
    if (!err.empty()) {
      set_error(err);
      return PRB_ERR_IO;
    }
  }
  // the band tables of a whole database build (tens of GB) are not what the query batches that follow need
  ctx->ra_band.release();
  ctx->ra_vec.release();
  return PRB_OK;
}

// -------------------------------------------------------------------- query batches
int prb_qbatch_create(prb_ctx *ctx, int32_t nq, const char *seqs, const int64_t *offsets, int32_t repeat_flag,
                      prb_qbatch **out) {
  if (!ctx || nq <= 0 || !seqs || !offsets || !out || repeat_flag < 0 || repeat_flag > 2) {
    set_error("prb_qbatch_create: bad argument");
    return PRB_ERR_ARG;
  }
  *out = nullptr;
  auto *qb = new prb_qbatch();
  qb->ctx = ctx;
  qb->nq = nq;
  qb->repeat_flag = repeat_flag;
  qb->off.resize(nq + 1);
  qb->len.resize(nq);
  qb->len_unmasked.resize(nq);
  int64_t t = 0;
  for (int32_t q = 0; q < nq; q++) {
    const int64_t L = offsets[q + 1] - offsets[q];
    if (L < 0 || L > (1 << 30)) {
      delete qb;
      set_error("prb_qbatch_create: bad offsets");
      return PRB_ERR_ARG;
    }
    qb->off[q] = t;
    qb->len[q] = (int32_t)L;
    t += L + 1;
  }
  qb->off[nq] = t;
  qb->seqs.assign((size_t)t, 0);
  qb->enc.assign((size_t)t, 0);
  qb->sa.assign((size_t)t, 0);
  Encoder enc(repeat_flag);
#pragma omp parallel for schedule(dynamic, 4) num_threads(host_threads(nq))
  for (int32_t q = 0; q < nq; q++) {
    const int64_t o = qb->off[q];
    const int32_t L = qb->len[q];
    std::memcpy(qb->seqs.data() + o, seqs + offsets[q], (size_t)L);
    enc.encode_query(seqs + offsets[q], L, qb->enc.data() + o);
    suffix_array(qb->enc.data() + o, L + 1, qb->sa.data() + o);
    int32_t c = 0;
    for (int32_t k = 0; k <= L; k++) c += qb->enc[o + k] >= 2 && qb->enc[o + k] <= 5; // rna_interaction_search.cpp:179-183
    qb->len_unmasked[q] = c;
  }
  if (hipError_t e = hipSetDevice(ctx->device); e != hipSuccess) {
    delete qb;
    return hip_fail(e, "hipSetDevice");
  }
  int rc = 0;
  const size_t n = (size_t)t;
  if ((rc = qb->d_enc.ensure(n)) || (rc = qb->d_sa.ensure(n * 4)) || (rc = qb->d_acc.ensure(n * 4)) ||
      (rc = qb->d_cond.ensure(n * 4)) || (rc = qb->d_off.ensure((size_t)(nq + 1) * 8)) ||
      (rc = qb->d_len.ensure((size_t)nq * 4))) {
    prb_qbatch_destroy(qb);
    return rc;
  }
  {
    hipError_t e = hipMemcpyAsync(qb->d_enc.p, qb->enc.data(), n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(qb->d_sa.p, qb->sa.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(qb->d_off.p, qb->off.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(qb->d_len.p, qb->len.data(), (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(qb->d_acc.p, 0, n * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(qb->d_cond.p, 0, n * 4, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      prb_qbatch_destroy(qb);
      return hip_fail(e, "prb_qbatch_create: upload");
    }
  }
  qb->view.enc = qb->d_enc.as<uint8_t>();
  qb->view.sa = qb->d_sa.as<int32_t>();
  qb->view.acc = qb->d_acc.as<float>();
  qb->view.cond = qb->d_cond.as<float>();
  qb->view.off = qb->d_off.as<int64_t>();
  qb->view.len = qb->d_len.as<int32_t>();
  qb->view.nq = nq;
  *out = qb;
  return PRB_OK;
}

void prb_qbatch_destroy(prb_qbatch *qb) {
  if (!qb) return;
  for (DevBuf *b : {&qb->d_enc, &qb->d_sa, &qb->d_acc, &qb->d_cond, &qb->d_off, &qb->d_len}) b->release();
  delete qb;
}

int prb_qbatch_accessibility(prb_ctx *ctx, prb_qbatch *qb, int32_t maximal_span, int32_t min_accessible_length) {
  if (!ctx || !qb || qb->ctx->device != ctx->device) return PRB_ERR_ARG;
  const size_t n = (size_t)qb->off[qb->nq];
  PRB_HIP(hipSetDevice(ctx->device));
  PRB_HIP(hipMemsetAsync(qb->d_acc.p, 0, n * 4, ctx->stream));
  PRB_HIP(hipMemsetAsync(qb->d_cond.p, 0, n * 4, ctx->stream));
  int rc = run_accessibility(ctx, qb->nq, qb->seqs.data(), qb->off.data(), qb->len.data(), qb->off.data(), maximal_span,
                             min_accessible_length, qb->d_acc.as<float>(), qb->d_cond.as<float>());
  if (rc) return rc;
  qb->have_acc = true;
  qb->W = maximal_span;
  qb->delta = min_accessible_length;
  return PRB_OK;
}

int prb_qbatch_get(prb_qbatch *qb, int32_t q, uint8_t *enc, int32_t *sa, float *acc, float *cond) {
  if (!qb || q < 0 || q >= qb->nq) return PRB_ERR_ARG;
  const int64_t o = qb->off[q];
  const int32_t L = qb->len[q];
  if (enc) std::memcpy(enc, qb->enc.data() + o, (size_t)L + 1);
  if (sa) std::memcpy(sa, qb->sa.data() + o, ((size_t)L + 1) * 4);
  if (acc || cond) {
    if (!qb->have_acc) {
      set_error("prb_qbatch_get: accessibilities not computed yet");
      return PRB_ERR_STATE;
    }
    PRB_HIP(hipSetDevice(qb->ctx->device));
    if (acc && L) PRB_HIP(hipMemcpy(acc, qb->d_acc.as<float>() + o, (size_t)L * 4, hipMemcpyDeviceToHost));
    if (cond && L) PRB_HIP(hipMemcpy(cond, qb->d_cond.as<float>() + o, (size_t)L * 4, hipMemcpyDeviceToHost));
  }
  return PRB_OK;
}

int32_t prb_qbatch_length_unmasked(const prb_qbatch *qb, int32_t q) {
  if (!qb || q < 0 || q >= qb->nq) return -1;
  return qb->len_unmasked[q];
}

} // extern "C"

namespace prb {
std::unique_ptr<SeedPlan> start_seed_plan(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page, int32_t max_seed_length,
                                          double hybrid_threshold) {
  std::unique_ptr<SeedPlan> pl(new SeedPlan());
  SeedPlan *P = pl.get();
  const int32_t nq = qb->nq;
  P->db = db;
  P->page = page;
  P->nq = nq;
  P->max_seed_length = max_seed_length;
  P->hybrid_threshold = hybrid_threshold;
  P->per_q.resize((size_t)nq);
  P->qpairs.assign((size_t)nq, 0);
  P->qrows.assign((size_t)nq, 0);
  P->qents.assign((size_t)nq, 0);
  P->done.reset(new std::atomic<int>[(size_t)nq]);
  for (int32_t q = 0; q < nq; q++) P->done[q].store(0, std::memory_order_relaxed);
  const EnergyParams *params = &ctx->params;
  const DbPage *pg = &db->pages[(size_t)page];
  const int hash_size = db->hdr.hash_size, delta = db->hdr.min_accessible_length;
  P->producer = std::thread([P, qb, params, pg, hash_size, delta, nq] {
    const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel num_threads(host_threads(nq))
    for (;;) {
      const int32_t q = P->next_query.fetch_add(1, std::memory_order_relaxed);
      if (q >= nq) break;
      seed_dfs(*params, qb->enc.data() + qb->off[q], qb->len[q] + 1, qb->sa.data() + qb->off[q], *pg, hash_size, P->max_seed_length, delta,
               P->hybrid_threshold, P->per_q[q]);
      double pairs = 0;
      int64_t rows = 0, ents = 0;
      for (auto &c : P->per_q[q]) {
        c.query = q;
        pairs += (double)(c.ep_q - c.sp_q + 1) * (double)(c.ep_db - c.sp_db + 1);
        rows += (int64_t)c.ep_db - c.sp_db + 1;
        ents += (int64_t)c.ep_q - c.sp_q + 1;
      }
      P->qpairs[q] = pairs;
      P->qrows[q] = rows;
      P->qents[q] = ents;
      P->done[q].store(1, std::memory_order_release);
    }
    P->dfs_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
  return pl;
}
} // namespace prb

extern "C" {

int prb_qbatch_seed_search_begin(prb_ctx *ctx, prb_qbatch *qb, const prb_db *db, int32_t page, const prb_ris_opts *opts) {
  if (!ctx || !qb || !db || !opts || page < 0 || page >= (int32_t)db->pages.size() || opts->max_seed_length < 1 ||
      opts->max_seed_length > 63 || qb->repeat_flag != db->hdr.repeat_flag) {
    set_error("prb_qbatch_seed_search_begin: bad argument");
    return PRB_ERR_ARG;
  }
  try {
    qb->plan = start_seed_plan(ctx, qb, db, page, opts->max_seed_length, opts->hybrid_threshold); // (an unused earlier one is joined and dropped)
  } catch (const std::exception &e) {
    set_error(std::string("prb_qbatch_seed_search_begin: ") + e.what());
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}

} // extern "C"
