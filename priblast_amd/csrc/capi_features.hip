// C ABI, part 15: the annotation of a database and the feature table of one batch - per (query, annotated feature of a
// target), the `-t` summary over the final hits whose span meets the feature (prb_annot_*, prb_featset_*, `ris -t -A
// FILE`).  The kernels are in feature_kernels.hip.  Every check of a call is made on the host before anything is
// enqueued: a refused call leaves the table as it was.
#include <numeric>

#include "capi_tables.hpp"

using namespace prb;

namespace {

const char *const kFinishFn = "prb_featset_finish";
const char *const kBadHit = "a hit merged into this feature table named a query or a sequence outside it, or its span left its sequence";
constexpr int64_t kFirstRoom = 4096; // records a new table has room for

// the block with room for `need` records (at least twice what it had), what it holds kept; on the table's device
int grow_block(prb_ctx *ctx, prb_featset *fs, int64_t need) {
  if (need <= fs->cap) return PRB_OK;
  const int64_t cap = std::max({need, 2 * fs->cap, kFirstRoom});
  ScratchBuf wider;
  if (wider.ensure(fs->head_bytes() + (size_t)cap * sizeof(prb_feature_pair)) != PRB_OK)
    return refuse("prb_featset", "can't allocate the feature table's records (" + std::to_string(cap) + " of them)", PRB_ERR_NOMEM);
  PRB_HIP(hipMemcpyAsync(wider.p, fs->table.p, fs->bytes(), hipMemcpyDeviceToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  std::swap(static_cast<DevBuf &>(wider), fs->table); // (the scratch buffer lets the old block go)
  fs->cap = cap;
  return PRB_OK;
}

// a feature table back to empty, on its own device and stream
int clear_feature_table(prb_featset &fs) {
  PRB_HIP(hipSetDevice(fs.ctx->device));
  PRB_HIP(hipMemsetAsync(fs.table.p, 0, fs.head_bytes(), fs.ctx->stream));
  PRB_HIP(hipStreamSynchronize(fs.ctx->stream));
  fs.nrec = 0;
  fs.unassigned = 0;
  return PRB_OK;
}

FeatWork work_of(const prb_featset *fs) {
  uint32_t *flags = fs->badflag.as<uint32_t>(); // bad, nlong, the 64-bit count of unassigned hits
  return FeatWork{fs->cnt.as<int32_t>(), fs->ioff.as<int64_t>(), fs->tmp.p, fs->flag.as<uint8_t>(), fs->long_list.as<uint32_t>(), flags + 1, flags};
}

} // namespace

// prb_featset_add_hits / prb_fnullset_add_hits: the caller's list against page g and a batch of nq queries, on the host -
// a refused call leaves the table as it was -, as columns
int prb::check_hit_list(const std::string &fn, const prb_annot::Page &g, int32_t nq, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                        int64_t npairs, HitColumns &c) {
  const int32_t nseq = (int32_t)g.slo.size();
  try {
    c.query.resize((size_t)nhits);
    c.db_id.resize((size_t)nhits);
    c.e_tot.resize((size_t)nhits);
    c.e_acc.resize((size_t)nhits);
    c.e_hyb.resize((size_t)nhits);
    c.ends.resize((size_t)nhits * 4);
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  for (int64_t i = 0; i < nhits; i++) {
    const prb_hit &x = hits[i];
    if (x.query < 0 || x.query >= nq || (i && x.query < hits[i - 1].query) || x.db_id < 0 || x.db_id >= nseq || x.bp_count < 1 ||
        x.bp_offset < 0 || x.bp_offset + x.bp_count > npairs)
      return refuse(fn, "hit record " + std::to_string(i) + " is inconsistent");
    const int32_t *first = basepairs + 2 * x.bp_offset, *last = basepairs + 2 * (x.bp_offset + x.bp_count - 1);
    const int64_t lo = std::min(first[1], last[1]), hi = std::max(first[1], last[1]);
    const int64_t s0 = g.slo[(size_t)x.db_id];
    if (lo < s0 || hi >= s0 + g.slen[(size_t)x.db_id])
      return refuse(fn, "the span of hit record " + std::to_string(i) + " leaves its sequence", PRB_ERR_STATE);
    c.query[(size_t)i] = x.query;
    c.db_id[(size_t)i] = x.db_id;
    c.e_tot[(size_t)i] = x.e_tot;
    c.e_acc[(size_t)i] = x.e_acc;
    c.e_hyb[(size_t)i] = x.e_hyb;
    c.ends[4 * (size_t)i] = first[0], c.ends[4 * (size_t)i + 1] = first[1], c.ends[4 * (size_t)i + 2] = last[0], c.ends[4 * (size_t)i + 3] = last[1];
  }
  return PRB_OK;
}
// ... to the device (the current one), in the table's six buffers: query, db_id, e_tot, e_acc, e_hyb, ends
int prb::upload_hit_list(prb_ctx *ctx, const HitColumns &c, DevBuf *const bufs[6], FeatHits *h) {
  const size_t N = c.query.size();
  const void *src[6] = {c.query.data(), c.db_id.data(), c.e_tot.data(), c.e_acc.data(), c.e_hyb.data(), c.ends.data()};
  const size_t bytes[6] = {N * 4, N * 4, N * 8, N * 8, N * 8, N * 16};
  for (int k = 0; k < 6; k++)
    if (int rc = bufs[k]->ensure(bytes[k])) return rc;
  for (int k = 0; k < 6; k++) PRB_HIP(hipMemcpyAsync(bufs[k]->p, src[k], bytes[k], hipMemcpyHostToDevice, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the vectors go)
  *h = FeatHits{(int64_t)N,           bufs[0]->as<int32_t>(), bufs[1]->as<int32_t>(), bufs[2]->as<double>(), bufs[3]->as<double>(),
                bufs[4]->as<double>(), bufs[5]->as<int32_t>()};
  return PRB_OK;
}
// ... and its runs of equal (query, db_id): head flags and the selection of the runs' first hits, two launches
int prb::hit_list_runs(prb_ctx *ctx, const FeatHits &h, DevBuf &head, DevBuf &start, const uint32_t **start_out, int64_t *npairs) {
  int rc;
  SearchWs &ws = ws_of(ctx);
  if ((rc = ws.count.ensure(16)) || (rc = head.ensure((size_t)h.n)) || (rc = start.ensure((size_t)h.n * 4))) return rc;
  PRB_HIP(launch_pair_heads(h.query, h.db_id, h.n, head.as<uint8_t>(), ctx->stream));
  if ((rc = select_flagged(ctx, ws, nullptr, head.as<uint8_t>(), start.as<uint32_t>(), (size_t)h.n, npairs))) return rc;
  *start_out = start.as<uint32_t>();
  return PRB_OK;
}

// prb_search_page_features (per sub-batch) and prb_featset_add_hits: the list's items folded and the ones with a hit
// appended to the block, in a bracket of the "feature" timer.  start == nullptr: the runs of the list - head flags and
// their selection - are made here first.
static int merge_feature_hits(prb_ctx *ctx, prb_featset *fs, int32_t page, const FeatHits &h, const uint32_t *start, int64_t npairs) {
  const char *fn = "prb_search_page_features";
  int rc;
  if (page < 0 || (size_t)page >= fs->annot->pages.size()) return refuse(fn, "page out of range", PRB_ERR_STATE);
  if (h.n <= 0) return PRB_OK;
  if (h.n > (int64_t)UINT32_MAX) return refuse(fn, "a list of " + std::to_string(h.n) + " hits (at most 2^32 - 1)");
  SearchWs &ws = ws_of(ctx);
  const FeatPage pg = fs->annot->page_view((size_t)page);
  if ((rc = ws.count.ensure(16))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  int64_t launches = 0;
  if (!start) {
    if ((rc = hit_list_runs(ctx, h, fs->head, fs->start, &start, &npairs))) return rc;
    launches += 2;
  }
  if (npairs <= 0 || npairs > h.n) return refuse(fn, std::to_string(npairs) + " pair runs for " + std::to_string(h.n) + " hits", PRB_ERR_STATE);
  const size_t N = (size_t)npairs + 1;
  if ((rc = fs->cnt.ensure(N * 4)) || (rc = fs->ioff.ensure(N * 8))) return rc;
  PRB_HIP(hipMemsetAsync(fs->badflag.p, 0, 16, ctx->stream));
  FeatWork w = work_of(fs);
  PRB_HIP(launch_feat_count(h, start, npairs, pg, fs->nq, w, ctx->stream));
  auto counts = rocprim::make_transform_iterator(fs->cnt.as<int32_t>(), ToI64());
  if ((rc = with_temp(fs->scanTmp, "rocprim::exclusive_scan", [&](void *t, size_t &b) {
         return rocprim::exclusive_scan(t, b, counts, fs->ioff.as<int64_t>(), (int64_t)0, N, rocprim::plus<int64_t>(), ctx->stream);
       })))
    return rc;
  PRB_HIP(launch_feat_unassigned(h, pg, fs->nq, w, ctx->stream));
  launches += 3;
  int64_t nitems = 0;
  PRB_HIP(hipMemcpyAsync(&nitems, fs->ioff.as<int64_t>() + npairs, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if (nitems < 0 || nitems > (int64_t)UINT32_MAX)
    return refuse(fn, std::to_string(nitems) + " (pair, feature) items in one sub-batch (at most 2^32 - 1): lower PRB_SEARCH_PAIRS", PRB_ERR_STATE);
  if (nitems > 0) {
    const size_t I = (size_t)nitems;
    if ((rc = fs->tmp.ensure(I * sizeof(prb_feature_pair))) || (rc = fs->flag.ensure(I)) || (rc = fs->long_list.ensure(I * 4)) ||
        (rc = fs->sel.ensure(I * 4)))
      return rc;
    w = work_of(fs);
    PRB_HIP(launch_feat_items(h, start, npairs, nitems, pg, w, ctx->stream));
    PRB_HIP(launch_feat_items_long(h, start, npairs, nitems, pg, w, ctx->stream));
    int64_t nsel = 0;
    if ((rc = select_flagged(ctx, ws, nullptr, fs->flag.as<uint8_t>(), fs->sel.as<uint32_t>(), I, &nsel))) return rc;
    if (nsel < 0 || nsel > nitems) return refuse(fn, "bad record count " + std::to_string(nsel), PRB_ERR_STATE);
    if (nsel) {
      if ((rc = grow_block(ctx, fs, fs->nrec + nsel))) return rc;
      void *b = fs->table.p;
      PRB_HIP(launch_feat_append(fs->tmp.p, fs->sel.as<uint32_t>(), nsel, fs->recs_of(b), fs->nrec, fs->first_of(b), fs->end_of(b), page, fs->nq,
                                 ctx->stream));
      fs->nrec += nsel;
    }
    launches += 4;
  }
  if ((rc = ctx->time_end(ModeTimer::kFeature, launches))) return rc;
  uint64_t flags[2] = {0, 0};
  PRB_HIP(hipMemcpyAsync(flags, fs->badflag.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  if ((uint32_t)flags[0]) {
    fs->bad = true;
    return refuse(fn, kBadHit, PRB_ERR_STATE);
  }
  fs->unassigned += (int64_t)flags[1];
  return PRB_OK;
}
int prb_featset::take(const SubBatch &b) {
  return merge_feature_hits(ctx, this, b.page, FeatHits{b.nfin, b.F.query, b.F.db_id, b.F.e_tot, b.F.e_acc, b.F.e_hyb, b.ends}, b.pair_start, b.npairs);
}

// the selection of prb_featset_finish_top behind the gather, in the same bracket of the "feature" timer: fs->out = the
// gathered records, fs->ioff = the scanned cell offsets.  The counts of chunks and kept records per query, their two
// scans, the chunks' lists, the queries' folds and the gather of the kept records: launches = 6.  *nkept = the records
// that fs->topOut then holds, in (query, rank) order.
static int select_top_records(const char *fn, prb_ctx *ctx, prb_featset *fs, int32_t n, int64_t total, int64_t *nkept) {
  int rc;
  const size_t Q = (size_t)fs->nq + 1;
  if (total >= (int64_t)UINT32_MAX) return refuse(fn, std::to_string(total) + " records in one feature table (at most 2^32 - 2 can be ranked)", PRB_ERR_STATE);
  if ((rc = fs->topCnt.ensure(2 * Q * 8)) || (rc = fs->topOff.ensure(2 * Q * 8)) || (rc = fs->topSel.ensure((size_t)fs->nq * (size_t)n * 4))) return rc;
  const FtopTab t{fs->ioff.as<int64_t>(), fs->badflag.as<uint32_t>(), total, fs->nq, (int32_t)fs->merged.size(), n};
  int64_t *nchunk = fs->topCnt.as<int64_t>(), *nkeep = nchunk + Q, *choff = fs->topOff.as<int64_t>(), *koff = choff + Q;
  PRB_HIP(launch_ftop_counts(t, nchunk, nkeep, ctx->stream));
  for (int k = 0; k < 2; k++)
    if ((rc = with_temp(fs->scanTmp, "rocprim::exclusive_scan", [&](void *tmp, size_t &bytes) {
           return rocprim::exclusive_scan(tmp, bytes, k ? nkeep : nchunk, k ? koff : choff, (int64_t)0, Q, rocprim::plus<int64_t>(), ctx->stream);
         })))
      return rc;
  int64_t sums[2] = {0, 0}; // the chunks, the kept records
  PRB_HIP(hipMemcpyAsync(&sums[0], choff + fs->nq, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipMemcpyAsync(&sums[1], koff + fs->nq, 8, hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t nchunks = sums[0];
  if (nchunks < 1 || nchunks > total / kFtopChunk + fs->nq || sums[1] < 1 || sums[1] > total || sums[1] > (int64_t)fs->nq * n)
    return refuse(fn, "bad counts of the ranked cut: " + std::to_string(nchunks) + " chunks, " + std::to_string(sums[1]) + " records kept of " +
                          std::to_string(total),
                  PRB_ERR_STATE);
  if ((rc = fs->topKey.ensure((size_t)nchunks * (size_t)n * 8)) || (rc = fs->topPlace.ensure((size_t)nchunks * (size_t)n * 4)) ||
      (rc = fs->topOut.ensure((size_t)sums[1] * sizeof(prb_feature_pair))))
    return rc;
  PRB_HIP(launch_ftop_chunks(t, fs->out.p, choff, nchunks, fs->topKey.as<unsigned long long>(), fs->topPlace.as<uint32_t>(), ctx->stream));
  PRB_HIP(launch_ftop_merge(t, choff, nchunks, fs->topKey.as<unsigned long long>(), fs->topPlace.as<uint32_t>(), fs->topSel.as<uint32_t>(), ctx->stream));
  PRB_HIP(launch_ftop_gather(t, fs->out.p, koff, fs->topSel.as<uint32_t>(), sums[1], fs->topOut.p, ctx->stream));
  *nkept = sums[1];
  return PRB_OK;
}

// prb_featset_finish proper, for `fn`: the record counts of the (page, query) cells scanned by query, then page, the
// records gathered in that order, one copy.  n > 0 (prb_featset_finish_top, prb_fnullset_create_top): each query's n
// best of them are selected on the device first, and only those are copied.  keep != nullptr (prb_fnullset_create[_top]):
// before the table's device memory is released, the records that were copied - still on the device - go to
// keep_feature_records (capi_fnull.hip).
int prb::finish_featset(const char *fn, prb_ctx *ctx, prb_featset *fs, int32_t n, prb_fnullset *keep) {
  if (int rc = finish_guard(fn, "feature", ctx, fs)) return rc;
  if (fs->finished) {
    if (fs->top_n == n) return PRB_OK; // (the records are on the host already)
    return refuse(fn, fs->top_n ? "the feature table is finished with each query's " + std::to_string(fs->top_n) + " best records (prb_featset_finish_top)"
                                : std::string("the feature table is finished with all its records (") + kFinishFn + ")",
                  PRB_ERR_STATE);
  }
  if (fs->bad) return refuse(fn, kBadHit, PRB_ERR_STATE);
  fs->recs.clear();
  PRB_HIP(hipSetDevice(ctx->device));
  const int64_t C = fs->cells();
  const void *recs_dev = fs->out.p;
  if (C > 0 && fs->nrec > 0) {
    int rc;
    const int32_t npages = (int32_t)fs->merged.size();
    if ((rc = fs->tmp.ensure(((size_t)C + 1) * 8)) || (rc = fs->ioff.ensure(((size_t)C + 1) * 8)) ||
        (rc = fs->out.ensure((size_t)fs->nrec * sizeof(prb_feature_pair))))
      return rc;
    if ((rc = ctx->time_begin())) return rc;
    void *b = fs->table.p;
    PRB_HIP(hipMemsetAsync(fs->badflag.p, 0, 16, ctx->stream));
    PRB_HIP(launch_feat_cell_counts(fs->first_of(b), fs->end_of(b), npages, fs->nq, fs->tmp.as<int64_t>(), ctx->stream));
    if ((rc = with_temp(fs->scanTmp, "rocprim::exclusive_scan", [&](void *t, size_t &bytes) {
           return rocprim::exclusive_scan(t, bytes, fs->tmp.as<int64_t>(), fs->ioff.as<int64_t>(), (int64_t)0, (size_t)C + 1, rocprim::plus<int64_t>(),
                                          ctx->stream);
         })))
      return rc;
    int64_t total = 0;
    PRB_HIP(hipMemcpyAsync(&total, fs->ioff.as<int64_t>() + C, 8, hipMemcpyDeviceToHost, ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    if (total != fs->nrec) {
      fs->recs.clear();
      return refuse(fn, "bad record count " + std::to_string(total) + " (the table holds " + std::to_string(fs->nrec) + ")", PRB_ERR_STATE);
    }
    PRB_HIP(launch_feat_gather(fs->recs_of(b), fs->nrec, fs->first_of(b), fs->ioff.as<int64_t>(), npages, fs->nq, total, fs->out.p,
                               fs->badflag.as<uint32_t>(), ctx->stream));
    recs_dev = fs->out.p;
    int64_t ncopy = total;
    if (n) {
      if ((rc = select_top_records(fn, ctx, fs, n, total, &ncopy))) return rc;
      recs_dev = fs->topOut.p;
    }
    try {
      fs->recs.resize((size_t)ncopy);
    } catch (const std::exception &e) {
      return refuse(fn, e.what(), PRB_ERR_NOMEM);
    }
    PRB_HIP(hipMemcpyAsync(fs->recs.data(), recs_dev, (size_t)ncopy * sizeof(prb_feature_pair), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ctx->time_end(ModeTimer::kFeature, n ? 9 : 3))) return rc; // (synchronises: the copy is over)
    if ((rc = fetch_bad(ctx, fs))) return rc;
    if (fs->bad) {
      fs->recs.clear();
      return refuse(fn, "a record lies outside the feature table", PRB_ERR_STATE);
    }
  }
  if (keep) // (the copied records are still on the device)
    if (int rc = keep_feature_records(ctx, keep, fs, recs_dev, (int64_t)fs->recs.size())) return rc;
  fs->finished = true;
  fs->top_n = n;
  fs->release(); // (only the host records are needed from here on)
  return PRB_OK;
}


extern "C" {

int prb_annot_create(prb_ctx *ctx, const prb_db *db, int64_t n, const int32_t *page, const int32_t *db_id, const int32_t *start,
                     const int32_t *end, prb_annot **out) {
  const char *fn = "prb_annot_create";
  if (!ctx || !db || !out || n < 0 || n > INT32_MAX || (n && (!page || !db_id || !start || !end)) || db->ctx->device != ctx->device)
    return refuse(fn, "bad argument");
  *out = nullptr;
  const int32_t npages = (int32_t)db->pages.size();
  for (int64_t i = 0; i < n; i++) {
    const std::string entry = "feature " + std::to_string(i);
    if (page[i] < 0 || page[i] >= npages)
      return refuse(fn, entry + ": page " + std::to_string(page[i]) + " out of range (the database has " + std::to_string(npages) + ")");
    const DbPage &pg = db->pages[(size_t)page[i]];
    if (db_id[i] < 0 || db_id[i] >= pg.nseq)
      return refuse(fn, entry + ": db_id " + std::to_string(db_id[i]) + " out of range (page " + std::to_string(page[i]) + " has " +
                            std::to_string(pg.nseq) + " sequences)");
    const int32_t len = pg.seq_length[(size_t)db_id[i]];
    if (start[i] < 0 || start[i] > end[i] || end[i] >= len)
      return refuse(fn, entry + ": need 0 <= start <= end < " + std::to_string(len) + ", the target's length (got " + std::to_string(start[i]) +
                            " and " + std::to_string(end[i]) + ")");
  }
  std::unique_ptr<prb_annot> an(new (std::nothrow) prb_annot());
  if (!an) return refuse(fn, "out of host memory", PRB_ERR_NOMEM);
  std::vector<std::vector<int32_t>> dev((size_t)npages);
  try {
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      if (page[a] != page[b]) return page[a] < page[b];
      if (db_id[a] != db_id[b]) return db_id[a] < db_id[b];
      if (start[a] != start[b]) return start[a] < start[b];
      if (end[a] != end[b]) return end[a] < end[b];
      return a < b;
    });
    an->pages.resize((size_t)npages);
    for (int32_t p = 0; p < npages; p++) {
      const DbPage &pg = db->pages[(size_t)p];
      prb_annot::Page &g = an->pages[(size_t)p];
      g.off.assign((size_t)pg.nseq + 1, 0);
      g.slo.assign(pg.start_pos.begin(), pg.start_pos.begin() + pg.nseq);
      g.slen.assign(pg.seq_length.begin(), pg.seq_length.begin() + pg.nseq);
    }
    for (int32_t i : order) {
      prb_annot::Page &g = an->pages[(size_t)page[i]];
      g.off[(size_t)db_id[i] + 1]++;
      g.start.push_back(start[i]);
      g.end.push_back(end[i]);
      g.idx.push_back(i);
    }
    for (int32_t p = 0; p < npages; p++) {
      prb_annot::Page &g = an->pages[(size_t)p];
      for (size_t d = 0; d + 1 < g.off.size(); d++) g.off[d + 1] += g.off[d];
      // what the device reads: off, slo, slen, then the features' ends in the page's text (which holds the sequences
      // reversed) and their indices
      std::vector<int32_t> &v = dev[(size_t)p];
      v.insert(v.end(), g.off.begin(), g.off.end());
      v.insert(v.end(), g.slo.begin(), g.slo.end());
      v.insert(v.end(), g.slen.begin(), g.slen.end());
      const size_t nf = g.idx.size();
      std::vector<int32_t> tlo(nf), thi(nf);
      for (size_t d = 0; d + 1 < g.off.size(); d++)
        for (int32_t f = g.off[d]; f < g.off[d + 1]; f++) {
          tlo[(size_t)f] = g.slo[d] + g.slen[d] - 1 - g.end[(size_t)f];
          thi[(size_t)f] = g.slo[d] + g.slen[d] - 1 - g.start[(size_t)f];
        }
      v.insert(v.end(), tlo.begin(), tlo.end());
      v.insert(v.end(), thi.begin(), thi.end());
      v.insert(v.end(), g.idx.begin(), g.idx.end());
    }
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  an->n = n;
  an->db = db;
  an->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  PRB_HIP(hipSetDevice(ctx->device));
  for (int32_t p = 0; p < npages; p++) {
    const std::vector<int32_t> &v = dev[(size_t)p];
    if (an->pages[(size_t)p].dev.ensure(std::max<size_t>(v.size() * 4, 16)) != PRB_OK)
      return refuse(fn, "can't allocate the annotation of page " + std::to_string(p), PRB_ERR_NOMEM);
    PRB_HIP(hipMemcpyAsync(an->pages[(size_t)p].dev.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  PRB_HIP(hipStreamSynchronize(ctx->stream)); // (pageable memory: the vectors go)
  *out = an.release();
  return PRB_OK;
}

int64_t prb_annot_count(const prb_annot *an) { return an ? an->n : -1; }
void prb_annot_free(prb_annot *an) { delete an; }

int prb_featset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_annot *an, prb_featset **out) {
  const char *fn = "prb_featset_create";
  std::unique_ptr<prb_featset> fs;
  const bool args_ok = ctx && qb && an && qb->ctx->device == ctx->device && an->ctx->device == ctx->device;
  if (int rc = new_table(fn, args_ok, out, fs)) return rc;
  try {
    fs->merged.assign(an->pages.size(), 0);
    fs->qlen = qb->len;
  } catch (const std::exception &e) {
    return refuse(fn, e.what(), PRB_ERR_NOMEM);
  }
  fs->nq = qb->nq;
  fs->annot = an;
  fs->ctx = ctx; // (from here on the destructor has a device and a stream to release under)
  fs->db = an->db;
  fs->qb = qb;
  fs->cap = kFirstRoom;
  PRB_HIP(hipSetDevice(ctx->device));
  if (fs->table.ensure(std::max<size_t>(fs->head_bytes() + (size_t)fs->cap * sizeof(prb_feature_pair), 16)) != PRB_OK ||
      fs->badflag.ensure(16) != PRB_OK)
    return refuse(fn, "can't allocate the feature table (" + std::to_string(fs->cells()) + " (page, query) cells)", PRB_ERR_NOMEM);
  PRB_HIP(hipMemsetAsync(fs->badflag.p, 0, 16, ctx->stream));
  if (int rc = clear_feature_table(*fs)) return rc;
  *out = fs.release();
  return PRB_OK;
}

int prb_search_page_features(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_featset *fs) {
  const char *fn = "prb_search_page_features";
  if (fs && fs->bad) return refuse(fn, kBadHit, PRB_ERR_STATE);
  return merge_page(fn, "feature", kFinishFn, fs, ctx, qb, db, page, opts);
}

// the caller's list checked on the host - a refused call leaves the table as it was -, then as columns to the device and
// through the fold of a sub-batch
int prb_featset_add_hits(prb_ctx *ctx, prb_featset *fs, int32_t page, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                         int64_t npairs) {
  const std::string fn = "prb_featset_add_hits";
  if (!ctx || !fs || nhits < 0 || nhits > INT32_MAX || npairs < 0 || (nhits && (!hits || !basepairs))) return refuse(fn, "bad argument");
  if (fs->ctx != ctx) return refuse(fn, "the feature table was made with another context");
  if (fs->broken) return refuse(fn, "an earlier merge into this feature table failed", PRB_ERR_STATE);
  if (fs->bad) return refuse(fn, kBadHit, PRB_ERR_STATE);
  if (fs->finished) return refuse(fn, std::string("the feature table is finished (") + kFinishFn + ")", PRB_ERR_STATE);
  if (page < 0 || (size_t)page >= fs->merged.size())
    return refuse(fn, "page " + std::to_string(page) + " out of range (the database has " + std::to_string(fs->merged.size()) + ")");
  if (fs->merged[(size_t)page]) return refuse(fn, "page " + std::to_string(page) + " is already merged into this feature table");
  HitColumns cols;
  if (int rc = check_hit_list(fn, fs->annot->pages[(size_t)page], fs->nq, hits, nhits, basepairs, npairs, cols)) return rc;
  DeviceScope restore;
  PRB_HIP(hipSetDevice(ctx->device));
  fs->merged[(size_t)page] = 1;
  if (!nhits) return PRB_OK;
  fs->broken = true; // (until the merge is whole)
  int rc;
  FeatHits h;
  DevBuf *const bufs[6] = {&fs->h_query, &fs->h_db_id, &fs->h_e_tot, &fs->h_e_acc, &fs->h_e_hyb, &fs->h_ends};
  if ((rc = upload_hit_list(ctx, cols, bufs, &h))) return rc;
  if ((rc = merge_feature_hits(ctx, fs, page, h, nullptr, 0))) return rc;
  fs->broken = false;
  return PRB_OK;
}

int prb_featset_merge(prb_ctx *ctx, prb_featset *dst, prb_featset *src) {
  const char *fn = "prb_featset_merge";
  if (int rc = merge_tables_guard(fn, "feature", ctx, dst, src)) return rc;
  if (dst->bad || src->bad) return refuse(fn, kBadHit, PRB_ERR_STATE);
  if (dst->annot != src->annot && !(dst->annot->pages == src->annot->pages))
    return refuse(fn, "the feature tables were made with different annotations");
  const prb_db *db = src->db;
  const size_t npages = src->merged.size();
  const int64_t nsrc = src->nrec, src_unassigned = src->unassigned;
  const int rc = join_tables(
      fn, ModeTimer::kFeature, 1, ctx, dst, src, src->bytes(), [&]() -> int { return grow_block(ctx, dst, dst->nrec + nsrc); },
      [&](void *block) -> int {
        void *b = dst->table.p;
        PRB_HIP(launch_feat_join(dst->recs_of(b), dst->nrec, dst->first_of(b), dst->end_of(b), src->recs_of(block), nsrc, src->first_of(block),
                                 src->end_of(block), dst->cells(), ctx->stream));
        dst->nrec += nsrc;
        dst->unassigned += src_unassigned;
        return PRB_OK;
      },
      clear_feature_table);
  // (src stays a table of its database, with no page merged: it can be finished to zero records)
  src->db = db;
  src->merged.assign(npages, 0);
  return rc;
}

int prb_featset_finish(prb_ctx *ctx, prb_featset *fs) { return finish_featset(kFinishFn, ctx, fs, 0, nullptr); }
int prb_featset_finish_top(prb_ctx *ctx, prb_featset *fs, int32_t n) {
  const char *fn = "prb_featset_finish_top";
  if (const std::string why = bad_n(n); !why.empty()) return refuse(fn, why);
  return finish_featset(fn, ctx, fs, n, nullptr);
}

int64_t prb_featset_size(const prb_featset *fs) { return fs ? (int64_t)fs->recs.size() : -1; }
const prb_feature_pair *prb_featset_records(const prb_featset *fs) { return fs ? fs->recs.data() : nullptr; }
void prb_featset_counts(const prb_featset *fs, int64_t counts[3]) {
  for (int i = 0; i < 3; i++) counts[i] = fs ? fs->counts[i] : 0;
}
int64_t prb_featset_unassigned(const prb_featset *fs) { return fs ? fs->unassigned : -1; }
void prb_featset_free(prb_featset *fs) { delete fs; }

} // extern "C"
