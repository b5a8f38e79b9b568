// What the host units of the search share (capi_pages.hip, capi_search.hip, capi_gapped.hip, capi_top.hip,
// capi_targets.hip, capi_grouprank.hip, capi_featrank.hip, capi_spans.hip, capi_lines.hip): the objects behind the C ABI's handles, the workspace of the search stages, and the
// rocPRIM idioms they all use.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include <rocprim/rocprim.hpp>

#include "../../include/priblast_hip.h"
#include "context.hpp"
#include "db_format.hpp"
#include "hitset.hpp"
#include "output.hpp"
#include "search_kernels.hpp"
#include "seed_dfs.hpp"

namespace prb {

struct SearchConstMem {
  DevBuf ints, bulge;
  SearchConst view{};
};

struct PageMem {
  DevBuf seqs, sa, sa_seq, blk_seq, start_pos, seq_length, acc, cond;
  PageDev view{};
};

// The device buffers of the search stages, reused across prb_search_page calls: X(name, trimmable), the one list that
// the members, trim() and release() come from.  Not trimmable (SearchWs::trim): `packed`, which may still be on its way to
// the host, and the three 16-byte cells `pending`, `count`, `resumeCount`, which never reach the limit.  `resumeSlot`
// (12 B per hit of a gapped chunk) and `accScratch` are spared as well, for no reason on record: they look like
// omissions from the list, and stay spared here only because this list restates what was there.
#define PRB_SEARCH_BUFFERS(X)                                                                                                   \
  X(cands, 1) X(row_count, 1) X(row_off, 1) X(row_cand, 1) X(seed_qacc, 1)                             /* seeds */              \
  X(hitsA, 1) X(hitsB, 1) X(hitsC, 1) X(hitsTmp, 1)                                                    /* hit lists */          \
  X(kE, 1) X(kL, 1) X(kQ, 1) X(kP, 1) X(kTmp, 1) X(kTmp2, 1) X(idxA, 1) X(idxB, 1) X(sortTmp, 1)       /* sort */               \
  X(endKey, 1) X(pmax, 1) X(state, 1) X(keep, 1) X(pending, 0) X(surv, 1) X(count, 0) X(scanTmp, 1)    /* filter, select */     \
  X(first, 1) X(cidx, 1)                                                                                                        \
  X(gapScratch, 1) X(overflow, 1) X(tierOf, 1) X(listA, 1) X(listB, 1) X(listC, 1) X(ntrace, 1) X(trace, 1) /* gapped */        \
  X(frontScratch, 1) X(accScratch, 0)                                                                                           \
  X(resumeSlot, 0) X(resumeCount, 0)                                                                                            \
  X(slowList, 1) X(slowSlot, 1) X(slowCnt, 1) X(slowTrace, 1)                                                                   \
  X(keptU, 1) X(keptFirst, 1) X(keptTier, 1) X(keptNtrace, 1) X(keptTrace, 1)                          /* chunked gapped */     \
  X(subset, 1) X(subset2, 1) X(tierFin, 1) X(ntraceFin, 1)                                             /* traceback */          \
  X(bpCount, 1) X(bpOff, 1) X(bpOff2, 1) X(bpOut, 1) X(bpEnds, 1)                                                               \
  X(packed, 0) X(pairHead, 1) X(pairStart, 1)                                                          /* results */

struct SearchWs {
#define X(name, trimmable) DevBuf name;
  PRB_SEARCH_BUFFERS(X)
#undef X
  DevBuf resumePool[kLdsTiers - 1]; // resumePool[t]: the state dumps of the hits that outgrow LDS tier t (trimmable)
  // The front of the one-pass seed path for a chunk of candidates - candidates and their pair offsets on the device,
  // query-side window sums, the pairs' keys and values in the chunk's layout (`lay`: 4 + 4 bytes per pair and buffer in
  // the narrow one, up to 8 + 8 in the wide one), sorted - in buffers of its own, so that it can be issued for
  // the NEXT sub-batch, on a stream of its own, while this sub-batch is in its last, nearly idle stretch (search_range):
  // ~7 ms of bandwidth-bound work per configs[2] query beside the ~2 ms that the ~150 longest extensions of a query run
  // alone (twice) and the final sort / filter / copies, instead of standing in line behind them.
  struct FrontStage {
    DevBuf cands, seed_qacc, pair0, keyA, keyB, valA, valB, sortTmp;
    PinnedBuf pair0_pin;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool ahead = false;         // holds the first chunk of the sub-batch whose candidates are at `cd`, issued on `stream`
    const CandDev *cd = nullptr;
    int32_t nc = 0;
    int64_t np = 0;
    PairLayout lay;             // how keyA / keyB / valA / valB hold the chunk's pairs
    const void *keys = nullptr, *vals = nullptr; // the sorted pairs (keyB, valB; under a pair mask keyA, valA: the compaction writes the B's)
    // Under a pair mask (issue_front): a ballot word, a count and its scanned offset per 64 pairs, and the number of
    // allowed pairs on its way to the host.  The sort takes that number, so a front issued ahead stops behind the
    // compaction; finish_front sorts what is left when the chunk is taken up.
    DevBuf ballot, wcount, woff, scanTmp;
    PinnedBuf kept_pin;
    bool unsorted = false;      // the compacted pairs are still to be sorted (by `lay`)
    int64_t np_all = 0;         // the chunk's pairs before the compaction
    int init() {
      if (stream) return PRB_OK;
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi); // (lo = the numerically largest = least urgent)
      if (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, lo) != hipSuccess ||
          hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
        set_error("hipStreamCreateWithPriority / hipEventCreate failed (seed front stage)");
        return PRB_ERR_HIP;
      }
      return PRB_OK;
    }
    void release() {
      if (stream) {
        (void)hipStreamSynchronize(stream);
        (void)hipStreamDestroy(stream);
        (void)hipEventDestroy(done);
        stream = nullptr;
      }
      for (DevBuf *b : {&cands, &seed_qacc, &pair0, &keyA, &keyB, &valA, &valB, &sortTmp, &ballot, &wcount, &woff, &scanTmp}) b->release();
      pair0_pin.release();
      kept_pin.release();
      ahead = false;
    }
  } front;
  // results leave on a stream of their own: the next sub-batch does not queue behind 60 MB over PCIe
  hipStream_t copy_stream = nullptr;
  hipEvent_t packed_ready = nullptr, copy_done = nullptr;
  bool copy_pending = false;
  int copy_init() {
    if (copy_stream) return PRB_OK;
    if (hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&packed_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&copy_done, hipEventDisableTiming) != hipSuccess) {
      set_error("hipStreamCreate / hipEventCreate failed (result copies)");
      return PRB_ERR_HIP;
    }
    return PRB_OK;
  }
  PinnedBuf pinned, cand_pinned[2], tb_pinned, pin_hits[2], pin_bp[2];
  bool trim_next = false; // the last sub-batch had a giant list: its buffers are let go before the next one starts
  // every trimmable stage buffer over 256 MB (the front stage's are not touched: they may hold the next sub-batch already)
  void trim() {
#define X(name, trimmable) \
  if (trimmable && name.cap > ((size_t)256 << 20)) name.release();
    PRB_SEARCH_BUFFERS(X)
#undef X
    for (DevBuf &b : resumePool)
      if (b.cap > ((size_t)256 << 20)) b.release();
    trim_next = false;
  }
  void release() {
#define X(name, trimmable) name.release();
    PRB_SEARCH_BUFFERS(X)
#undef X
    for (DevBuf &b : resumePool) b.release();
    front.release();
    if (copy_stream) {
      (void)hipStreamSynchronize(copy_stream);
      (void)hipStreamDestroy(copy_stream);
      (void)hipEventDestroy(packed_ready);
      (void)hipEventDestroy(copy_done);
      copy_stream = nullptr;
    }
    for (PinnedBuf *b : {&pinned, &cand_pinned[0], &cand_pinned[1], &tb_pinned, &pin_hits[0], &pin_hits[1], &pin_bp[0], &pin_bp[1]})
      b->release();
  }
};

inline SearchWs &ws_of(prb_ctx *ctx) {
  if (!ctx->search_ws) ctx->search_ws = new SearchWs();
  return *static_cast<SearchWs *>(ctx->search_ws);
}

// Appends the results of finished sub-batches (pinned staging slots filled by asynchronous
// copies on the compute stream) to the hit set while the GPU already works on the next one.
struct Drainer {
  struct Job {
    int slot;
    int64_t nhits, nbp_ints;
  };
  std::vector<prb_hit> *hits;
  std::vector<int32_t> *bp;
  std::vector<prb_pair_summary> *pairs = nullptr; // summary searches: the slots hold pair records (Job::nhits of them)
  PinnedBuf *pin_hits, *pin_bp; // [2]
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy[2] = {false, false}, stop = false, failed = false;
  // what the whole search is expected to deliver (extrapolated by the submitting thread from the queries done so far):
  // the vectors then grow once instead of doubling five times - each doubling of a list of 1e7 hits is a fresh 1 GB
  // mapping, page faults and a copy, on a thread the next staging slot waits for
  std::atomic<size_t> hint_hits{0}, hint_bp{0};

  Drainer(std::vector<prb_hit> *h, std::vector<int32_t> *b, PinnedBuf *ph, PinnedBuf *pb)
      : hits(h), bp(b), pin_hits(ph), pin_bp(pb) {}
  int start() {
    for (int i = 0; i < 2; i++)
      if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return PRB_ERR_HIP;
    th = std::thread([this] { run(); });
    return PRB_OK;
  }
  void run() {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [this] { return stop || !jobs.empty(); });
        if (jobs.empty()) return;
        j = jobs.front();
        jobs.pop_front();
      }
      if (hipEventSynchronize(ev[j.slot]) != hipSuccess) failed = true;
      if (pairs) {
        const prb_pair_summary *ps = static_cast<const prb_pair_summary *>(pin_hits[j.slot].p);
        pairs->insert(pairs->end(), ps, ps + j.nhits);
      } else {
        const prb_hit *src = static_cast<const prb_hit *>(pin_hits[j.slot].p);
        if (hits->capacity() < hits->size() + (size_t)j.nhits)
          hits->reserve(std::max({2 * hits->capacity(), hits->size() + (size_t)j.nhits, hint_hits.load()}));
        hits->insert(hits->end(), src, src + j.nhits);
        const int32_t *bsrc = static_cast<const int32_t *>(pin_bp[j.slot].p);
        if (bp->capacity() < bp->size() + (size_t)j.nbp_ints)
          bp->reserve(std::max({2 * bp->capacity(), bp->size() + (size_t)j.nbp_ints, hint_bp.load()}));
        bp->insert(bp->end(), bsrc, bsrc + j.nbp_ints);
      }
      { // slot done: the submitting thread may fill it again
        std::lock_guard<std::mutex> lk(m);
        busy[j.slot] = false;
      }
      cv.notify_all();
    }
  }
  // blocks until the staging slot is no longer read by the background thread
  void acquire(int slot) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return !busy[slot]; });
    busy[slot] = true;
  }
  void submit(const Job &j) {
    {
      std::lock_guard<std::mutex> lk(m);
      jobs.push_back(j);
    }
    cv.notify_all();
  }
  int finish() { // everything submitted is in the hit set afterwards
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
    for (int i = 0; i < 2; i++)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    return failed ? PRB_ERR_HIP : PRB_OK;
  }
};

// wall-clock timer for host-side pieces, reported next to the device stage timers (pseudo-stage names "host_*")
struct HostTimer {
  prb_ctx *ctx;
  const char *name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  HostTimer(prb_ctx *c, const char *n) : ctx(c), name(n) {}
  ~HostTimer() {
    auto &t = ctx->timers[name];
    t.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t.launches++;
  }
};

// ---------------------------------------------------------------- rocPRIM idioms
// a 32-bit count as what a 64-bit scan adds up
struct ToI64 {
  __host__ __device__ int64_t operator()(const int32_t &v) const { return (int64_t)v; }
};
// the bits of a sort key's field whose largest value is max_value
inline int bits_for(int64_t max_value) {
  int b = 1;
  while (b < 40 && (int64_t(1) << b) <= max_value) b++;
  return b;
}

// rocPRIM's two calls: `call(nullptr, bytes)` asks for the size of the temporary storage, `tmp` grows to it,
// `call(tmp.p, bytes)` does the work.  (Where several primitives share one temporary buffer within a stream sequence,
// all are sized before the first is enqueued instead - a DevBuf that grows frees memory that work in flight still reads.)
template <class Call> int with_temp(DevBuf &tmp, const char *what, Call &&call) {
  size_t bytes = 0;
  if (hipError_t e = call(nullptr, bytes); e != hipSuccess) return hip_fail(e, what);
  if (int rc = tmp.ensure(bytes)) return rc;
  if (hipError_t e = call(tmp.p, bytes); e != hipSuccess) return hip_fail(e, what);
  return PRB_OK;
}

// one stable radix sort of (key, value) pairs by the bits [begin, end) of the keys
template <class K, class V>
int sort_pairs(hipStream_t s, DevBuf &tmp, const K *kin, K *kout, const V *vin, V *vout, size_t n, unsigned begin, unsigned end) {
  return with_temp(tmp, "rocprim::radix_sort_pairs",
                   [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin, end, s); });
}
// ... by the low `bits` bits of the keys
template <class K, class V>
int sort_pairs(hipStream_t s, DevBuf &tmp, const K *kin, K *kout, const V *vin, V *vout, size_t n, unsigned bits) {
  return sort_pairs(s, tmp, kin, kout, vin, vout, n, 0u, bits);
}

// The layout of a chunk's pairs (PairLayout, search_kernels.hpp) for a page of `nchars` characters, queries that span
// `qspan` (last - first of the chunk) and the knobs PRB_SEED_ROW_SHIFT, PRB_SEED_SORT_BITS, PRB_SEED_LOCAL_ORDER and
// PRB_SEED_PAIR_WIDE.  Narrow when position and query fit 32 bits together.  The radix sort then covers at most
// `sort_bits` bits from the top - two passes of 8 bits by default - and leaves up to kPairLocalBits bits above the row
// shift to the tiles of k_seed_extend: begin = max(shift, kbits - sort_bits), but no more than shift + kPairLocalBits
// (pairs further apart than that within a tile gain nothing from the tile's order: the sort takes those bits, in a
// pass more).  A row shift beyond the position bits sorts by query alone.  row_shift < 0 (suffix-array order: the list
// form takes every chunk): no layout, kbits = 0.
inline PairLayout pair_layout(int64_t nchars, int64_t qspan, int row_shift, int sort_bits, bool local_order, bool force_wide) {
  PairLayout L;
  if (row_shift < 0) return L;
  const int qbits = bits_for(std::max<int64_t>(1, qspan)), pbits = bits_for(std::max<int64_t>(1, nchars - 1));
  if (!force_wide && pbits + qbits <= 32) {
    L.narrow = true;
    L.pbits = pbits;
    L.kbits = pbits + qbits;
    const int shift = std::min(row_shift, pbits);
    L.begin = shift;
    if (local_order) L.begin = std::min(std::max(shift, L.kbits - std::max(sort_bits, 1)), shift + kPairLocalBits);
    L.local_bits = L.begin - shift;
    return L;
  }
  L.shift = row_shift;
  L.pbits = bits_for(std::max<int64_t>(1, (nchars - 1) >> row_shift));
  L.kbits = L.pbits + qbits;
  return L;
}

// out <- the entries of `in` (a list, or nullptr: 0..n-1) whose flag is set, in order; *nsel = how many, copied back
// through w.count (the caller has ensured it) - which synchronises the stream
inline int select_flagged(prb_ctx *ctx, SearchWs &w, const uint32_t *in, const uint8_t *flags, uint32_t *out, size_t n, int64_t *nsel) {
  int rc;
  if (in)
    rc = with_temp(w.scanTmp, "rocprim::select",
                   [&](void *t, size_t &b) { return rocprim::select(t, b, in, flags, out, w.count.as<size_t>(), n, ctx->stream); });
  else
    rc = with_temp(w.scanTmp, "rocprim::select", [&](void *t, size_t &b) {
      return rocprim::select(t, b, rocprim::counting_iterator<uint32_t>(0), flags, out, w.count.as<size_t>(), n, ctx->stream);
    });
  if (rc) return rc;
  size_t cnt = 0;
  PRB_HIP(hipMemcpyAsync(&cnt, w.count.p, sizeof(size_t), hipMemcpyDeviceToHost, ctx->stream));
  PRB_HIP(hipStreamSynchronize(ctx->stream));
  *nsel = (int64_t)cnt;
  return PRB_OK;
}

} // namespace prb

// ---------------------------------------------------------------- the objects behind the handles
struct prb_db {
  prb_ctx *ctx = nullptr;
  prb::DbHeader hdr;
  std::vector<prb::DbPage> pages;
  // Device residency (DbReader::LoadDatabases loads every page eagerly, db_reader.cpp:29-59; here a database
  // larger than HBM - or than the share of it one wants to give it - is streamed): `mem` are slots, at most
  // max_resident of them; a page that is searched is uploaded into a slot if it is not there (the least recently
  // used page makes room), and with two slots or more the NEXT page's upload runs on a copy stream of its own
  // while this one is searched (the host copies are page-locked for that).
  std::vector<prb::PageMem> mem;
  std::vector<int> slot_of_page, page_in_slot;
  std::vector<uint64_t> slot_used; // "time" of the last search that used the slot
  std::vector<hipEvent_t> slot_ready;
  uint64_t clock = 0;
  hipStream_t copy_stream = nullptr;
  bool pinned = false;
  int64_t uploads = 0; // pages uploaded so far (tests)
  std::vector<prb::SeqTable> tabs; // per page: what the result lines print about its sequences
};

namespace prb {
// The seed search proper of a batch against one page (SeedSearch::Run's DFS, seed_search.cpp:153-295): per query,
// on host threads, in the background; a consumer waits for query q with wait_for(q).  It needs the encoded queries,
// their suffix arrays and the page's k-mer table only - not the accessibilities - so it can be started as soon as a
// batch exists (prb_qbatch_seed_search_begin), long before the batch is searched.
struct SeedPlan {
  const prb_db *db = nullptr;
  int32_t page = 0, nq = 0, max_seed_length = 0;
  double hybrid_threshold = 0;
  std::vector<std::vector<SeedCandidate>> per_q;
  std::vector<double> qpairs;
  std::vector<int64_t> qrows, qents;
  std::unique_ptr<std::atomic<int>[]> done;
  std::atomic<int32_t> next_query{0}; // queries are handed out strictly in order: the consumer needs the first ones first
  std::thread producer;
  double dfs_ms = 0;
  ~SeedPlan() {
    if (producer.joinable()) producer.join();
  }
  void wait_for(int32_t q) const {
    while (!done[q].load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
};
} // namespace prb

struct prb_qbatch {
  prb_ctx *ctx = nullptr;
  int32_t nq = 0, repeat_flag = 0;
  std::vector<int64_t> off; // nq + 1; query q occupies [off[q], off[q] + len[q] + 1)
  std::vector<int32_t> len, len_unmasked;
  std::vector<char> seqs;   // same offsets, NUL after each query
  std::vector<uint8_t> enc;
  std::vector<int32_t> sa;
  prb::DevBuf d_enc, d_sa, d_acc, d_cond, d_off, d_len;
  bool have_acc = false;
  int32_t W = 0, delta = 0;
  prb::QBatchDev view{};
  std::unique_ptr<prb::SeedPlan> plan; // a seed search started ahead of prb_search_page, if any
};

// prb_pairmask_create .. prb_pairmask_free (capi_pairmask.hip): the pairs a search of `qb` against `db` is restricted to.
// The bits are set on the host; the first search that uses the mask uploads them (use_pairmask) and closes it to changes.
struct prb_pairmask {
  prb_ctx *ctx = nullptr;
  const prb_qbatch *qb = nullptr;
  const prb_db *db = nullptr;
  int32_t nq = 0;
  std::vector<int64_t> tbase; // [npages + 1] the first target of every page; back() = the targets
  int64_t row_words = 0;      // 32-bit words per query
  std::vector<uint32_t> bits; // [nq * row_words]
  int64_t count = 0;          // bits set
  bool used = false;
  std::mutex first_use;       // the upload, whoever comes first
  prb::DevBuf dev;
  ~prb_pairmask() {
    if (dev.p) (void)hipSetDevice(ctx->device);
    dev.release();
  }
};

namespace prb {
// capi_pairmask.hip: opts->allowed_pairs checked against the search it is given to (PRB_ERR_ARG with `fn` in the message)
// and, at its first use, uploaded; *view = the mask as the kernels take it for `page`.  Not called for NULL.
int use_pairmask(const char *fn, prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page, const prb_pairmask *pm, AllowDev *view);

// What a result table takes from every sub-batch of a page search - what the search driver (emit_to_table,
// capi_search.hip) prepares before it calls TableState::take; each of the first three has all that the one above it has:
enum class TableFeed {
  kHits,        // the final hits F with their end pairs, as the simplified output has them (SubBatch::ends)
  kPairRuns,    // ... and the runs of equal (query, db_id) in F: pair_start, npairs
  kPairRecords, // ... and the runs folded into records: prb_pair_summary[npairs]
  kHitRecords,  // F and its records: prb_hit[nfin] as prb_search_page packs them, their base-pair ranges counted from pair
                // TableState::bp_base() on; fresh_bp = the ints that the ranges index (none of the three above)
};
// One sub-batch as a table takes it: the queries [q0, q1) of a batch of nq against `page` (of nseq sequences).  What
// the table's feed does not include is null; everything is on the device, and nothing of it outlives the call.
struct SubBatch {
  int32_t page, q0, q1, nq, nseq;
  HitSoA F;
  int64_t nfin;
  const int32_t *ends = nullptr;
  const uint32_t *pair_start = nullptr;
  int64_t npairs = 0;
  void *records = nullptr;
  const int32_t *fresh_bp = nullptr;
};

// What the thirteen result tables have in common (prb_topset, prb_tophits, prb_profset, prb_targetset, prb_covset,
// prb_nullset, prb_groupset, prb_grouprank, prb_gnullset, prb_evalset, prb_featset, prb_fnullset, prb_featrank): whose they are, whether they can still be merged into, and the block on the device that
// the merges work on.  What every prb_*_merge and prb_*_finish checks (capi_tables.hpp), and what a page search hands
// its sub-batches to: the table says which feed it takes, and takes it - in a bracket of its own stage timer, in its
// own file; nothing leaves the device.
struct TableState {
  virtual ~TableState() = default;
  virtual TableFeed feed() const = 0;
  virtual int64_t bp_base() const { return 0; } // (kHitRecords)
  virtual int take(const SubBatch &b) = 0;
  prb_ctx *ctx = nullptr;
  const prb_db *db = nullptr;  // batch tables: of the first merged page; run tables: the one they were made for
  bool broken = false;         // a merge failed part way
  bool finished = false;       // prb_*_finish: the records are on the host, the device memory is released
  int32_t distinct = -1;       // opts->distinct_sites of the merged pages (-1: none yet)
  int32_t chain = -1;          // opts->chain_sites of the merged pages, likewise
  int64_t counts[3] = {0, 0, 0};
  DevBuf table;                // the table proper, one block (every table says what it holds)
  bool bad = false;            // the device's `bad` flag, as the last call left it (fetch_bad, capi_tables.hpp) - of the
  DevBuf badflag;              // tables that keep one of their own: prb_nullset, prb_groupset, prb_grouprank, prb_gnullset, prb_evalset, prb_featrank
  // What their release() starts with - nothing of such a table is released while work on it may still be queued on its
  // context's stream: false = there is no context yet, and so nothing to release
  bool quiesce() const {
    if (!ctx) return false;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    return true;
  }
};

// The tables that a batch's pages are merged into one by one (prb_topset, prb_profset, prb_tophits): a byte per page
struct MergeTable : TableState {
  const prb_qbatch *qb = nullptr;
  int32_t nq = 0;
  std::vector<int32_t> qlen;   // the queries' lengths (what two tables must share to be merged, prb_*_merge)
  std::vector<uint8_t> merged; // per page of db
};

// The tables that live for a whole run and are keyed by the database's targets (page, db_id) (prb_targetset, prb_covset)
// or by its groups or features (prb_grouprank, prb_featrank: one "page", its "targets" the groups / the features): such a table takes any number of batches, so
// it keeps a bit per (page, query identifier)
struct RunTable : TableState {
  std::vector<int64_t> tbase;                 // [npages + 1] the first target of every page; back() = the targets
  std::vector<std::vector<uint64_t>> merged;  // per page: a bit per query identifier merged, grown on demand
  DevBuf ids;                                 // the identifiers of the batch being merged
  int64_t targets() const { return tbase.empty() ? 0 : tbase.back(); }
  bool has(size_t page, int32_t id) const {
    const std::vector<uint64_t> &m = merged[page];
    return ((size_t)id >> 6) < m.size() && (m[(size_t)id >> 6] >> (id & 63) & 1);
  }
  void set(size_t page, int32_t id) {
    std::vector<uint64_t> &m = merged[page];
    if (((size_t)id >> 6) >= m.size()) m.resize(((size_t)id >> 6) + 1, 0);
    m[(size_t)id >> 6] |= 1ull << (id & 63);
  }
};

// What the tables that take a batch's decoys keep of them (prb_nullset, prb_evalset, prb_gnullset, prb_fnullset): a bit per (query,
// decoy) that is merged - a row of them per page, where the table keeps the pages apart: `bit0` = the bit of (0, 0) in
// the row - and the batch of decoys being merged, on the device (decoys_guard, mark_decoys, upload_owners, capi_tables.hpp)
struct DecoySet {
  int32_t nq = 0, ndecoys = 0;
  std::vector<uint64_t> merged; // the bits
  int64_t nmerged = 0;          // ... that are set
  DevBuf own;                   // the decoy batch being merged: owner[ndq], then decoy[ndq]
  int32_t ndq = 0;              // ... its number of decoys
  int64_t decoys_all() const { return (int64_t)nq * ndecoys; }
  int64_t bit_of(int64_t bit0, int32_t q, int32_t d) const { return bit0 + (int64_t)q * ndecoys + d; }
};
// The tables that a batch's decoys are searched into page by page, batch by batch, behind the real batch (prb_nullset,
// prb_evalset): a bit per (page, query, decoy)
struct DecoyTable : TableState, DecoySet {
  const prb_qbatch *qb = nullptr;
  int32_t npages = 0;
  int64_t decoy_counts[3] = {0, 0, 0}; // the stage counts of the decoy searches (`counts`: of the real batch's)
  bool decoy_phase = false;            // the batch being searched is one of decoys: what take() merges (else the real batch)
  int64_t triples() const { return (int64_t)npages * decoys_all(); }
  int64_t bit0(int32_t page) const { return (int64_t)page * decoys_all(); }
};

// What the two span tables own beside their block (prb_profset, prb_covset; capi_spans.hip): per merge the hits in
// (owner, first position) order - keys and values before and behind the sort, the spans' ends and their running
// maximum - and the temporary storage of the sorts, scans and selects
struct SpanBufs {
  DevBuf keyA, keyB, valA, valB, span, scan, sortTmp;
  void release() {
    for (DevBuf *b : {&keyA, &keyB, &valA, &valB, &span, &scan, &sortTmp}) b->release();
  }
};

// What the two top-N tables have in common (prb_topset, prb_tophits): n slots of `Slot` per query and the queries' fill
// counts, one block on the device: Slot[nq * n] (`rank` = the record's ordinal within its query's run on the device),
// then int32_t fill[nq]
template <class Slot> struct TopTable : MergeTable {
  int32_t n = 0;
  size_t slots_bytes() const { return (size_t)nq * (size_t)n * sizeof(Slot); }
  size_t bytes() const { return slots_bytes() + (size_t)nq * sizeof(int32_t); }
  int32_t *fill() const { return reinterpret_cast<int32_t *>(table.template as<char>() + slots_bytes()); }
};

// What the three ranked run tables have in common (prb_targetset, prb_grouprank, prb_featrank; capi_ranked.hpp): per
// list - a target, a group, a feature: L = targets() of them - its n best queries as the ranked lists of rank_kernels.hpp,
// merged into for as many batches as the caller likes, and the sort buffers of those merges.  It owns all its device memory.
// The block: TargetKey[L * n], Payload[L * n], int32_t fill[L + 1] (the last one 0)
template <class P> struct RankedTable : RunTable {
  using Payload = P;
  int32_t n = 0;
  DevBuf key, keyS, val, valS, rkey, head, start, sortTmp; // per merge: the candidates in list order
  DevBuf h_rec;                                            // prb_*_add_records: the caller's records
  std::vector<Payload> recs;                               // prb_*_finish
  TableFeed feed() const override { return TableFeed::kPairRecords; }
  int take(const SubBatch &) override { return PRB_ERR_STATE; } // (no search feeds it, unless the table says otherwise)
  size_t entries() const { return (size_t)targets() * (size_t)n; }
  size_t bytes() const { return entries() * (sizeof(TargetKey) + sizeof(Payload)) + ((size_t)targets() + 1) * sizeof(int32_t); }
  // the three arrays of a block at b (the table's own, or a copy of another table's)
  TargetKey *keys_of(void *b) const { return static_cast<TargetKey *>(b); }
  Payload *slots_of(void *b) const { return reinterpret_cast<Payload *>(static_cast<char *>(b) + entries() * sizeof(TargetKey)); }
  int32_t *fill_of(void *b) const { return reinterpret_cast<int32_t *>(static_cast<char *>(b) + entries() * (sizeof(TargetKey) + sizeof(Payload))); }
  RankedLists lists_of(void *b) const { return RankedLists{keys_of(b), slots_of(b), fill_of(b), targets(), n}; }
  // every key, payload slot and fill count of the table back to "nothing", on its own device and stream
  int clear() {
    PRB_HIP(hipSetDevice(ctx->device));
    PRB_HIP(hipMemsetAsync(table.p, 0, bytes(), ctx->stream));
    PRB_HIP(hipStreamSynchronize(ctx->stream));
    return PRB_OK;
  }
  void release(std::initializer_list<DevBuf *> own = {}) { // (`own`: what the table has beside)
    if (!quiesce()) return;
    for (DevBuf *b : {&table, &badflag, &ids, &key, &keyS, &val, &valS, &rkey, &head, &start, &sortTmp, &h_rec}) b->release();
    for (DevBuf *b : own) b->release();
  }
  ~RankedTable() { release(); } // (also on the error paths of prb_*_create)
};
} // namespace prb

// prb_topset_create .. prb_topset_free: the top-N table of one batch, merged into page by page (launch_top_merge)
struct prb_topset : prb::TopTable<prb_top_pair> {
  std::vector<prb_top_pair> pairs; // prb_topset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRecords; }
  int take(const prb::SubBatch &b) override;
  ~prb_topset() { // (also on the error paths of prb_topset_create)
    if (table.p) (void)hipSetDevice(ctx->device);
    table.release();
  }
};

// prb_tophits_create .. prb_tophits_free: the top-N hit table of one batch, merged into sub-batch by sub-batch
// (capi_top.hip), and the pool of the kept hits' base pairs
struct prb_tophits : prb::TopTable<prb_top_hit> {
  int32_t style = -1;              // opts->output_style of the merged pages (-1: none yet)
  prb::DevBuf pool, pool2;         // the kept hits' pairs in table order (h.bp_offset indexes `pool`); the gather's target
  int64_t pool_pairs = 0;          // pairs in `pool`
  prb::DevBuf cnt, off, scanTmp;   // per slot (+ 1): pair counts, their exclusive scan
  std::vector<prb_top_hit> hits;   // prb_tophits_finish
  std::vector<int32_t> bp;
  prb::TableFeed feed() const override { return prb::TableFeed::kHitRecords; }
  int64_t bp_base() const override { return pool_pairs; } // (a newcomer's pairs lie behind the pool's until the gather)
  int take(const prb::SubBatch &b) override;
  void release() {
    for (prb::DevBuf *b : {&table, &pool, &pool2, &cnt, &off, &scanTmp}) b->release();
  }
  ~prb_tophits() { // (also on the error paths of prb_tophits_create)
    if (table.p || pool.p || pool2.p || cnt.p) (void)hipSetDevice(ctx->device);
    release();
  }
};

// prb_profset_create .. prb_profset_free: the per-position table of one batch, merged into sub-batch by sub-batch
// (merge_profile, capi_spans.hip), and the sort / scan buffers of those merges (per sub-batch: the hits in (pair, first
// position) order)
struct prb_profset : prb::MergeTable, prb::SpanBufs {
  std::vector<int64_t> off;    // [nq + 1] the queries' first slots (ProfTab::off)
  std::vector<prb_profile_pos> rows; // prb_profset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRuns; }
  int take(const prb::SubBatch &b) override;
  int64_t slots() const { return off.empty() ? 0 : off.back(); }
  // the block (view()): off, then the 8-byte arrays hdiff, key, tie, skey, e_min, then the 4-byte arrays tdiff, stie,
  // db_id, bp (x4), bad
  size_t bytes() const { return (off.size() + 5 * (size_t)slots()) * 8 + (7 * (size_t)slots() + 2) * 4; }
  prb::ProfTab view() const { return view_of(table.as<char>()); }
  // the arrays of a block at b (the table's own, or a copy of another table's)
  prb::ProfTab view_of(char *b) const {
    prb::ProfTab t;
    const size_t P = (size_t)slots();
    t.off = reinterpret_cast<const int64_t *>(b);
    b += off.size() * 8;
    t.hdiff = reinterpret_cast<unsigned long long *>(b);
    t.key = t.hdiff + P;
    t.tie = t.key + P;
    t.skey = t.tie + P;
    t.e_min = reinterpret_cast<double *>(t.skey + P);
    t.tdiff = reinterpret_cast<int32_t *>(t.e_min + P);
    t.stie = reinterpret_cast<uint32_t *>(t.tdiff + P);
    t.db_id = reinterpret_cast<int32_t *>(t.stie + P);
    t.bp = t.db_id + P;
    t.bad = reinterpret_cast<uint32_t *>(t.bp + 4 * P);
    t.nq = nq;
    return t;
  }
  void release() {
    table.release();
    SpanBufs::release();
  }
  ~prb_profset() { // (also on the error paths of prb_profset_create)
    if (table.p || keyA.p || sortTmp.p) (void)hipSetDevice(ctx->device);
    release();
  }
};

// prb_targetset_create .. prb_targetset_free: the per-target table of one database, merged into sub-batch by sub-batch
// (prb_targetset::take, capi_targets.hip) for as many batches as the caller likes: a ranked table whose lists are the
// database's targets, page by page
struct prb_targetset : prb::RankedTable<prb_target_pair> {
  int take(const prb::SubBatch &b) override;
};

// prb_covset_create .. prb_covset_free: the per-position coverage table of one database, merged into sub-batch by
// sub-batch (prb_search_page_coverage) or list by list (prb_covset_add_hits) for as many batches as the caller likes
// (merge_coverage, capi_spans.hip), and the sort / scan buffers of those merges (per merge: the hits in (query, first
// position) order)
struct prb_covset : prb::RunTable, prb::SpanBufs {
  std::vector<int64_t> seq_lo;  // [T + 1] the first slot of every target (CovTab::seq_lo); back() = the slots
  std::vector<int64_t> slot0;   // [npages + 1] the first slot of every page
  prb::DevBuf place;                              // per merge: every hit's place in its list
  prb::DevBuf h_query, h_db_id, h_e_tot, h_ends;  // prb_covset_add_hits: the caller's list as columns
  std::vector<prb_target_region> regions; // prb_covset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kHits; }
  int take(const prb::SubBatch &b) override;
  int64_t slots() const { return seq_lo.empty() ? 0 : seq_lo.back(); }
  size_t head_bytes() const { return (seq_lo.size() + tbase.size()) * 8; }
  // the block (view()): seq_lo and tbase, then the 8-byte arrays hdiff, key, tie, skey, stie, e_min, then the 4-byte
  // arrays qdiff, starts, bp (x4), bad
  size_t bytes() const { return head_bytes() + 6 * (size_t)slots() * 8 + (6 * (size_t)slots() + 2) * 4; }
  prb::CovTab view() const { return view_of(table.as<char>()); }
  const int64_t *tbase_dev() const { return table.as<int64_t>() + seq_lo.size(); }
  // the arrays of a block at b (the table's own, or a copy of another table's)
  prb::CovTab view_of(char *b) const {
    prb::CovTab t;
    const size_t P = (size_t)slots();
    t.seq_lo = reinterpret_cast<const int64_t *>(b);
    b += head_bytes();
    t.hdiff = reinterpret_cast<unsigned long long *>(b);
    t.key = t.hdiff + P;
    t.tie = t.key + P;
    t.skey = t.tie + P;
    t.stie = t.skey + P;
    t.e_min = reinterpret_cast<double *>(t.stie + P);
    t.qdiff = reinterpret_cast<int32_t *>(t.e_min + P);
    t.starts = reinterpret_cast<uint32_t *>(t.qdiff + P);
    t.bp = reinterpret_cast<int32_t *>(t.starts + P);
    t.bad = reinterpret_cast<uint32_t *>(t.bp + 4 * P);
    return t;
  }
  prb::CovPage page_view(size_t page) const {
    return prb::CovPage{slot0[page], tbase[page], (int32_t)(tbase[page + 1] - tbase[page])};
  }
  void release() {
    for (prb::DevBuf *b : {&table, &ids, &place, &h_query, &h_db_id, &h_e_tot, &h_ends}) b->release();
    SpanBufs::release();
  }
  ~prb_covset() { // (also on the error paths of prb_covset_create)
    if (table.p || ids.p || keyA.p || h_query.p) (void)hipSetDevice(ctx->device);
    release();
  }
};

// prb_nullset_create .. prb_nullset_free: the null table of one batch against one database (capi_null.hip), merged into
// sub-batch by sub-batch - the real batch's pairs page by page first (merge_null_observed), then the pairs of its decoys
// (merge_null_decoys).  Between two batches of decoys prb_nullset_retire may retire the decided pairs: a retired slot takes
// no further decoys, and a query without live slots needs none.  It owns all its device memory; `table` = NullSlot[nq * targets]
struct prb_nullset : prb::DecoyTable {
  std::vector<int64_t> tbase;        // [npages + 1] the first target of every page; back() = the targets
  std::vector<uint8_t> observed;     // per page: the real batch's search is merged
  prb::DevBuf obs, tbase_dev;        // the selection's flags, tbase on the device
  prb::DevBuf live, live_dev;        // a byte per slot: it still takes decoys; prb_nullset_retire's counts per query
  int32_t retired_upto = 0;          // `upto` of the last prb_nullset_retire (0: none yet)
  std::vector<int64_t> live_q;       // [nq] the live slots of every query after that call (before the first: not known, -1)
  std::vector<int32_t> needs;        // [nq] the decoys a query must have merged for prb_nullset_finish: ndecoys while it has
                                     // live slots, else `upto` of the call that found it without
  prb::DevBuf h_rec;                 // prb_nullset_observe / _add_pairs: the caller's records
  prb::DevBuf sel, out;              // prb_nullset_finish: the observed slots, their records
  prb::DevBuf fdr_out;               // prb_nullset_finish_fdr: their figures
  std::vector<prb_null_pair> pairs;  // prb_nullset_finish
  std::vector<prb_null_fdr> fdr;     // prb_nullset_finish_fdr: parallel to pairs
  bool has_fdr = false;              // ... finished it
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRecords; }
  int take(const prb::SubBatch &b) override;
  int64_t targets() const { return tbase.empty() ? 0 : tbase.back(); }
  int64_t slots() const { return (int64_t)nq * targets(); }
  prb::NullTab view() const {
    return prb::NullTab{table.as<prb::NullSlot>(), obs.as<uint8_t>(), live.as<uint8_t>(), badflag.as<uint32_t>(), slots(), targets(), nq, ndecoys};
  }
  bool merged_bit(int32_t page, int32_t q, int32_t d) const {
    const int64_t b = bit_of(bit0(page), q, d);
    return (merged[(size_t)(b >> 6)] >> (b & 63)) & 1;
  }
  prb::NullPage page_view(size_t page) const { return prb::NullPage{tbase[page], (int32_t)(tbase[page + 1] - tbase[page])}; }
  void release() {
    if (!quiesce()) return;
    for (prb::DevBuf *b : {&table, &obs, &live, &live_dev, &badflag, &tbase_dev, &own, &h_rec, &sel, &out, &fdr_out}) b->release();
  }
  ~prb_nullset() { release(); } // (also on the error paths of prb_nullset_create)
};

// prb_groupset_create .. prb_groupset_free: the group table of one batch against one database (capi_groups.hip), folded
// into sub-batch by sub-batch (merge_group_pairs).  It owns all its device memory; `table` = GroupSlot[nq * ngroups],
// the one block that prb_groupset_merge reads of another table
struct prb_groupset : prb::MergeTable {
  int32_t ngroups = 0;
  std::vector<std::vector<int32_t>> map; // per page: the groups of its sequences (what two tables must share to be merged)
  std::vector<prb::DevBuf> map_dev;      // ... on the device
  prb::DevBuf h_rec;                     // prb_groupset_add_pairs: the caller's records
  prb::DevBuf occ, sel, top, keep, out;  // prb_groupset_finish: flags and lists of the selection, the records
  std::vector<prb_group_pair> pairs;     // prb_groupset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRecords; }
  int take(const prb::SubBatch &b) override;
  int64_t slots() const { return (int64_t)nq * ngroups; }
  size_t bytes() const { return (size_t)slots() * sizeof(prb::GroupSlot); }
  prb::GroupTab view() const {
    return prb::GroupTab{table.as<prb::GroupSlot>(), badflag.as<uint32_t>(), slots(), nq, ngroups, (int32_t)map.size()};
  }
  prb::GroupPage page_view(size_t page) const { return prb::GroupPage{map_dev[page].as<int32_t>(), (int32_t)page, (int32_t)map[page].size()}; }
  void release() {
    if (!quiesce()) return;
    for (prb::DevBuf *b : {&table, &badflag, &h_rec, &occ, &sel, &top, &keep, &out}) b->release();
    for (prb::DevBuf &b : map_dev) b.release();
  }
  ~prb_groupset() { release(); } // (also on the error paths of prb_groupset_create)
};

// prb_grouprank_create .. prb_grouprank_free: the group ranking table of a run (capi_grouprank.hip): per group its n best
// queries over as many batches as the caller likes, fed from each batch's complete group table or from a caller's
// records (merge_ranked_candidates, capi_ranked.hpp) - never by a search itself.  A ranked table with one "page": `merged`
// keeps a bit per query identifier, tbase = {0, ngroups}.
struct prb_grouprank : prb::RankedTable<prb_group_pair> {
  int32_t ngroups = 0;
  prb::DevBuf occ, sel; // per merge: the group table's occupied slots
  void release() { RankedTable::release({&occ, &sel}); }
  ~prb_grouprank() { release(); }
};

// prb_gnullset_create .. prb_gnullset_free: the group null table of one batch (capi_gnull.hip): the records that a group
// table was finished into, kept on the device with a lookup from (query, group), and their decoy counters.  Decoys come
// in batches between prb_gnullset_begin and prb_gnullset_end; the pages of the open batch are folded into `cell`
// sub-batch by sub-batch (merge_gnull_pairs).  It owns all its device memory - the page maps are the group table's,
// taken over when that is finished.  `table` = GNullCount[nkept]
struct prb_gnullset : prb::TableState, prb::DecoySet { // (`merged`: a bit per (query, decoy) whose batch is closed, prb_gnullset_end)
  int32_t ngroups = 0;
  int64_t nkept = 0;
  std::vector<std::vector<int32_t>> map; // per page: the groups of its sequences
  std::vector<prb::DevBuf> map_dev;      // ... on the device
  bool open = false;                     // between prb_gnullset_begin and prb_gnullset_end
  std::vector<int32_t> owner, decoy;     // the open batch
  std::vector<uint8_t> page_merged;      // per page: merged in the open batch
  prb::DevBuf lookup, kept, cell;
  prb::DevBuf h_rec;                     // prb_gnullset_add_pairs: the caller's records
  prb::DevBuf out;                       // prb_gnullset_finish: the records
  std::vector<prb_gnull_pair> pairs;     // prb_gnullset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRecords; }
  int take(const prb::SubBatch &b) override;
  int64_t slots() const { return (int64_t)nq * ngroups; }
  prb::GNullTab view() const {
    const int32_t ndq = (int32_t)owner.size();
    return prb::GNullTab{lookup.as<uint32_t>(), table.as<prb::GNullCount>(), cell.as<unsigned long long>(), own.as<int32_t>(),
                         own.as<int32_t>() + ndq, badflag.as<uint32_t>(), nkept, nq, ngroups, ndecoys, (int32_t)map.size(), ndq};
  }
  prb::GroupPage page_view(size_t page) const { return prb::GroupPage{map_dev[page].as<int32_t>(), (int32_t)page, (int32_t)map[page].size()}; }
  void release() {
    if (!quiesce()) return;
    for (prb::DevBuf *b : {&table, &lookup, &kept, &cell, &own, &badflag, &h_rec, &out}) b->release();
    for (prb::DevBuf &b : map_dev) b.release();
  }
  ~prb_gnullset() { release(); } // (also on the error paths of prb_gnullset_create)
};

// prb_evalset_create .. prb_evalset_free: the evalset of one batch against one database (capi_eval.hip): the energy keys
// of the real batch's final hits and of its decoys', appended sub-batch by sub-batch (append_eval_keys) and closed into
// sorted segments with every real hit's figures.  It owns all its device memory; `table` is not used.
struct prb_evalset : prb::DecoyTable {
  // a list of (key, owner) that grows on the host's side between launches and keeps what it holds; a buffer that is
  // outgrown is retired, not freed, until the close (hipFree waits for the whole device)
  struct List {
    prb::DevBuf key, own; // unsigned long long [cap], uint32_t [cap]
    int64_t n = 0, cap = 0;
    std::vector<prb::DevBuf> retired;
  };
  List real, dec;
  std::vector<uint8_t> real_merged;  // per page: the real batch's search is merged
  int64_t nreal_merged = 0;          // ... bytes set
  bool searched = false;             // something came by a search: the close asks for all of it
  prb_tophits *tee = nullptr;        // prb_search_page_scored: the table that the sub-batch is handed on to
  prb::DevBuf h_ids, h_energy;       // prb_evalset_add_keys / _score: the caller's list
  prb::DevBuf off, null_le, rank, qnum, qden, out; // the close: roff, doff [nq + 1] each; per real entry; the look-up's records
  prb::TableFeed feed() const override { return tee && !decoy_phase ? prb::TableFeed::kHitRecords : prb::TableFeed::kHits; }
  int64_t bp_base() const override { return tee && !decoy_phase ? tee->bp_base() : 0; }
  int take(const prb::SubBatch &b) override;
  prb::EvalTab view() const {
    return prb::EvalTab{real.key.as<unsigned long long>(), dec.key.as<unsigned long long>(), off.as<int64_t>(), off.as<int64_t>() + (nq + 1),
                        null_le.as<uint32_t>(), rank.as<uint32_t>(), qnum.as<uint32_t>(), qden.as<uint32_t>(), badflag.as<uint32_t>(),
                        real.n, dec.n, nq, ndecoys};
  }
  void drop_retired() {
    for (List *l : {&real, &dec}) {
      for (prb::DevBuf &b : l->retired) b.release();
      l->retired.clear();
    }
  }
  void release() {
    if (!quiesce()) return;
    drop_retired();
    for (prb::DevBuf *b : {&real.key, &real.own, &dec.key, &dec.own, &badflag, &own, &h_ids, &h_energy, &off, &null_le, &rank, &qnum, &qden, &out})
      b->release();
  }
  ~prb_evalset() { release(); } // (also on the error paths of prb_evalset_create)
};

// prb_annot_create .. prb_annot_free (capi_features.hip): the annotation of one database, sorted by (page, db_id, start,
// end, index), on the host - what two feature tables must share to be merged - and as one CSR per page on the device
struct prb_annot {
  prb_ctx *ctx = nullptr;
  const prb_db *db = nullptr;
  int64_t n = 0;
  struct Page {
    std::vector<int32_t> off, slo, slen; // [nseq + 1], [nseq], [nseq]
    std::vector<int32_t> start, end, idx; // the features in order: forward coordinates, the caller's index
    prb::DevBuf dev;                      // off, slo, slen, tlo, thi, idx
    bool operator==(const Page &o) const { return off == o.off && slen == o.slen && start == o.start && end == o.end && idx == o.idx; }
  };
  std::vector<Page> pages;
  prb::FeatPage page_view(size_t p) const {
    const Page &g = pages[p];
    const int32_t *b = g.dev.as<int32_t>();
    const size_t ns = g.slo.size(), nf = g.idx.size();
    return prb::FeatPage{b, b + ns + 1, b + 2 * ns + 1, b + 3 * ns + 1, b + 3 * ns + 1 + nf, b + 3 * ns + 1 + 2 * nf, (int32_t)p, (int32_t)ns};
  }
  ~prb_annot() {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (Page &g : pages) g.dev.release();
  }
};

// prb_featset_create .. prb_featset_free: the feature table of one batch against one annotated database
// (capi_features.hip), folded into sub-batch by sub-batch (merge_feature_hits).  It owns all its device memory; `table` =
// int64_t first[cells], end[cells] (cells = pages x queries: the places of a (page, query)'s records), then
// prb_feature_pair[cap], of which nrec are in use - the one block that prb_featset_merge reads of another table
struct prb_featset : prb::MergeTable {
  const prb_annot *annot = nullptr;
  int64_t nrec = 0, cap = 0;       // records in the block, and its room
  int64_t unassigned = 0;          // final hits that belong to no feature
  prb::DevBuf cnt, ioff, tmp, flag, long_list, sel, scanTmp, count; // per fold: FeatWork, the selected items
  prb::DevBuf head, start;                                          // prb_featset_add_hits: the runs of the caller's list
  prb::DevBuf h_query, h_db_id, h_e_tot, h_e_acc, h_e_hyb, h_ends;  // ... and the list as columns
  prb::DevBuf out;                                                  // prb_featset_finish: the records in order
  prb::DevBuf topCnt, topOff, topKey, topPlace, topSel, topOut;     // prb_featset_finish_top: the counts and their scans, the chunks' lists, the ranked places and records
  int32_t top_n = 0;                                                // ... the n it was finished with (0: a plain finish)
  std::vector<prb_feature_pair> recs;                               // prb_featset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRuns; }
  int take(const prb::SubBatch &b) override;
  int64_t cells() const { return (int64_t)merged.size() * nq; }
  size_t head_bytes() const { return (size_t)cells() * 16; }
  size_t bytes() const { return head_bytes() + (size_t)nrec * sizeof(prb_feature_pair); } // (what is in use)
  int64_t *first_of(void *b) const { return static_cast<int64_t *>(b); }
  int64_t *end_of(void *b) const { return static_cast<int64_t *>(b) + cells(); }
  prb_feature_pair *recs_of(void *b) const { return reinterpret_cast<prb_feature_pair *>(static_cast<char *>(b) + head_bytes()); }
  void release() {
    if (!quiesce()) return;
    for (prb::DevBuf *b : {&table, &badflag, &cnt, &ioff, &tmp, &flag, &long_list, &sel, &scanTmp, &count, &head, &start, &h_query, &h_db_id,
                           &h_e_tot, &h_e_acc, &h_e_hyb, &h_ends, &out, &topCnt, &topOff, &topKey, &topPlace, &topSel, &topOut})
      b->release();
  }
  ~prb_featset() { release(); } // (also on the error paths of prb_featset_create)
};

// prb_fnullset_create .. prb_fnullset_free: the feature null table of one batch (capi_fnull.hip): the records that a
// feature table was finished into, kept on the device with their sorted lookup keys, and their decoy counters.  Decoys
// come in batches between prb_fnullset_begin and prb_fnullset_end; the pages of the open batch are folded into `cell`
// sub-batch by sub-batch (merge_fnull_hits).  It owns all its device memory.  `table` = GNullCount[nkept]
struct prb_fnullset : prb::TableState, prb::DecoySet { // (`merged`: a bit per (query, decoy) whose batch is closed, prb_fnullset_end)
  const prb_annot *annot = nullptr;
  int64_t nkept = 0, ncells = 0;         // records; the cells of the open batch
  std::vector<int64_t> qoff;             // [nq + 1] the first key of every query (FNullTab::qoff)
  bool open = false;                     // between prb_fnullset_begin and prb_fnullset_end
  std::vector<int32_t> owner, decoy;     // the open batch
  std::vector<uint8_t> page_merged;      // per page: merged in the open batch
  prb::DevBuf key, rec, qoff_dev, kept, cell, doff;
  prb::DevBuf cnt, ioff, long_list, scanTmp;             // per fold: FeatWork
  prb::DevBuf head, start;                               // prb_fnullset_add_hits: the runs of the caller's list
  prb::DevBuf h_query, h_db_id, h_e_tot, h_e_acc, h_e_hyb, h_ends; // ... and the list as columns
  prb::DevBuf out;                       // prb_fnullset_finish: the records
  std::vector<prb_fnull_pair> recs;      // prb_fnullset_finish
  prb::TableFeed feed() const override { return prb::TableFeed::kPairRuns; }
  int take(const prb::SubBatch &b) override;
  prb::FNullTab view() const {
    const int32_t ndq = (int32_t)owner.size();
    return prb::FNullTab{key.as<unsigned long long>(), rec.as<uint32_t>(), qoff_dev.as<int64_t>(), table.as<prb::GNullCount>(),
                         cell.as<unsigned long long>(), own.as<int32_t>(), own.as<int32_t>() + ndq, doff.as<int64_t>(), badflag.as<uint32_t>(),
                         nkept, ncells, annot->n, nq, ndecoys, (int32_t)annot->pages.size(), ndq};
  }
  void release() {
    if (!quiesce()) return;
    for (prb::DevBuf *b : {&table, &badflag, &own, &key, &rec, &qoff_dev, &kept, &cell, &doff, &cnt, &ioff, &long_list, &scanTmp, &head, &start,
                           &h_query, &h_db_id, &h_e_tot, &h_e_acc, &h_e_hyb, &h_ends, &out})
      b->release();
  }
  ~prb_fnullset() { release(); } // (also on the error paths of prb_fnullset_create)
};

// prb_featrank_create .. prb_featrank_free: the feature ranking table of a run (capi_featrank.hip): per feature of the
// annotation its n best queries over as many batches as the caller likes, fed from each batch's complete feature table or
// from a caller's records (merge_ranked_candidates, capi_ranked.hpp) - never by a search itself.  A ranked table with one
// "page": `merged` keeps a bit per query identifier, tbase = {0, nfeat}.
struct prb_featrank : prb::RankedTable<prb_featrank_pair> {
  const prb_annot *annot = nullptr;
  int32_t nfeat = 0;
  int64_t unassigned = 0; // summed over the feature tables merged
  int clear() {
    if (int rc = RankedTable::clear()) return rc;
    unassigned = 0;
    return PRB_OK;
  }
};

namespace prb {
// capi_features.hip: prb_featset_finish proper, for `fn_name`; n > 0 (prb_featset_finish_top, prb_fnullset_create_top):
// each query's n best records only, ranked on the device.  keep != nullptr (prb_fnullset_create[_top]): before the
// feature table's device memory is released, the records that the host gets - still on the device, the ranked ones with
// n > 0 - go to keep_feature_records (capi_fnull.hip).
int finish_featset(const char *fn_name, prb_ctx *ctx, prb_featset *fs, int32_t n, prb_fnullset *keep);
int keep_feature_records(prb_ctx *ctx, prb_fnullset *fn, prb_featset *fs, const void *recs_dev, int64_t nrec);
// capi_features.hip: what prb_featset_add_hits and prb_fnullset_add_hits do with a caller's list of final hits of one
// page: checked on the host against the page `g` of the annotation and a batch of nq queries, as columns; the columns to
// the device in the table's six buffers (query, db_id, e_tot, e_acc, e_hyb, ends); and the runs of equal (query, db_id)
// of such a list - two launches, and a synchronisation for their number
struct HitColumns {
  std::vector<int32_t> query, db_id, ends;
  std::vector<double> e_tot, e_acc, e_hyb;
};
int check_hit_list(const std::string &fn, const prb_annot::Page &g, int32_t nq, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                   int64_t npairs, HitColumns &c);
int upload_hit_list(prb_ctx *ctx, const HitColumns &c, DevBuf *const bufs[6], FeatHits *h);
int hit_list_runs(prb_ctx *ctx, const FeatHits &h, DevBuf &head, DevBuf &start, const uint32_t **start_out, int64_t *npairs);
} // namespace prb

namespace prb {
// capi_groups.hip: prb_groupset_finish proper, for `fn_name`.  keep != nullptr (prb_gnullset_create): before the group
// table's device memory is released, the gathered records - still on the device - go to keep_group_records
// (capi_gnull.hip), which also takes the page maps over.
int finish_groupset(const char *fn_name, prb_ctx *ctx, prb_groupset *gs, int32_t n, prb_gnullset *keep);
int keep_group_records(prb_ctx *ctx, prb_gnullset *gn, prb_groupset *gs, const void *recs_dev, int64_t nrec);
} // namespace prb

namespace prb {
// Host threads for the per-query host work (suffix arrays, seed DFS): PRB_HOST_THREADS, else half of the CPUs the
// process may keep busy, at most 32 (capi_pages.hip)
int host_threads(int work_items);

// where the final hits of a search go
enum class SearchMode {
  kRecords, // prb_search_page: hit records and base pairs to the host
  kSummary, // prb_search_page_summary: per-pair records to the host
  kTable,   // every prb_search_page_* of a result table: into the table on the device, by the table's feed
};
// (every mode but the first: no hit records for the host; a table that takes hit records keeps them itself)
inline bool reduces_to_pairs(SearchMode m) { return m != SearchMode::kRecords; }

// capi_pages.hip
int page_slot(prb_ctx *user, prb_db *db, int page, int keep, hipStream_t stream, int *slot_out);
std::unique_ptr<SeedPlan> start_seed_plan(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page, int32_t max_seed_length,
                                          double hybrid_threshold);
// capi_search.hip: the argument checks and option limits of a search (`fn` names the entry point in the messages), and
// the search of one page in `mode`; `table` = the table of kTable (search_into_table, capi_tables.hpp)
int check_search_args(const char *fn, const prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t page,
                      const prb_ris_opts *opts, int32_t last_stage);
int search_page(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, int32_t last_stage,
                SearchMode mode, prb_hitset **out, TableState *table = nullptr);
// capi_search.hip: the two radix sorts of the tables' merges - by the low `bits` bits of 32-bit keys, through `tmp`
// (the ranked run tables, capi_ranked.hpp), and rocPRIM's two calls for 64-bit keys (capi_spans.hip).  Every radix sort of the search is
// instantiated in that one unit: the register count and the code the compiler gives a rocPRIM sort kernel depend on
// which other sorts the unit instantiates.  With these two in the tables' units, five kernels came out otherwise: the
// block sort of (u32, u32), the block sort of (u64, u32) in both its `const *` and plain-pointer forms (52 VGPRs against
// 48, the former without having left this unit), and the two onesweep iterations of (u64, u32).
int sort_target_keys(hipStream_t s, DevBuf &tmp, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits);
hipError_t sort_span_keys(void *tmp, size_t &bytes, uint64_t *kin, uint64_t *kout, uint32_t *vin, uint32_t *vout, size_t n, int bits, hipStream_t s);
// (What a table does with a sub-batch - its merge_* - is called from its own file alone: by its take() and by the entry
// points that merge a caller's list.)
} // namespace prb
