// What the stages of the search of one sub-batch share across their two units - capi_search.hip (search_page,
// search_range and every stage but one) and capi_gapped.hip (the gapped stage): the knobs of a search, the state of a
// sub-batch on its way through the stages, and the helpers on lists of hits that both sides use.
#pragma once
#include <functional>

#include "search_host.hpp"

namespace prb {

// ------------------------------------------------------------------------- knobs
// The environment of a search, read once per prb_search_page* call (INTEGRATION.md has the table; most exist for the
// tests, which compare the default path against the paths these select).  Not cached beyond the call: a process may
// change its environment between two searches.
struct SearchKnobs { // (read_search_knobs, capi_search.hip)
  double budget;       // pairs per sub-batch
  double chunk_pairs;  // pairs per chunk of candidates
  int row_shift;       // rows / pairs in (query, database position >> row_shift) order, see k_row_key; -1 keeps suffix-array order
  int sort_bits;       // the one-pass form's radix sort covers at most this many key bits from the top (pair_layout, search_host.hpp)
  bool local_order;    // ... and the tiles of k_seed_extend order the bits it leaves above the row shift (0: the sort takes them all)
  bool pair_wide;      // testing: the wide pair layout for every chunk
  bool fused;          // seeds -> hits under -f in one pass (0: written as a list, extended and thinned in separate passes)
  bool front_ahead;    // the front of the next sub-batch's seed path is issued while this one is extended
  bool sort_four_keys, sort_two_lengths;
  size_t big_list_bytes;  // a list behind -f beyond this takes the memory of stages already over (tests: every list)
  int64_t gapped_chunk_hits;
  int first_tier;      // the cascade starts at this kernel (4 = the wave-per-hit kernel alone), so the rarely taken kernels see every hit
  bool wave_hbm, no_resume, front_paired, front, handover;
  GapTierKnobs tiers;  // the experiments inside the LDS tiers (search_kernels.hpp)
  bool filter_tiles;   // the redundancy filter scans windows of the list in LDS (0: the plain kernels)
  int resume_cap;      // > 0, testing: pools that run out (those hits are redone instead)
  int skip_tiers;      // experiment: bit t set = LDS tier t is left out behind the front kernel
  bool trace_no_long, trace_no_slots; // testing: no long traces; re-extend every final hit as well
  int trace_long_cap, trace_slot_cap; // testing: pretend the slots are shorter
  int distinct_lds_hits; // testing: the LDS capacity of the distinct-sites selection (runs beyond it keep their state in HBM)
  int chain_lds_hits;    // testing: the same for the chain selection (PRB_CHAIN_LDS_HITS)
  bool debug_rows, debug_mem;
};

// ------------------------------------------------------------------------- state
// Field bounds of the hits of one sub-batch, for the one-key sort
struct SortBounds {
  int32_t qmin = 0, qspan = 1, max_qlen = 0, max_dblen = 0, nchars = 0;
  int32_t eq_len_max = 0; // > 0: every hit of the list has q_len = db_len <= this (the one-pass seed path reports it)
};

// What the search of a page is given: the same for all its sub-batches
struct PageSearch {
  prb_ctx *ctx;
  SearchWs &w;
  const prb_qbatch *qb;
  const DbPage &pg;
  const PageDev &pd;
  const SearchConst &sc;
  const ExtOpts eo;
  const prb_ris_opts &opts;
  const SearchKnobs &k;
  const int page, last_stage;
  const SearchMode mode;
  TableState *table; // SearchMode::kTable: where the final hits go
  prb_hitset *hs;
  int max_qlen;
  int32_t max_dblen;
  const AllowDev *allow = nullptr; // opts.allowed_pairs on the device, for this page; nullptr: every pair
};

// the candidates of a sub-batch: queries [q0, q1), in page-locked memory, rows and query entries numbered from 0
struct CandBatch {
  int32_t q0 = 0, q1 = 0;
  CandDev *cd = nullptr; // in query order, row0 / qoff filled in (each is rebased once, for its chunk)
  int64_t ncand = 0, nrows = 0, nqent = 0;
};

// One sub-batch on its way through the stages: what it is given, then what each stage hands to the ones behind it.
// (The lists themselves are in the workspace's buffers; the HitSoA views here say which.)
struct SubSearch : PageSearch {
  const CandBatch &b;
  // called at most once, behind the LDS tiers of the gapped cascade (the front stage's buffers are long free by then): the
  // caller's chance to issue the front of the NEXT sub-batch ahead (call_front_free)
  const std::function<void()> &front_free;
  bool front_called = false;
  int32_t ncand = 0;
  SortBounds sb;
  // seeds_to_hits: nf hits under the -f threshold, as records in w.hitsB
  int64_t nf = 0, one_pass_maxlen = 0;
  bool all_one_pass = true; // every chunk through k_seed_extend: lengths known, q_len = db_len
  // sort_filter_ungapped: the nung survivors
  int64_t nung = 0;
  // The gapped stage's view of the list: hits U -> G, `first` = their first-of-query flags, per-hit arrays indexed from
  // 0.  That is the whole list (U in w.hitsA) - or, while the stage runs in chunks, the chunk at hand, and behind it the
  // kept lists.  The traceback re-extends final hits through the same view.
  HitSoA U, G;
  const uint8_t *first = nullptr;
  int64_t nch = 0;        // hits in the view while the cascade runs
  bool chunked = false;
  int64_t nmax = 0;       // what the per-hit buffers of the stage hold
  int64_t ngap = 0;       // hits not above -g behind the stage, as records in w.hitsB (w.cidx: their indices in U)
  LongTrace lt{};         // long traces of wave-kernel hits (search_kernels.hpp)
  int32_t lt_used = 0;
  // what the traceback reads per hit of U: the stage's own arrays, or the kept lists when it ran in chunks
  const uint8_t *tier_all = nullptr;
  const int32_t *ntrace_all = nullptr;
  const uint16_t *trace_all = nullptr;
  // final_sort_filter: the nfin final hits F (w.hitsB), w.subset = the index of each one's pre-gapped state in U
  HitSoA F;
  int64_t nfin = 0;
  // traceback: base pairs in all (w.bpCount / w.bpOff / w.bpOut hold them per hit)
  int64_t bp_total = 0;
};

inline void call_front_free(SubSearch &s) {
  if (s.front_free && !s.front_called) {
    s.front_free();
    s.front_called = true;
  }
}

// ------------------------------------------------------------------------- lists of hits (defined in capi_search.hip)
HitSoA carve_hits(uint8_t *p, int64_t n); // the columns of n hits in the block at p
inline HitSoA carve_hits(DevBuf &b, int64_t n) { return carve_hits(b.as<uint8_t>(), n); }
inline size_t hits_bytes(int64_t n) { return (((size_t)n + 1) & ~(size_t)1) * kHitBytes + 64; }
// the hits from `first` on, as a list of their own
inline HitSoA offset_hits(const HitSoA &h, int64_t first) {
  return HitSoA{h.q_sp + first, h.db_sp + first, h.q_len + first, h.db_len + first, h.db_id + first, h.db_id_start + first,
                h.query + first, h.e_acc + first, h.e_hyb + first, h.e_tot + first};
}
// `need` bytes in a buffer whose first `have` bytes are kept
int grow_keep(prb_ctx *ctx, DevBuf &buf, size_t have, size_t need, size_t spare_limit = SIZE_MAX);
// recbuf <- the hits of `in` that are not above `thr`, as records behind the `have` it holds; idxbuf[i] = index in `in`
int compact_below(prb_ctx *ctx, SearchWs &w, const HitSoA &in, int64_t n, double thr, DevBuf &idxbuf, DevBuf &recbuf, int64_t *m,
                  int64_t have = 0);

// ------------------------------------------------------------------------- the gapped stage (capi_gapped.hip)
// s.U -> s.G through the cascade of gapped kernels (whole, or in chunks of which only the hits under -g are kept)
int gapped_stage(SubSearch &s);
// the traceback's second extension: the base pairs of the m hits `subset2` (device; indices into s.U) that `tier`
// completed, written at bpOff2[0 .. m) in w.bpOut
int retrace_tier(SubSearch &s, int tier, const uint32_t *subset2, const int64_t *bpOff2, int64_t m);

} // namespace prb
