// Host-visible interface of the interaction-search kernels: the structs the device sees, then one section per kernel
// file in the order of the pipeline - seed expansion, ungapped extension, sort, redundancy filter, gapped extension,
// traceback - and behind it the output modes' own stages (pair summaries and distinct sites, top-N tables, per-target
// table, profile, coverage).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace prb {

// ============================================================================ device-visible structs
// Integer Turner tables (0.01 kcal/mol) as used by the extension stages
// (ungapped_extension.cpp:157-186, gapped_extension.cpp:366-399, 426-473).
// layout of the concatenated integer table `SearchConst::tab`
struct SearchTab {
  static constexpr int kStack = 0;                 // [7][7]
  static constexpr int kInternal = kStack + 49;    // [31]
  static constexpr int kMismatchI = kInternal + 31; // [7][5][5]
  static constexpr int kInt11 = kMismatchI + 175;  // [8][8][5][5]
  static constexpr int kInt21 = kInt11 + 1600;     // [8][8][5][5][5]
  static constexpr int kInt22 = kInt21 + 8000;     // [8][8][5][5][5][5]
  static constexpr int kDangle5 = kInt22 + 40000;  // [8][5]
  static constexpr int kDangle3 = kDangle5 + 40;   // [8][5]
  static constexpr int kBulge = kDangle3 + 40;     // [31] bulge37
  static constexpr int kTau = kBulge + 31;         // [8] TerminalAU if pair type > 2 else 0
  static constexpr int kZero = kTau + 8;           // one 0
  static constexpr int kCount = kZero + 1;
};

struct SearchConst {
  const int32_t *tab;       // SearchTab
  const int32_t *stack37;   // [7][7]
  const int32_t *internal37; // [31]
  const int32_t *mismatchI37; // [7][5][5]
  const int32_t *int11;     // [8][8][5][5]
  const int32_t *int21;     // [8][8][5][5][5]
  const int32_t *int22;     // [8][8][5][5][5][5]
  const int32_t *dangle5;   // [8][5]
  const int32_t *dangle3;   // [8][5]
  const double *bulge;      // [64]: bulge37[u] for u <= 30, logarithmic extrapolation beyond
  int32_t terminal_au;
  // BP_pair (energy_par.hpp:17-23) packed 3 bits per entry, row a (1..4) at bit 15*(a-1);
  // rtype (energy_par.hpp:26) is the involution ((t-1)^1)+1, checked on the host
  uint64_t bp_rows;
  uint32_t pair_mask, wobble_mask; // bit 5 * a + b: bases a, b pair / form a wobble pair (types 3, 4)
  unsigned char bp_pair[25];
};

struct PageDev {
  const uint8_t *seqs; // page text: reversed sequences, 0 after each
  const int32_t *sa;
  const int32_t *sa_seq;  // sequence that SA entry k lies in (GetSeqIdAndStart's search, done once per page)
  const int32_t *blk_seq; // sequence that character 32 b of the page text lies in (b = 0 .. (nchars - 1) / 32)
  const int32_t *start_pos;
  const int32_t *seq_length;
  const float *acc;  // padded to L per sequence; sequence id at start_pos[id] - id
  const float *cond;
  int32_t nchars, nseq;
};

struct QBatchDev {
  const uint8_t *enc;   // query q at off[q], L+1 codes (trailing 0)
  const int32_t *sa;    // same offsets
  const float *acc;     // same offsets (L values + one 0)
  const float *cond;
  const int64_t *off;
  const int32_t *len;   // L
  int32_t nq;
};

struct CandDev { // SeedCandidate + first row of the candidate (one row per db SA entry)
  int32_t sp_q, ep_q, sp_db, ep_db, length, query;
  double score;
  int64_t row0;
  int64_t qoff; // first of the candidate's ep_q - sp_q + 1 entries in the query-side window sums
};

// The pairs a search is restricted to (prb_pairmask, include/priblast_hip.h): a bit per (query of the batch, target of
// the database), row q at bits + q * row_words; tbase = the number of the first target of the page being searched
struct AllowDev {
  const uint32_t *bits;
  int64_t row_words, tbase;
};
__host__ __device__ inline bool pair_allowed(const AllowDev &a, int query, int db_id) {
  const int64_t t = a.tbase + db_id;
  return (a.bits[(int64_t)query * a.row_words + (t >> 5)] >> (t & 31)) & 1u;
}

struct HitSoA {
  int32_t *q_sp, *db_sp, *q_len, *db_len, *db_id, *db_id_start, *query;
  double *e_acc, *e_hyb, *e_tot;
};
constexpr int kHitInts = 7, kHitDoubles = 3;
constexpr size_t kHitBytes = kHitInts * 4 + kHitDoubles * 8;

struct ExtOpts {
  int32_t delta;       // min accessible length
  int32_t drop_wo_gap; // -y
  int32_t drop_w_gap;  // -x
  int32_t min_helix;   // -m
};

// The hits between a threshold compaction and the sort behind it, one 64-byte record each: the sort
// ends in a gather in random order, which then costs one cache line per hit instead of one per field.
struct alignas(16) HitRec {
  int32_t q_sp, db_sp, q_len, db_len, db_id, db_id_start, query, pad0;
  double e_acc, e_hyb, e_tot;
  int64_t pad1;
};
static_assert(sizeof(HitRec) == 64, "one cache line half, two per 128-byte line");

// ============================================================================ seed_kernels.hip: seed expansion
// sa_seq[k] for every SA entry of a page
hipError_t launch_sa_seq(const PageDev &pg, int32_t *sa_seq, hipStream_t s);
// qacc[c.qoff + t] = accessibility energy of the query window of candidate c at its SA entry sp_q + t
hipError_t launch_seed_qacc(const CandDev *cands, int32_t ncand, int64_t nq_entries, const QBatchDev &qb, int delta, double *qacc,
                            hipStream_t s);
// every row its candidate (row_cand) and the key to sort the rows by: (query - qmin) << dbits | position in the page
// text >> shift; 64-bit keys if `wide`, else 32-bit; val = the row
hipError_t launch_row_keys(const CandDev *cands, int32_t ncand, int64_t nrows, const PageDev &pg, int qmin, int shift, int dbits,
                           bool wide, int32_t *row_cand, void *key, uint32_t *val, hipStream_t s);
// the two passes over the rows: seeds per row, then the seeds themselves at the scanned offsets.  row_perm (optional,
// both passes alike): the order in which the rows are taken, launch_row_keys' rows sorted by key
hipError_t launch_seed_count(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                             int delta, const double *qacc, int32_t *row_count, int32_t *row_cand, const uint32_t *row_perm,
                             hipStream_t s);
hipError_t launch_seed_emit(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                            int delta, const double *qacc, const int32_t *row_cand, const int64_t *row_off, HitSoA hits,
                            const uint32_t *row_perm, hipStream_t s);
// The same two passes under a pair mask: a row - one (candidate, database entry), so one (query, target) pair - that is
// not allowed counts no seed, and the emit pass skips the rows that counted none.  (Kernels of their own: the passes
// above are what they were.)
hipError_t launch_seed_count_allowed(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                                     int delta, const double *qacc, int32_t *row_count, int32_t *row_cand, const uint32_t *row_perm,
                                     const AllowDev &allow, hipStream_t s);
hipError_t launch_seed_emit_allowed(const CandDev *cands, int32_t ncand, int64_t nrows, const QBatchDev &qb, const PageDev &pg,
                                    int delta, const double *qacc, const int32_t *row_cand, const int64_t *row_off, HitSoA hits,
                                    const uint32_t *row_perm, const AllowDev &allow, hipStream_t s);

// ============================================================================ ungapped_kernels.hip: ungapped extension
// the walk on a list of seed hits, in place
hipError_t launch_ungapped(HitSoA hits, int64_t n, const QBatchDev &qb, const PageDev &pg, const SearchConst &sc,
                           ExtOpts o, int max_query_len, hipStream_t s);
// blk_seq for a page (PageDev::blk_seq, blk_seq_entries(nchars) values)
inline int64_t blk_seq_entries(int64_t nchars) { return (nchars >> 5) + 1; }
hipError_t launch_blk_seq(const PageDev &pg, int32_t *blk_seq, hipStream_t s);
// Seeds to extended hits in one pass over the (query SA entry, database SA entry) pairs of a chunk of candidates
// (ungapped_kernels.hip, "seeds -> extended hits in one pass").  pair0[c] = first pair of candidate c; at most
// kMaxFusedCands candidates of at most kMaxFusedEntries query entries each.
constexpr int64_t kMaxFusedCands = 1 << 20, kMaxFusedEntries = 1 << 12;
// How the pairs of a chunk are held between launch_pair_keys, the radix sort and launch_seed_extend (chosen by
// pair_layout, search_host.hpp).  The order wanted is (query, database position >> row shift), for locality only.
//   narrow  key   u32 (query - first query) << pbits | database position; sorted on its bits [begin, kbits) alone,
//           value u32 candidate : 20 | query entry within the candidate : 12
//   wide    key   u32 or u64 (query - first query) << pbits | database position >> shift; sorted on all kbits bits,
//           value u64 database position : 32 | candidate : 20 | query entry : 12
struct PairLayout {
  bool narrow = false;
  int shift = 0;      // wide: the key holds the position >> shift (narrow: 0, the key holds the position itself)
  int pbits = 0;      // bits of the key's position part
  int kbits = 0;      // bits of the whole key: the end bit of the sort (0: no pair sort at all, suffix-array order)
  int begin = 0;      // the begin bit of the sort
  int local_bits = 0; // narrow: key bits [begin - local_bits, begin) are put in order tile by tile in launch_seed_extend
  bool wide_key() const { return !narrow && kbits > 32; }
  size_t key_bytes() const { return wide_key() ? 8 : 4; }
  size_t val_bytes() const { return narrow ? 4 : 8; }
};
constexpr int kPairLocalBits = 5; // a tile is ordered on at most as many bits (32 buckets of ~64 pairs, a wavefront each)
hipError_t launch_pair_keys(const CandDev *cands, const int64_t *pair0, int32_t ncand, int64_t npairs, const PageDev &pg, int qmin,
                            const PairLayout &lay, void *key, void *val, hipStream_t s);
// Under a pair mask, between launch_pair_keys and the sort: the pairs whose (query, target) is allowed, compacted in
// order.  launch_allow_test: pair p's bit - the query of its candidate, the sequence of its database entry (sa_seq) - as
// one ballot word and one count per 64 pairs (allow_words(npairs) of each, and one more count, a zero, for the scan);
// launch_allow_scatter: behind the exclusive scan `off` of the counts, the allowed pairs' keys and values to their places.
inline int64_t allow_words(int64_t npairs) { return (npairs + 63) / 64; }
hipError_t launch_allow_test(const CandDev *cands, const int64_t *pair0, const void *val, const PairLayout &lay, int64_t npairs,
                             const PageDev &pg, const AllowDev &allow, uint64_t *ballot, int32_t *count, hipStream_t s);
hipError_t launch_allow_scatter(const void *key_in, const void *val_in, int64_t npairs, const PairLayout &lay, const uint64_t *ballot,
                                const int64_t *off, void *key_out, void *val_out, hipStream_t s);
// A workgroup takes kFusePairs pairs and keeps what survives in its slice of `slices` (kFusePairs records of
// kSliceRecBytes each), slice_count[b] of them; nseed[0] += seeds, nseed[1] = max(nseed[1], length of the longest hit
// kept).  keys, vals = the sorted pairs in the layout `lay` (the wide one reads no keys).  launch_collect_slices packs the
// slices into `out` (slice b at slice_off[b] = the exclusive scan of the counts).
constexpr int kFusePairs = 2048, kSliceRecBytes = 48;
inline int64_t fused_slices(int64_t npairs) { return (npairs + kFusePairs - 1) / kFusePairs; }
hipError_t launch_seed_extend(const CandDev *cands, const void *keys, const void *vals, const PairLayout &lay, int64_t npairs,
                              const QBatchDev &qb, const PageDev &pg, const SearchConst &sc, ExtOpts o, const double *qacc, double thr,
                              int max_query_len, void *slices, int32_t *slice_count, uint64_t *nseed, hipStream_t s);
hipError_t launch_collect_slices(const void *slices, const int32_t *slice_count, const int64_t *slice_off, int64_t nslices, HitRec *out,
                                 hipStream_t s);

// ============================================================================ sort_kernels.hip: sort keys, gathers, flags
// One-key form of the sort (when the fields fit 64 bits): field widths and the offsets
struct PackedKeyInfo {
  int32_t qmin, lmax; // first query of the sub-batch; upper bound of q_len / db_len
  int32_t bl, bq, bd; // bits of a length, of q_sp, of db_sp
  int32_t one_len = 0; // every hit has q_len = db_len (hits extended without gaps): the key holds the length once
};
hipError_t launch_make_packed_keys(const HitSoA &hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                   uint32_t *idx, hipStream_t s);
hipError_t launch_make_packed_keys_recs(const HitRec *hits, int64_t n, const PackedKeyInfo &f, uint64_t *key, uint64_t *k_energy,
                                        uint32_t *idx, hipStream_t s);
// after the stable sort by the packed key: perm_out = perm with every run of equal keys put in (energy, its parts,
// input index) order; *too_long is set if a run is longer than the kernel handles (the caller then sorts by the four
// keys instead)
hipError_t launch_fix_ties(const uint64_t *key_sorted, const uint64_t *e_sorted, const uint32_t *perm, int64_t n, const HitRec *recs,
                           uint32_t *perm_out, int32_t *too_long, hipStream_t s);
// the four keys of that sort
hipError_t launch_make_keys(const HitSoA &hits, int64_t n, uint64_t *k_energy, uint32_t *k_len, uint32_t *k_qsp,
                            uint64_t *k_pos, uint32_t *idx, hipStream_t s);
hipError_t launch_order_keys(const double *v, int64_t n, uint64_t *key, hipStream_t s); // monotone u64 image of doubles
hipError_t launch_gather_u64(const uint64_t *src, const uint32_t *idx, uint64_t *dst, int64_t n, hipStream_t s);
hipError_t launch_gather_u32(const uint32_t *src, const uint32_t *idx, uint32_t *dst, int64_t n, hipStream_t s);
hipError_t launch_gather_u8(const uint8_t *src, const uint32_t *idx, uint8_t *dst, int64_t n, hipStream_t s);
hipError_t launch_iota_u32(uint32_t *dst, int64_t n, hipStream_t s); // dst[i] = i
// dst row r = src row idx[r], rows of row_bytes (a multiple of 16) bytes
hipError_t launch_gather_rows(const void *src, const uint32_t *idx, void *dst, int64_t n, int row_bytes, hipStream_t s);
hipError_t launch_gather_hits(const HitSoA &src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s);
hipError_t launch_gather_hits_to_recs(const HitSoA &src, const uint32_t *idx, HitRec *dst, int64_t n, hipStream_t s);
// idx == nullptr: in order
hipError_t launch_gather_recs_to_hits(const HitRec *src, const uint32_t *idx, HitSoA dst, int64_t n, hipStream_t s);
// flags[i] = marks[list[i]] & mask != 0
hipError_t launch_flag_marked(const uint8_t *marks, const uint32_t *list, int64_t n, uint8_t mask, uint8_t *flags, hipStream_t s);
// keep[i] = 1 unless e_tot[i] > thr
hipError_t launch_flag_not_above(const double *e_tot, int64_t n, double thr, uint8_t *keep, hipStream_t s);
// first[i] = 1 for the first hit of every query of a query-sorted list
hipError_t launch_mark_first(const int32_t *query, int64_t n, uint8_t *first, hipStream_t s);
// out: n records of prb_hit (include/priblast_hip.h) in device memory; bp_base >= 0 also fills their
// base-pair ranges (bp_count / bp_off per hit, or 2 pairs per hit when those are null)
hipError_t launch_pack_hits(const HitSoA &src, int64_t n, const int32_t *bp_count, const int64_t *bp_off, int64_t bp_base,
                            void *out, hipStream_t s);

// ============================================================================ filter_kernels.hip: redundancy filter
// On a sorted list.  state: 0 unknown, 1 active, 2 inactive; keep[i] = 1 for survivors.  tiles: the forms that scan a
// window of the list in LDS (the default; PRB_FILTER_TILES=0 selects the plain ones)
hipError_t launch_filter_init(const HitSoA &h, int64_t n, double thr, int64_t *db_end_key, uint8_t *state, hipStream_t s);
hipError_t launch_filter_round(const HitSoA &h, int64_t n, const int64_t *pmax, uint8_t *state, int32_t *pending, bool tiles,
                               hipStream_t s);
hipError_t launch_filter_final(const HitSoA &h, int64_t n, const int64_t *pmax, const uint8_t *state, uint8_t *keep, bool tiles,
                               hipStream_t s);

// ============================================================================ gapped_lds.hip: gapped extension
constexpr size_t kGapWaveLdsBytes = 64 * 1024; // a state block up to this size can live in the workgroup's LDS
struct GapScratch {
  uint8_t *base;         // one block per wavefront; nullptr = in the wavefront's (dynamic) LDS
  size_t bytes_per_wave; // bytes per block = gapped_wave_scratch_bytes(cap_diag, cap_rec)
  int32_t cap_rec, cap_diag;
  int32_t nwaves;        // wavefronts that own a state block (= grid size)
};
size_t gapped_wave_scratch_bytes(int cap_diag, int cap_rec);
// State dumps of the hits that outgrow LDS tier 0 / tier 1 (mode 0): the next tier continues from
// them instead of starting over.  slot[x] = -1 or the hit's dump; pool = cap dumps of
// gapped_resume_bytes(tier that writes them) each; *count = dumps taken so far (zero it together
// with the slots).  All null / 0: no dumps.  A launch gets the pool it may continue (rin: tier 1
// <- tier 0's, tier 2 <- tier 1's) and the pool it fills (rout: tiers 0 and 1).
struct GapResume {
  int32_t *slot = nullptr;
  uint8_t *pool = nullptr;
  uint32_t *count = nullptr;
  int32_t cap = 0;
};
size_t gapped_resume_bytes(int tier);
// ids of the gapped kernels a hit can be completed by (tier_out): LDS tiers 0..3, then the
// wavefront-per-hit kernel with its state in HBM scratch
constexpr int kLdsTiers = 4, kWaveTier = 4;
// The experiments of the LDS tiers, as the driver read them from the environment (read_search_knobs, capi_search.hip -
// SearchKnobs::tiers, search_stages.hpp;
// INTEGRATION.md has the table).  The per-tier lists count only where their variable is set.
struct GapTierKnobs {
  bool pair = true; // PRB_GAPPED_PAIR: tier 0 takes two anti-diagonals per step (0: one)
  bool pool = true; // PRB_GAPPED_POOL: the filled cells of such a step pooled over the wavefront (0: each group its own)
  bool pad_set = false, period_set = false, early_set = false;
  int pad[kLdsTiers] = {};    // PRB_GAPPED_LDS_PAD "b1,b2,b3": unused dynamic LDS per workgroup of tiers 1 - 3 (mode 0, not tier 0's paired form)
  int period[kLdsTiers] = {}; // PRB_GAPPED_PERIOD "p0,p1,p2,p3": GapArgs::period per tier (mode 0)
  int early[kLdsTiers] = {};  // PRB_GAPPED_EARLY "k0,k1,k2,k3": GapArgs::early per tier, in place of the default 0,0,2,0
};
// Trace slots: the extension pass (mode 0, LDS tiers) leaves the first kTraceCap cells (i | j << 8)
// of each direction's traceback chain of hit x at trace[(2x + direction) * kTraceCap ...];
// launch_bp_expand writes the base pairs of the final hits from them (hits of the wave kernel or
// with longer chains are skipped: they are traced by a mode-2 pass).
constexpr int kTraceCap = 32;
// Long traces: the wavefront-per-hit kernel (mode 0) leaves the whole traceback chain of a direction it ran - cells as
// i | j << 16 - in a pool of its own, trace[(2 * slot[x] + direction) * cap ...], and count[2 * slot[x] + direction] = its
// length (-1: the direction was not run by this kernel - an LDS tier's trace slot has it -, -2: longer than cap).  A hit
// whose two chains are all there is reported as kLongTraceTier instead of kWaveTier, and launch_bp_expand writes its pairs
// from them: no second extension of the ~150 longest hits of a query (2 - 3 ms on an otherwise idle GPU).
constexpr int kLongTraceTier = 5;
struct LongTrace {
  uint32_t *trace = nullptr;
  int32_t *count = nullptr;
  const int32_t *slot = nullptr; // per hit x; -1: none
  int32_t cap = 0;
};
// tier_out[x] of a hit whose first direction is done and whose second one is somebody else's business: out.*[x] and
// bp_count[x] hold its state after direction 0.  kResumeMark: the next kernel of the cascade extends the other
// direction (a hit that outgrew a kernel in direction 1, or that the front kernel handed on with a first direction that
// finds nothing).  kHandoverMark: an LDS tier stopped behind direction 0 on purpose (GapArgs::handover): the second
// direction goes to the front kernel first - it finds nothing nine times in ten, which that kernel proves at a fraction of
// a tier's cost.  The low three bits are the LDS tier that has room for the first direction: a hit is reported as the
// larger of the tiers its two directions needed (the tier that would have to extend it again for its pairs).
constexpr uint8_t kResumeMark = 0x40, kHandoverMark = 0x80, kMarkTier = 0x07;
__host__ __device__ inline bool is_resumed(uint8_t t) { return (t & (kResumeMark | kHandoverMark)) != 0; }
// What a gapped kernel is launched with: the driver (capi_gapped.hip) fills it by name, the launchers below take it and
// set what is their kernel's own business.  Passed to the kernels by value.  mode 0: extend the n hits of the list
// `subset` (indices into in / out and the per-hit arrays; nullptr: 0..n-1) into `out`; mode 2: write the base pairs of
// list entry w at bp_off[w] (hits beyond the kernel's capacity are skipped).  A field that names a mode or a kernel is
// read by no other.
struct GapArgs {
  HitSoA in{}, out{}; // coordinates and energies before / behind the extension
  int64_t n = 0;
  const uint32_t *subset = nullptr;
  QBatchDev qb{};
  PageDev pg{};
  SearchConst sc{};
  ExtOpts o{};
  uint8_t *overflow = nullptr; // mode 0: overflow[w] = 1 if the capacities of this kernel did not suffice
  uint8_t *tier_out = nullptr; // mode 0: tier_out[x] = tier_id when hit x was completed here (the front kernel: its `tier_id`, 0)
  int tier_id = 0;             // set by launch_gapped_lds (its tier) and launch_gapped_wave (kWaveTier)
  const uint8_t *first_flag = nullptr; // mode 2: first_flag[x] = 1 for the first hit of a query, whose pairs keep the order they were found in
  int32_t *bp_count = nullptr; // mode 0: traced pairs of hit x, left | right << 16
  uint16_t *trace = nullptr;   // mode 0 (LDS tiers): the first kTraceCap traced cells (i | j << 8) per direction of hit x
  const int64_t *bp_off = nullptr; // mode 2: where the pairs of list entry w go in bp_out
  int32_t *bp_out = nullptr;   // mode 2: the pairs, (q, db) each
  unsigned long long *next_work = nullptr; // LDS and front kernels: 8 bytes of scratch, the work counter (zeroed by the launcher) behind the statically assigned first hits
  // mode 0: state dumps of hits that outgrow an LDS tier, for the next one to continue from
  // (slot[x] = -1: none): `rin` = what this kernel may continue, `rout` = where it leaves its own
  GapResume rin{}, rout{};
  LongTrace lt{};   // mode 0, the wavefront-per-hit kernel: where it leaves whole traceback chains
  double *acc_scratch = nullptr; // LDS tiers: gapped_acc_scratch_bytes() of device memory, 2 x capacity doubles per resident group
  // set by launch_gapped_lds from GapTierKnobs:
  int period = 0;   // LDS tiers: lockstep iterations between the boundaries at which groups change direction / hit (0: the drop-out length)
  int early = 0;    // LDS tiers: a boundary also as soon as this many groups of the wavefront have finished their direction (0: never)
  int pool = 1;     // tier 0 with two anti-diagonals per step: the filled cells of a step pooled over the wavefront (0: each group its own)
  int handover = 0; // mode 0, LDS tiers and the wavefront-per-hit kernel: stop behind a first direction that this kernel ran (kHandoverMark)
};
// launch_gapped_lds: a group of lanes per hit, state in LDS with fixed capacities: tiers 0 and 1 = 8 lanes (32 and 40
// anti-diagonals), tier 2 = 16 lanes, 64 anti-diagonals; tier 3 = a wavefront, 128 anti-diagonals.  Passes `handover`
// on only in mode 0, and no `lt`.
hipError_t launch_gapped_lds(const GapArgs &a, int mode, int tier, const GapTierKnobs &knobs, hipStream_t s);
size_t gapped_acc_scratch_bytes();
// launch_gapped_wave: one wavefront per hit, state in the scratch (`scratch.nwaves` wavefronts).  Passes `lt` and
// `handover` on only in mode 0, and no `trace`, `next_work`, `rin` or `rout`.
hipError_t launch_gapped_wave(const GapArgs &a, GapScratch scratch, int mode, hipStream_t s);

// ============================================================================ gapped_front.hip: in front of the cascade
// launch_gapped_front proves that a direction finds nothing within its `-x` anti-diagonals (phases that are dense over
// directions / filled cells / (cell, candidate) pairs of 64 directions at a time) and completes the hits whose two directions both find nothing; the others are flagged in
// overflow[] (with direction 0 handed over when it found nothing) and go on to the LDS tiers.  Completed hits are
// reported as `tier_id`.  Takes -x <= kFrontMaxDrop.  Mode 0 only; passes no `first_flag`, `trace`, `bp_off`, `bp_out`,
// `rin` or `rout` on.  second_only: every hit of the list has its first direction done (a resume / hand-over mark).
constexpr int kFrontMaxDrop = 16;
bool gapped_front_supported(const SearchConst &sc, const ExtOpts &o);
size_t gapped_front_scratch_bytes(); // HBM scratch of a launch (accessibility sums of the resident wavefronts; stays in L2)
hipError_t launch_gapped_front(const GapArgs &a, void *scratch, bool second_only, hipStream_t s);

// ============================================================================ traceback_kernels.hip: base pairs
// slot[list[p]] = base + p (the long-trace slots of the hits that go to the wavefront-per-hit kernel)
hipError_t launch_assign_slots(const uint32_t *list, int64_t n, int32_t base, int32_t *slot, hipStream_t s);
// bp_count[w] = total pairs of list entry w: its ungapped diagonal's plus what the two extensions traced (ntrace)
hipError_t launch_bp_count(const HitSoA &in, int64_t n, const uint32_t *subset, const QBatchDev &qb, const PageDev &pg,
                           const SearchConst &sc, const int32_t *ntrace, int32_t *bp_count, hipStream_t s);
// the pairs of list entry w at bp_off[w], from the trace slots and long traces of the extension pass
hipError_t launch_bp_expand(const HitSoA &in, int64_t n, const uint32_t *subset, const QBatchDev &qb, const PageDev &pg,
                            const SearchConst &sc, const uint8_t *first_flag, const int32_t *ntrace, const uint8_t *tier_of,
                            const uint16_t *trace, const LongTrace &lt, const int64_t *bp_off, int32_t *bp_out, hipStream_t s);
// ends[4w .. 4w + 3] = first and last pair (q0, db0, qN, dbN) of list entry w
hipError_t launch_bp_ends(const int64_t *bp_off, int64_t n, const int32_t *bp, int32_t *ends, hipStream_t s);

// ============================================================================ site_kernels.hip: (query, db_id) runs
// ---- per-pair summaries (prb_search_page_summary) over a final, sorted hit list ----
// head[i] = 1 where (query, db_id) differs from hit i - 1 (and for i = 0): the first hit of every pair
hipError_t launch_pair_heads(const int32_t *query, const int32_t *db_id, int64_t n, uint8_t *head, hipStream_t s);
// one lane per pair k, hits [start[k], start[k + 1]) (the last one up to n), walked in order: count, first minimum of
// e_tot, left-to-right sum; writes prb_pair_summary records with the best hit's e_acc / e_hyb and its two end pairs
// from `ends` (4 ints per hit, launch_bp_ends)
hipError_t launch_pair_fold(const HitSoA &h, int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, void *out,
                            hipStream_t s);
// ---- distinct interaction sites (prb_ris_opts::distinct_sites) over a final, sorted hit list ----
// keep[i] = 1 for the hits that the greedy selection of include/priblast_hip.h keeps within their run, 0 for the others;
// head = launch_pair_heads' flags (a caller's list: any flags that start a run at hit 0).  Two launches: runs of up to
// 64 hits several per wavefront, state in registers; the longer ones, which the first launch lists in w.long_list, a
// workgroup each - with rectangles and state in LDS up to lds_hits hits (clamped to 1 .. kSiteLdsHits; below 64 it
// also lowers the first launch's limit, so that tests reach the other paths with short runs), beyond that read from
// the list with the state in w.lo / w.hi / w.state.  Nothing comes back to the host.  n <= INT32_MAX.
constexpr int kSiteLdsHits = 2048; // 31 bytes of LDS per hit
constexpr int kSiteLongGrid = 1024;
inline int64_t site_long_runs_max(int64_t n) { return n / 2 + 1; } // a listed run has two hits at least
struct SiteScratch {
  uint32_t *long_list; // site_long_runs_max(n) entries
  uint32_t *nlong;     // one counter
  int32_t *lo, *hi;    // n entries each
  uint8_t *state;      // n entries
};
hipError_t launch_site_select(const HitSoA &h, int64_t n, const uint8_t *head, int lds_hits, const SiteScratch &w, uint8_t *keep,
                              hipStream_t s);
// ---- best co-linear chain of sites (prb_ris_opts::chain_sites) over a final hit list sorted by db_sp inside its runs ----
// keep[i] = 1 for the hits of their run's best chain (the dynamic programme of include/priblast_hip.h), 0 for the
// others; head as above.  Two launches of the same shape as launch_site_select's: runs of up to 64 hits several per
// wavefront, scores and predecessors in registers; the longer ones, listed in w.long_list, a workgroup each in tiles
// of 64 hits - with rectangles, energies, scores and predecessors in LDS up to lds_hits hits (clamped to
// 1 .. kChainLdsHits; below 64 it also lowers the first launch's limit), beyond that read from the list with scores and
// predecessors in w.score / w.prev.  Nothing comes back to the host.  n <= INT32_MAX.
constexpr int kChainLdsHits = 1536; // 36 bytes of LDS per hit
struct ChainScratch {
  uint32_t *long_list; // site_long_runs_max(n) entries
  uint32_t *nlong;     // one counter
  double *score;       // n entries
  int32_t *prev;       // n entries
};
hipError_t launch_chain_select(const HitSoA &h, int64_t n, const uint8_t *head, int lds_hits, const ChainScratch &w, uint8_t *keep,
                               hipStream_t s);

// ============================================================================ table_kernels.hip: top-N tables
// ---- top-N table (prb_search_page_top) ----
constexpr int kTopMaxN = 1024; // the largest N: the set's keys and a candidate buffer of as many fit a workgroup's LDS
// merges the pair records rec[0, nrec) (prb_pair_summary, launch_pair_fold's output for queries [q0, q1), ascending by
// query) of `page` into the table: tab = prb_top_pair[nq * n] (slot `rank` = the pair's ordinal while on the device),
// fill = int32_t[nq] (slots in use per query).  One workgroup per query; the page must not be in the table yet.
hipError_t launch_top_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                            hipStream_t s);
// ---- top-N hit table (prb_search_page_tophits) ----
// the same merge for final hits: rec = prb_hit[nrec] (launch_pack_hits' output for queries [q0, q1), ascending by query),
// ranked by e_tot, then page, then the hit's place among its query's hits of the page; tab = prb_top_hit[nq * n]
hipError_t launch_tophits_merge(const void *rec, int64_t nrec, int32_t q0, int32_t q1, int32_t page, int32_t n, void *tab, int32_t *fill,
                                hipStream_t s);
// cnt[i] = the base pairs of slot i of the table (0 for a slot not in use), i < nslots = nq * n; cnt[nslots] = 0, so that
// an exclusive scan over nslots + 1 values ends with the total
hipError_t launch_tophits_counts(const void *tab, const int32_t *fill, int32_t n, int64_t nslots, int32_t *cnt, hipStream_t s);
// The kept hits' base-pair lists gathered into `pool` in table order: slot i's list goes to pair off[i].  Its source is
// `old_pool` at the slot's bp_offset when that is below `split` (the old pool's pairs), else `fresh` at bp_offset - split:
// the newcomers' lists (this sub-batch's pairs, with launch_pack_hits' offsets counted from `split` on; or the pool of the
// table that launch_tophits_join took them from); the slot's bp_offset becomes off[i].  All three arrays are (q, db) pairs
// of two int32.
hipError_t launch_tophits_gather(void *tab, const int32_t *fill, int32_t n, int64_t nslots, const int64_t *off, int64_t split,
                                 const int32_t *old_pool, const int32_t *fresh, int32_t *pool, hipStream_t s);
// ---- two tables over disjoint page sets into one (prb_topset_merge, prb_tophits_merge) ----
// per query, tab's and src's ranked slots in use merged under the tables' order, the first n kept, in tab (src is only
// read); one workgroup per query, nq of them.  launch_tophits_join adds `shift` to the bp_offset of every record it
// takes from src.
hipError_t launch_top_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, hipStream_t s);
hipError_t launch_tophits_join(void *tab, int32_t *fill, const void *src, const int32_t *src_fill, int32_t nq, int32_t n, int64_t shift,
                               hipStream_t s);

// ============================================================================ profile_kernels.hip: per-position profile
// (prb_search_page_profile)
// The table of one batch in HBM.  Query q owns the slots [off[q], off[q + 1]) = its len + 1 positions (the last one
// takes the -1 of a span that ends at the query's last base), so the difference arrays of all queries are one array
// whose every query segment sums to zero.  Best-hit keys: key = energy key of e_tot, tie = page << 32 | the hit's place
// in the page's final list; ~0 = none yet.  skey / stie: the (energy key, place) minima of the sub-batch being merged,
// ~0 between sub-batches.  bad: set when a hit's span lies outside its query (never for a consistent search).
struct ProfTab {
  const int64_t *off;           // [nq + 1]
  unsigned long long *hdiff;    // [P] hits: +1 at a span's first position, -1 behind its last (two's complement)
  unsigned long long *key, *tie; // [P] the best hit so far
  unsigned long long *skey;     // [P] sub-batch scratch
  double *e_min;                // [P] the best hit's e_tot
  int32_t *tdiff;               // [P] targets: the same over the union of each pair's spans
  uint32_t *stie;               // [P] sub-batch scratch
  int32_t *db_id;               // [P] the best hit's sequence
  int32_t *bp;                  // [4 P] the best hit's first and last base pair (q, db, q, db)
  uint32_t *bad;
  int32_t nq;
};
// key[i] = pair << 32 | first query position of final hit i's span, val[i] = i (start = the pairs' first hits, as
// launch_pair_fold takes them; ends = launch_bp_ends)
hipError_t launch_prof_keys(int64_t n, const uint32_t *start, int64_t npairs, const int32_t *ends, uint64_t *key, uint32_t *val,
                            hipStream_t s);
// v[i] = (key[i] with its position bits cleared) | (last position of hit val[i]'s span + 1): what the max-scan takes
hipError_t launch_prof_span(int64_t n, const uint64_t *key, const uint32_t *val, const int32_t *ends, uint64_t *v, hipStream_t s);
// the difference arrays: every hit's span into hdiff, and the part of it that no earlier hit of its pair (in key order)
// covers into tdiff; m = the inclusive max-scan of launch_prof_span's v
hipError_t launch_prof_add(const HitSoA &h, int64_t n, const uint64_t *key, const uint32_t *val, const uint64_t *m, const int32_t *ends,
                           const ProfTab &t, hipStream_t s);
// the sub-batch's minima: skey = smallest energy key over the covering hits, then stie = the first covering hit with it
hipError_t launch_prof_min(const HitSoA &h, int64_t n, const uint32_t *val, const int32_t *ends, const ProfTab &t, hipStream_t s);
// slots [p0, p1): the sub-batch's minima merged into the best hits (page `page`), the scratch reset
hipError_t launch_prof_merge(const HitSoA &h, const int32_t *ends, const ProfTab &t, int64_t p0, int64_t p1, int32_t page,
                             hipStream_t s);
// prb_profset_merge: slots [0, P) of src (same queries, other pages) into t: counts added, the lower best hit kept
hipError_t launch_prof_join(const ProfTab &t, const ProfTab &src, int64_t P, hipStream_t s);
// rows[j] (prb_profile_pos) of the covered slot idx[j]; hits / targets = the scanned difference arrays
hipError_t launch_prof_rows(const ProfTab &t, const uint32_t *idx, int64_t n, const int64_t *hits, const int32_t *targets, void *rows,
                            hipStream_t s);

// ============================================================================ coverage_kernels.hip: per-target coverage
// (prb_search_page_coverage, prb_covset_add_hits)
// The table of one database in HBM, a slot per character of every page's text: page after page, and within a page the
// text position itself - so every sequence is followed by its separator's slot, which takes the -1 of a span that ends
// at the sequence's last character and keeps two neighbouring sequences' regions apart (its counts stay 0).  seq_lo[t] =
// the first slot of target t (targets numbered page by page), seq_lo[ntargets] = the number of slots.  Best-hit keys:
// key = energy key of e_tot, tie = query identifier << 32 | the hit's place among that query's hits of the page; ~0 = none
// yet.  skey / stie: the (energy key, tie) minima of the list being merged, ~0 between merges.  bad: set when a hit's
// span leaves its sequence.
struct CovTab {
  const int64_t *seq_lo;           // [ntargets + 1]
  unsigned long long *hdiff;       // [P] hits: +1 at a span's first position, -1 behind its last (two's complement)
  unsigned long long *key, *tie;   // [P] the best hit so far
  unsigned long long *skey, *stie; // [P] scratch of a merge; prb_covset_finish: the scanned hits, the scanned queries and the heads
  double *e_min;                   // [P] the best hit's e_tot
  int32_t *qdiff;                  // [P] queries: the same as hdiff over the union of each (identifier, target)'s spans
  uint32_t *starts;                // [P] hits whose span begins here
  int32_t *bp;                     // [4 P] the best hit's first and last base pair (q, db, q, db)
  uint32_t *bad;
};
struct CovPage {
  int64_t slot0, target0; // the page's first slot and first target
  int32_t nseq;
};
// a list of final hits of one page, ascending by `query` (index in the call's batch): SoA columns in device memory
struct CovHits {
  int64_t n;
  const int32_t *query, *db_id;
  const double *e_tot;
  const int32_t *ends; // launch_bp_ends' four ints per hit
};
// key[i] = query << 32 | first text position of hit i's span, val[i] = i, place[i] = i's index among its query's hits
hipError_t launch_cov_keys(const CovHits &h, const CovTab &t, const CovPage &pg, uint64_t *key, uint32_t *val, uint32_t *place, hipStream_t s);
// v[i] = (key[i] with its position bits cleared) | (last position of hit val[i]'s span + 1): what the max-scan takes
hipError_t launch_cov_span(const CovHits &h, const uint64_t *key, const uint32_t *val, const CovTab &t, const CovPage &pg, uint64_t *v,
                           hipStream_t s);
// the difference arrays: every hit's span into hdiff and starts, and the part of it that no earlier hit of its query (in
// key order) covers into qdiff; m = the inclusive max-scan of launch_cov_span's v
hipError_t launch_cov_add(const CovHits &h, const uint64_t *key, const uint32_t *val, const uint64_t *m, const CovTab &t, const CovPage &pg,
                          hipStream_t s);
// four launches: the list's minima per covered slot (energy key, then (ids[query], place)), the take-over of the slots
// where that hit is below the table's best, the scratch reset
hipError_t launch_cov_min(const CovHits &h, const uint32_t *val, const uint32_t *place, const int32_t *ids, const CovTab &t, const CovPage &pg,
                          hipStream_t s);
// prb_covset_merge: slots [0, P) of src (same database) into t: counts added, the lower best hit kept
hipError_t launch_cov_join(const CovTab &t, const CovTab &src, int64_t P, hipStream_t s);
// prb_covset_finish: out[r] (prb_target_region) of the region that begins at slot first[r], a wavefront each; hits /
// queries = the scanned difference arrays, D = the depth, tbase[npages + 1] = the pages' first targets
hipError_t launch_cov_regions(const CovTab &t, const int64_t *tbase, int32_t npages, int64_t ntargets, const uint32_t *first, int64_t nregions,
                              const int64_t *hits, const int32_t *queries, int32_t D, void *out, hipStream_t s);

// ============================================================================ null_kernels.hip: the null table
// (prb_nullset_*)  The table of one batch against one database in HBM: a slot per (query q, target t), slot
// q * ntargets + t, targets numbered page by page.  A slot: the observed pair's summary record, the number of decoys
// with a hit against the target, the number of those whose e_min is not above the observed one, and the smallest decoy
// e_min as its energy key (the key of +infinity: none).  obs[slot] = the slot's `observed` as the flag the selection of
// prb_nullset_finish takes.  live[slot]: the slot still takes decoys - set when it is observed, cleared when it retires
// (launch_null_retire), which writes the number of decoys it has seen into `seen` (0: not retired).  bad: set when a
// record names a query, a sequence, an owner or a decoy outside the table.
struct NullSlot {
  uint64_t s[8];                                 // the observed pair's prb_pair_summary
  unsigned long long null_hits, null_le, null_min;
  uint32_t observed, seen;
};
static_assert(sizeof(NullSlot) == 96, "NullSlot: 64 B of record, three counters, the flag, the decoys seen");
struct NullTab {
  NullSlot *slot;    // [nslots]
  uint8_t *obs;      // [nslots]
  uint8_t *live;     // [nslots]
  uint32_t *bad;
  int64_t nslots, ntargets; // nslots = nq * ntargets
  int32_t nq, ndecoys;
};
struct NullPage {
  int64_t target0; // the page's first target
  int32_t nseq;
};
// every slot back to "not observed"
hipError_t launch_null_clear(const NullTab &t, hipStream_t s);
// rec[0, nrec) = launch_pair_fold's records (prb_pair_summary) of the real batch against the page, or a caller's: each
// into the slot of its (query, db_id), a lane per record; a (query, page) comes once
hipError_t launch_null_observe(const void *rec, int64_t nrec, const NullTab &t, const NullPage &pg, hipStream_t s);
// rec[0, nrec) = the records of a batch of ndq decoys against the page: record i is decoy decoy[query] of the real query
// owner[query]; folded into the counters of the live slots with integer atomics, a lane per record
hipError_t launch_null_count(const void *rec, int64_t nrec, const int32_t *owner, const int32_t *decoy, int32_t ndq, const NullTab &t,
                             const NullPage &pg, hipStream_t s);
// prb_nullset_retire: every live slot with null_le >= min_le retires with seen = upto, a lane per slot; live_q[nq] (zeroed
// by the caller) += the slots of each query that stay live, one atomic per wavefront and query
hipError_t launch_null_retire(const NullTab &t, unsigned long long min_le, uint32_t upto, unsigned long long *live_q, hipStream_t s);
// prb_pairmask_create_live: the rows of a decoy batch's pair mask from the live bytes.  The batch's distinct owners are
// uowner[nown]; owner u has the rows rows[rowoff[u], rowoff[u + 1]) of bits (row_words 32-bit words each).  A wavefront
// per (owner, 64 consecutive targets); *count (zeroed by the caller) += the bits set
struct LiveMaskRows {
  const int32_t *uowner, *rowoff, *rows;
  int32_t nown;
};
hipError_t launch_null_live_mask(const NullTab &t, const LiveMaskRows &r, uint32_t *bits, int64_t row_words, unsigned long long *count,
                                 hipStream_t s);
// prb_nullset_finish: out[j] (prb_null_pair) of the observed slot idx[j]; tbase[npages + 1] = the pages' first targets
hipError_t launch_null_gather(const NullTab &t, const uint32_t *idx, int64_t n, const int64_t *tbase, int32_t npages, void *out, hipStream_t s);

// ============================================================================ fdr_kernels.hip: q-values of the null table
// (prb_nullset_finish_fdr)  Per observed pair of a null table the Benjamini-Hochberg figures of include/priblast_hip.h,
// all in integers.  The n observed slots sel[0, n) ascend, so place j of sel is record j of the finish.  A pair's p-value
// is num / den = (null_le + 1) / (decoys + 1); its sort key (query << kFdrKeyBits) | ((num << 40) / den) orders the pairs
// of a query exactly as their p-values and makes equal p-values collide.  After the sort: key / place [n] in
// (query, p-value) order, off[nq + 1] the queries' segments, and per sorted entry ent = (num, den, rank, first) - rank =
// the end of its run of equal keys, first = the run's start, both counted from the segment's start - and qv = the
// triple (q_num, q_den, q_rank, 0) of the suffix minimum from the entry on.  bad (the null table's): a slot, a place, a
// query or a segment lies outside its range, or a slot holds a p-value above 1.
inline constexpr int kFdrKeyBits = 41;  // p-keys lie in [0, 2^40]
inline constexpr int kFdrChunk = 256;   // the entries of a segment that the workgroup of launch_fdr_stepup scans at a time
inline constexpr uint32_t kFdrMaxDen = 100001; // ndecoys + 1 at most: with ranks below 2^30 the cross products stay below 2^64
struct FdrTab {
  const unsigned long long *key; // [n] sorted
  const uint32_t *place;         // [n] sorted
  const int64_t *off;            // [nq + 1]
  const int64_t *tests;          // [nq]
  const uint2 *frac;             // [n] by place: (num, den)
  uint4 *ent, *qv;               // [n] sorted
  uint32_t *bad;
  int64_t n;
  int32_t nq;
};
// the key pass, a lane per place j: key[j], place[j] = j, frac[j], and cnt[query] (zeroed by the caller) += 1, one atomic
// per wavefront and query
hipError_t launch_fdr_keys(const NullTab &t, const uint32_t *sel, int64_t n, unsigned long long *key, uint32_t *place, uint2 *frac,
                           uint32_t *cnt, hipStream_t s);
// behind the sort, a lane per sorted entry: its segment from its key, the ends of its run by bisection, ent
hipError_t launch_fdr_rank(const FdrTab &f, hipStream_t s);
// the suffix minimum of tests * num / (den * rank) within every query's segment, from the highest p-value down, compared
// by cross-multiplication in 64 bits with ties to the lower rank, then the lower den; a workgroup per query walking its
// segment in chunks of kFdrChunk (chunk_suffix_min, stepup_device.hpp); a minimum above 1 is stored as (0, 0, 0)
hipError_t launch_fdr_stepup(const FdrTab &f, hipStream_t s);
// out[place] (prb_null_fdr) = the query's tests, the entry's rank and the triple at the start of its run, a lane per entry
hipError_t launch_fdr_scatter(const FdrTab &f, void *out, hipStream_t s);

// ============================================================================ group_kernels.hip: the group table
// (prb_groupset_*)  The table of one batch against one database in HBM: a slot per (query q, group g), slot
// q * ngroups + g.  A slot: the best member pair's summary record, the 128-bit key it won with - the energy key of its
// e_min, then page << 32 | db_id - and the integer sums over the members.  An empty slot has members == 0 and both keys
// all ones.  bad: set when a record or a slot names a query, a sequence, a page or a group outside the table.
struct GroupSlot {
  uint64_t s[8];                  // the best member's prb_pair_summary
  unsigned long long ekey, tie;   // the key of that record
  unsigned long long hits;        // sum of the members' hits
  uint32_t members, reserved;     // member pairs merged
};
static_assert(sizeof(GroupSlot) == 96, "GroupSlot: 64 B of record, two keys, two counters");
struct GroupTab {
  GroupSlot *slot;  // [nslots]
  uint32_t *bad;
  int64_t nslots;   // nq * ngroups
  int32_t nq, ngroups, npages;
};
struct GroupPage {
  const int32_t *group_of; // [nseq] the groups of the page's sequences
  int32_t page, nseq;
};
inline constexpr int kGroupSelect = 2048; // the entries a workgroup of launch_group_select sorts at a time
// every slot back to empty
hipError_t launch_group_clear(const GroupTab &t, hipStream_t s);
// rec[0, nrec) = launch_pair_fold's records (prb_pair_summary) of the batch against the page, or a caller's, folded into
// the slots of their (query, group of db_id), a lane per record, in three launches: the counters and the minimum energy
// key per slot (a slot whose key drops forgets its tie key), the minimum tie key among the records that hold their
// slot's energy key, and the one record that holds both keys into its slot.  A (query, page) comes once.
hipError_t launch_group_fold(const void *rec, int64_t nrec, const GroupTab &t, const GroupPage &pg, hipStream_t s);
// prb_groupset_merge: slot by slot of src (a table of the same shape) into t: counters added, the lower key's record kept
hipError_t launch_group_join(const GroupTab &t, const GroupSlot *src, hipStream_t s);
// prb_groupset_finish: occ[i] = slot i has members
hipError_t launch_group_flags(const GroupTab &t, uint8_t *occ, hipStream_t s);
// ... with n > 0: occ[0, nocc) = the occupied slots, ascending; a workgroup per query sorts its slots by key, kGroupSelect
// entries in LDS at a time, and leaves the n lowest: top[q * n + r] = the slot of rank r, keep[q * n + r] = there is one
hipError_t launch_group_select(const GroupTab &t, const uint32_t *occ, int64_t nocc, int32_t n, uint32_t *top, uint8_t *keep, hipStream_t s);
// ... out[j] (prb_group_pair) of the slot idx[j] (top == nullptr, rank 0), or of the slot top[idx[j]] with rank idx[j] % n
hipError_t launch_group_gather(const GroupTab &t, const uint32_t *idx, int64_t nrec, const uint32_t *top, int32_t n, void *out, hipStream_t s);

// ============================================================================ gnull_kernels.hip: the group null table
// (prb_gnullset_*)  The kept (query, group) records of a finished group table, and per record how the query's decoys
// fare against the group.  lookup[q * ngroups + g] = the record of (q, g), all ones: not kept.  A record's counters: the
// energy key of its e_min, the decoys with a hit in the group, those whose minimum over the group is not above e_min,
// and the smallest such minimum as its energy key (the key of +infinity: none).  cell[d * ngroups + g] = the minimum
// energy key of decoy d of the OPEN batch (owner[d], decoy[d]; ndq of them) over the members of g, all ones: no hit yet.
// bad: set when a record names a query, a sequence, a page, a group, an owner or a decoy outside the table.
struct GNullCount {
  unsigned long long ekey, null_hits, null_le, null_min;
};
struct GNullTab {
  uint32_t *lookup;         // [nq * ngroups]
  GNullCount *cnt;          // [nkept]
  unsigned long long *cell; // [ndq * ngroups] (more is allocated when an earlier batch was larger)
  const int32_t *owner, *decoy; // [ndq]
  uint32_t *bad;
  int64_t nkept;
  int32_t nq, ngroups, ndecoys, npages, ndq;
};
// prb_gnullset_create: rec[0, nkept) (prb_group_pair, on the device) copied to kept[], each into the lookup (all ones
// before), with its energy key and empty counters; a lane per record
hipError_t launch_gnull_keep(const void *rec, const GNullTab &t, void *kept, hipStream_t s);
// rec[0, nrec) = launch_pair_fold's records (prb_pair_summary) of the open decoy batch against the page, or a caller's:
// an atomic minimum of each record's energy key into the cell of (its decoy, the group of its db_id) when that group is
// kept for the decoy's owner; a lane per record
hipError_t launch_gnull_fold(const void *rec, int64_t nrec, const GNullTab &t, const GroupPage &pg, hipStream_t s);
// prb_gnullset_end: every cell of the open batch that holds a key counted into its record and emptied; a lane per cell
hipError_t launch_gnull_close(const GNullTab &t, hipStream_t s);
// prb_gnullset_finish: out[k] (prb_gnull_pair) = kept[k] with its counters
hipError_t launch_gnull_gather(const GNullTab &t, const void *kept, void *out, hipStream_t s);

// ============================================================================ eval_kernels.hip: the evalset
// (prb_evalset_*)  Two lists of (owner query, energy key) in HBM, the real batch's final hits and its decoys'.  After the
// close both are sorted by (query, key): rkey / dkey with the queries' segments roff / doff [nq + 1], and per real entry
// null_le (the decoy keys of its query that are <= its key), rank (the real ones, itself included) and the pair
// (qnum, qden) of its q-value.  bad: set when a record names a query, an owner or a decoy outside the table, an index of
// the close lies outside its list, or a looked-up key is not in its query's segment.
struct EvalTab {
  const unsigned long long *rkey, *dkey;
  const int64_t *roff, *doff;
  uint32_t *null_le, *rank, *qnum, *qden;
  uint32_t *bad;
  int64_t nreal, ndecoy;
  int32_t nq, ndecoys;
};
inline constexpr int kEvalChunk = 256; // the entries of a segment that the workgroup of launch_eval_qmin scans at a time
// energy[i] under ids[i], i < n, appended at key / own (the list's end: the host has made room), a lane per hit.  owner ==
// nullptr: ids[i] is the owner itself, in [0, nq).  Else ids[i] is a query of a batch of ndq decoys: the owner is
// owner[ids[i]], and decoy[ids[i]] lies in [0, ndecoys).
hipError_t launch_eval_append(const int32_t *ids, const double *energy, int64_t n, const int32_t *owner, const int32_t *decoy, int32_t ndq,
                              int32_t nq, int32_t ndecoys, unsigned long long *key, uint32_t *own, uint32_t *bad, hipStream_t s);
// prb_evalset_close: v[i] = i;
hipError_t launch_eval_iota(uint32_t *v, int64_t n, hipStream_t s);
// ... dst[i] = src[idx[i]] for 4-byte and for 8-byte entries (an index outside [0, n) raises bad);
hipError_t launch_eval_gather32(const uint32_t *src, const uint32_t *idx, uint32_t *dst, int64_t n, uint32_t *bad, hipStream_t s);
hipError_t launch_eval_gather64(const unsigned long long *src, const uint32_t *idx, unsigned long long *dst, int64_t n, uint32_t *bad, hipStream_t s);
// ... cnt[own[i]] += 1 (cnt zeroed by the caller): the queries' segment sizes by counting;
hipError_t launch_eval_count(const uint32_t *own, int64_t n, int32_t nq, uint32_t *cnt, uint32_t *bad, hipStream_t s);
// ... rank and null_le of every real entry, a lane each: upper bounds in its own and in its owner's decoy segment;
hipError_t launch_eval_rank(const EvalTab &t, hipStream_t s);
// ... the suffix minimum of null_le / rank within every query's segment, from the highest key down, a workgroup per query
// walking its segment in chunks of kEvalChunk with a wave-level scan and a carry between the chunks
hipError_t launch_eval_qmin(const EvalTab &t, hipStream_t s);
// prb_evalset_score: out[i] (prb_eval_score) of the real hit (query[i], energy[i]), a lane each
hipError_t launch_eval_lookup(const EvalTab &t, const int32_t *query, const double *energy, int64_t n, void *out, hipStream_t s);

// ============================================================================ feature_kernels.hip: the feature table
// (prb_featset_*)  The annotation of one page as the kernels read it: a CSR over the page's sequences - off[d] = the
// first feature of sequence d - and per feature its two ends as positions of the page's text (which holds the sequences
// reversed: tlo = start_pos + length - 1 - end, thi = start_pos + length - 1 - start) and its index in the caller's list;
// a target's features stand by (start, end, index) of their forward coordinates.  slo / slen: the sequences' first text
// position and length, what a span is checked against.
struct FeatPage {
  const int32_t *off;              // [nseq + 1]
  const int32_t *slo, *slen;       // [nseq]
  const int32_t *tlo, *thi, *idx;  // [off[nseq]]
  int32_t page, nseq;
};
// a list of final hits of one page in output order, as columns (a sub-batch's F, or a caller's list)
struct FeatHits {
  int64_t n;
  const int32_t *query, *db_id;
  const double *e_tot, *e_acc, *e_hyb;
  const int32_t *ends; // launch_bp_ends' four ints per hit
};
// What a fold works in: cnt / ioff [npairs + 1] the items per pair run and their exclusive scan, tmp [nitems] the items'
// records (prb_feature_pair; written where flag is set), flag [nitems], long_list [nitems] and nlong: the items that the
// lane form left to the wavefront form.  bad[0]: a hit or a run names a query or a sequence outside the page, or a span
// leaves its sequence (such a hit is counted nowhere); the 64-bit word at bad + 2: the unassigned hits.
struct FeatWork {
  int32_t *cnt;
  int64_t *ioff;
  void *tmp;
  uint8_t *flag;
  uint32_t *long_list, *nlong;
  uint32_t *bad;
};
inline constexpr int kFeatLongRun = 128; // a run of more hits goes to a wavefront per item
// cnt[k] = the features of the target of run k (start[k] = its first hit), cnt[npairs] = 0
hipError_t launch_feat_count(const FeatHits &h, const uint32_t *start, int64_t npairs, const FeatPage &pg, int32_t nq, const FeatWork &w,
                             hipStream_t s);
// The items (run k, feature f of its target), item x = ioff[k] + (f - off[d]): a lane per item finds its run by binary
// search in ioff and walks it in list order - count, inside, strict-`<` minimum, left-to-right sum - over the hits whose
// span meets the feature; items of runs longer than kFeatLongRun are listed for launch_feat_items_long, which gives each
// a wavefront: 64 hits tested at a time, the members' energies added one by one in list order.  Both write tmp and flag.
hipError_t launch_feat_items(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg, const FeatWork &w,
                             hipStream_t s);
hipError_t launch_feat_items_long(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg,
                                  const FeatWork &w, hipStream_t s);
// the hits whose span meets no feature of their target, added to the 64-bit word at w.bad + 2 (a lane per hit, one
// integer atomic per wavefront)
hipError_t launch_feat_unassigned(const FeatHits &h, const FeatPage &pg, int32_t nq, const FeatWork &w, hipStream_t s);
// sel[0, nsel) = the items with a hit, ascending: their records to rec[base + j] (prb_feature_pair), and per query of
// the list the place of its first record and the place behind its last: first / end [page * nq + query]
hipError_t launch_feat_append(const void *tmp, const uint32_t *sel, int64_t nsel, void *rec, int64_t base, int64_t *first, int64_t *end,
                              int32_t page, int32_t nq, hipStream_t s);
// prb_featset_merge: src's nsrc records behind dst's `base`, and the cells of src that hold records moved by `base`
hipError_t launch_feat_join(void *rec, int64_t base, int64_t *first, int64_t *end, const void *src_rec, int64_t nsrc, const int64_t *src_first,
                            const int64_t *src_end, int64_t ncells, hipStream_t s);
// prb_featset_finish: cnt[c'] for the cells in (query, page) order, c' = q * npages + p of the cell p * nq + q ...
hipError_t launch_feat_cell_counts(const int64_t *first, const int64_t *end, int32_t npages, int32_t nq, int64_t *cnt, hipStream_t s);
// ... and out[o] = the record at first[cell] + (o - off[c']) of the cell whose scanned range [off[c'], off[c' + 1]) holds o
hipError_t launch_feat_gather(const void *rec, int64_t nrec, const int64_t *first, const int64_t *off, int32_t npages, int32_t nq, int64_t total,
                              void *out, uint32_t *bad, hipStream_t s);

// ---- featuretop_kernels.hip: each query's n best records (prb_featset_finish_top, prb_fnullset_create_top) ----
// The gathered records of launch_feat_gather and their scanned cell offsets: query q's records are the segment
// [ioff[q * npages], ioff[(q + 1) * npages]) of rec[0, total); the rank key of a record is (energy_key(s.e_min), its
// place in the segment), ascending.  bad: raised where a segment, a chunk, a place or a rank lies outside the table.
struct FtopTab {
  const int64_t *ioff; // [nq * npages + 1]
  uint32_t *bad;
  int64_t total;
  int32_t nq, npages, n;
};
inline constexpr int kFtopChunk = 2048; // records per (query, chunk) work item: a power of two, at least 2 * kTopMaxN
// nchunk[q] = the chunks of query q's segment, nkeep[q] = min(n, its length); [nq] of both = 0 (for their scans)
hipError_t launch_ftop_counts(const FtopTab &t, int64_t *nchunk, int64_t *nkeep, hipStream_t s);
// choff = the scan of nchunk: a workgroup per chunk w (of the query q with choff[q] <= w < choff[q + 1]) orders the
// chunk's keys in LDS and writes its min(n, length) lowest to pe / pp [w * n + r] (energy key, place)
hipError_t launch_ftop_chunks(const FtopTab &t, const void *rec, const int64_t *choff, int64_t nchunks, unsigned long long *pe, uint32_t *pp,
                              hipStream_t s);
// a workgroup per query folds its chunks' lists: top[q * n + r] = the place of query q's record of rank r < nkeep[q]
hipError_t launch_ftop_merge(const FtopTab &t, const int64_t *choff, int64_t nchunks, const unsigned long long *pe, const uint32_t *pp,
                             uint32_t *top, hipStream_t s);
// koff = the scan of nkeep: out[o] (prb_feature_pair) = the record of rank o - koff[q] of query q, a lane per record
hipError_t launch_ftop_gather(const FtopTab &t, const void *rec, const int64_t *koff, const uint32_t *top, int64_t nkept, void *out,
                              hipStream_t s);

// ============================================================================ ranked_kernels.hip: the ranked run tables
// (prb_search_page_targets, prb_grouprank_*, prb_featrank_*)  Per list - a target (page, db_id), numbered page by page;
// a group; a feature of the annotation - n ranked keys, n payload slots and a fill count, the lists of rank_kernels.hpp.
// A key: the order-preserving image of e_min, the query's identifier, and `at` - in the table the payload slot of the
// entry (payloads never move), in a merge's run the candidate's name at its source.  The payloads: prb_target_pair,
// prb_group_pair, prb_featrank_pair.
struct alignas(16) TargetKey {
  uint64_t e;
  uint32_t id, at;
};
// the three arrays of a table's block (or of a copy of another table's): nlists lists of n slots, fill[nlists + 1]
struct RankedLists {
  TargetKey *keys;
  void *slots;
  int32_t *fill;
  int64_t nlists;
  int32_t n;
};
// The candidates of one merge, by their source.  bad: set when a candidate names a slot, a list, a query or an identifier
// outside its table; such a candidate is skipped and nothing is written for it.
// ... launch_pair_fold's records (prb_pair_summary) of a sub-batch against `page` (nseq sequences, the lists tbase ..):
// `query` (index in the batch, < nq) becomes ids[query] in place; there is nothing to refuse, and no flag
struct PairFeed {
  void *rec; // [nrec]
  int64_t nrec;
  const int32_t *ids; // [nq]
  int32_t nq, page, nseq;
  int64_t tbase;
};
// ... the occupied slots cand[0, ncand), ascending, of a batch's group table; ids[q] = the identifier of query q
struct GroupSlotFeed {
  GroupTab t;
  const uint32_t *cand; // [ncand]
  int64_t ncand;
  const int32_t *ids; // [t.nq]
  uint32_t *bad;
};
// ... the records rec[0, nrec) (prb_feature_pair) of a batch's unfinished feature table, named by their place in its
// block; ids[q] = the identifier of query q of its nq
struct FeatTableFeed {
  const void *rec; // [nrec]
  int64_t nrec;
  const int32_t *ids; // [nq]
  int32_t nq, nfeat;
  uint32_t *bad;
};
// ... a caller's records (Payload = prb_group_pair, prb_featrank_pair: their query is the identifier already, their
// group / feature lies below nlists), named by their index
template <class Payload> struct RecordFeed {
  const void *rec; // [nrec]
  int64_t nrec;
  int32_t nlists;
  uint32_t *bad;
};
// key[c] = the list of candidate c, val[c] = its name at its source: what the stable sort by list takes
template <class Feed> hipError_t launch_ranked_lists(const Feed &f, uint32_t *key, uint32_t *val, hipStream_t s);
// behind that sort (key, val sorted): rkey[i] = (the energy key of candidate val[i], its identifier, val[i]), head[i] = 1
// where key changes (and for i = 0): the first candidate of every list's run
template <class Feed>
hipError_t launch_ranked_runs(const Feed &f, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head, hipStream_t s);
// the runs [start[r], start[r + 1]) (the last one up to ncand) of rkey - run r is list list_of[start[r]] of the feed -
// merged into the table, a wavefront per run; no (identifier, list) - of the feed's page - may be in the table yet
struct RankedRuns {
  const TargetKey *rkey;
  const uint32_t *list_of, *start;
  int64_t nruns, ncand;
};
template <class Feed> hipError_t launch_ranked_merge(const Feed &f, const RankedRuns &r, const RankedLists &l, hipStream_t s);
// (the per-target table's candidates are grouped by two kernels of its own)
template <> hipError_t launch_ranked_lists(const PairFeed &f, uint32_t *key, uint32_t *val, hipStream_t s);
template <>
hipError_t launch_ranked_runs(const PairFeed &f, const uint32_t *key, const uint32_t *val, TargetKey *rkey, uint8_t *head, hipStream_t s);
// prb_*_merge: per list, the table's and src's (same shape) ranked entries merged under the table's order, the first n
// kept, in the table (src is only read); a wavefront per list
template <class Payload> hipError_t launch_ranked_join(const RankedLists &l, const RankedLists &src, hipStream_t s);
// prb_*_finish: out[0, total) = the filled slots by list, then rank (`rank` set); off = the exclusive scan of fill over
// nlists + 1 values
template <class Payload> hipError_t launch_ranked_gather(const RankedLists &l, const int64_t *off, int64_t total, void *out, hipStream_t s);

// ============================================================================ fnull_kernels.hip: the feature null table
// (prb_fnullset_*)  The kept (query, feature) records of a finished feature table, and per record how the query's decoys
// fare against the feature.  There is no dense lookup - queries x features is too many -: key[0, nkept) = the records'
// (query << 32 | feature), ascending, rec[j] = the record of key j, and qoff[q] = the first key of query q, so a (query,
// feature) is found by binary search in its query's keys.  A record's counters are the group null table's (GNullCount).
// The scratch of the OPEN batch (owner[d], decoy[d]; ndq decoys) has a cell per (decoy d, kept record of its owner):
// cell[doff[d] + (j - qoff[owner[d]])] = the minimum energy key of decoy d over the hits that meet the feature of key j,
// all ones: none yet.  bad: set when a hit, a run, a record or a cell lies outside the table, or the keys are not in order.
struct FNullTab {
  const unsigned long long *key; // [nkept]
  const uint32_t *rec;           // [nkept]
  const int64_t *qoff;           // [nq + 1]
  GNullCount *cnt;               // [nkept]
  unsigned long long *cell;      // [ncells] (more is allocated when an earlier batch was larger)
  const int32_t *owner, *decoy;  // [ndq]
  const int64_t *doff;           // [ndq + 1]; doff[ndq] = ncells
  uint32_t *bad;
  int64_t nkept, ncells, nfeat;
  int32_t nq, ndecoys, npages, ndq;
};
// prb_fnullset_create: rec[0, nkept) (prb_feature_pair, on the device) copied to kept[], each with its energy key and
// empty counters, its lookup key to key[k] and k to idx[k] (to be sorted by key); a lane per record
hipError_t launch_fnull_keep(const void *rec, const FNullTab &t, void *kept, unsigned long long *key, uint32_t *idx, hipStream_t s);
// ... and, the keys sorted: they ascend strictly, lie in their queries' ranges of qoff and name records of the table
hipError_t launch_fnull_order(const FNullTab &t, hipStream_t s);
// The items of a list of decoy hits (launch_feat_count and its scan: w.cnt, w.ioff), a lane per item: the (owner of the
// run's decoy, feature) is looked up first - not kept: the lane is done, no hit is read -, then the minimum energy key
// over the run's hits whose span meets the feature goes into the item's cell with one atomic minimum.  Items of runs
// longer than kFeatLongRun are listed (w.long_list, w.nlong) for launch_fnull_items_long: a wavefront per listed item,
// 64 hits at a time and a cross-lane minimum.
hipError_t launch_fnull_items(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg, const FeatWork &w,
                              const FNullTab &t, hipStream_t s);
hipError_t launch_fnull_items_long(const FeatHits &h, const uint32_t *start, int64_t npairs, int64_t nitems, const FeatPage &pg,
                                   const FeatWork &w, const FNullTab &t, hipStream_t s);
// prb_fnullset_end: every cell of the open batch that holds a key counted into its record and emptied; a lane per cell
hipError_t launch_fnull_close(const FNullTab &t, hipStream_t s);
// prb_fnullset_finish: out[k] (prb_fnull_pair) = kept[k] with its counters
hipError_t launch_fnull_gather(const FNullTab &t, const void *kept, void *out, hipStream_t s);

} // namespace prb
