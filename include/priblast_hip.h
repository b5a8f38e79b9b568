/* include/priblast_hip.h -- C ABI of the MI355X-native `ris` hot path (libpriblast_hip.so).
 *
 * The reference (UDC-GAC/pRIblast) has no FFI / plugin interface; its only internal seam is
 * the five private per-query stage wrappers of RnaInteractionSearch
 * (rna_interaction_search.hpp:51-79, called from rna_interaction_search.cpp:171-197):
 *
 *   CalculateAccessibility  rna_interaction_search.cpp:242-250  -> prb_qbatch_accessibility
 *   ConstructSuffixArray    rna_interaction_search.cpp:252-262  -> prb_qbatch_create (host)
 *   SearchSeed              rna_interaction_search.cpp:264-283  -> prb_search_page (stage 1)
 *   ExtendWithoutGap        rna_interaction_search.cpp:285-300  -> prb_search_page (stage 2)
 *   ExtendWithGap           rna_interaction_search.cpp:302-320  -> prb_search_page (stage 3)
 *   DbReader::LoadDatabases db_reader.cpp:29-59                 -> prb_db_open
 *   Raccess::Run(seq, idx)  raccess.cpp:34-40 (db side)         -> prb_accessibility
 *
 * The entry points below are the batched form of that seam: plain pointers and sizes,
 * opaque handles, integer status returns (0 = ok, <0 = error; prb_last_error() gives the
 * text), no exceptions and no C++/torch types across the boundary.  All device work runs
 * on the handle's own HIP stream; the library never falls back to the CPU - if no HIP
 * device can be initialised prb_ctx_create fails.
 *
 * Layouts follow the reference: accessibility arrays are `float[L]` per sequence
 * (raccess.cpp:484-528), encoded queries are `uint8_t[L+1]` (encoder.cpp:38-44), suffix
 * arrays `int32_t[L+1]`, database files are read unchanged (.bas/.seq/.acc/.nam/.ind).
 */
#ifndef PRIBLAST_HIP_H
#define PRIBLAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRB_OK 0
#define PRB_ERR_ARG (-1)
#define PRB_ERR_IO (-2)
#define PRB_ERR_HIP (-3)
#define PRB_ERR_NOMEM (-4)
#define PRB_ERR_STATE (-5)

typedef struct prb_ctx prb_ctx;       /* one GPU: stream, parameter tables, workspaces.  A context is used by one
                                       * host thread at a time; several contexts may share a device (each has its
                                       * own stream), and query batches / databases made under one of them can be
                                       * used under another one of the same device - e.g. the accessibilities of the
                                       * next batch computed under a second context while the first one searches */
typedef struct prb_db prb_db;         /* database pages resident in HBM */
typedef struct prb_qbatch prb_qbatch; /* a batch of queries: enc + SA + accessibilities */
typedef struct prb_hitset prb_hitset; /* result of prb_search_page, host side */
typedef struct prb_pairmask prb_pairmask; /* the (query, target) pairs a search is restricted to, see below */
typedef struct prb_nullset prb_nullset;   /* the null table of `ris -t -z N`, see below (prb_pairmask_create_live takes one) */

/* `ris` options, defaults of rna_interaction_search_parameters.hpp:54-62 */
typedef struct prb_ris_opts {
  int32_t max_seed_length;    /* -l 20 */
  double hybrid_threshold;    /* -e -6.0 */
  double interaction_threshold; /* -f -4.0 */
  double final_threshold;     /* -g -8.0 */
  int32_t drop_out_wo_gap;    /* -y 5  */
  int32_t drop_out_w_gap;     /* -x 16 */
  int32_t min_helix_length;   /* -m 3  */
  int32_t output_style;       /* -s 0  */
  int32_t distinct_sites;     /* -u: 0 = every final hit (the default), 1 = the distinct sites of each pair only, see below;
                               * anything else is PRB_ERR_ARG.  Ignored for last_stage 1 and 2 */
  int32_t chain_sites;        /* -j: 0 = every final hit (the default), 1 = each pair's best co-linear chain of sites only, see
                               * below; anything else, and 1 together with distinct_sites = 1, is PRB_ERR_ARG.  Ignored for
                               * last_stage 1 and 2.  (It takes what used to be the struct's tail padding.) */
  const prb_pairmask *allowed_pairs; /* -L: NULL = every pair (the default); else only the pairs the mask allows are searched,
                               * see below.  A mask made for another batch or database is PRB_ERR_ARG */
} prb_ris_opts;
#ifdef __cplusplus
static_assert(sizeof(prb_ris_opts) == 64, "prb_ris_opts: eleven fields, allowed_pairs the last one, no tail padding");
#endif

/* POD form of hit.hpp:38-118 (`Hit`) */
/* ---- distinct interaction sites (opts->distinct_sites = 1, `ris -u`) ----
 * CheckRedundancy (rna_interaction_search.cpp:387-424) removes a final hit only when another one contains it; hits that
 * merely overlap all survive, so a binding site comes out as a dozen hits shifted by a few bases.  With distinct_sites
 * the final hits of every pair are thinned by greedy non-maximum suppression on the device, between the final filter and
 * the traceback:
 *   extent     of a final hit: the rectangle [q_sp, q_sp + q_len - 1] x [db_sp, db_sp + db_len - 1] of its record,
 *              inclusive ends (the coordinates CheckRedundancy compares).  Two hits INTERSECT when their query intervals
 *              and their target intervals each share at least one position
 *   pair       the final hits of one query with one db_id of one page
 *   order      within a pair: e_tot ascending, compared as doubles (-0.0 == +0.0); equal values in output order (the
 *              hit's place in the list prb_search_page returns)
 *   selection  the pair's hits are walked in that order; a hit is kept if and only if it intersects no hit kept before
 *              it.  Dropped hits suppress nothing.  Kept hits stay in output order
 * The order is total, a pair lies within one page and a sub-batch is a range of whole queries, so the result depends
 * neither on how the batch is cut up, nor on PRB_SEARCH_PAIRS / PRB_GAPPED_CHUNK_HITS / page residency, nor on PRB_SPLIT
 * or the order of the pages.  A kept hit is, field for field and base pair for base pair (SURVEY a17 quirk included), the
 * hit that the search without the option returns; only bp_offset may differ.  Every mode takes the thinned list:
 * prb_search_page, _summary, _top, _tophits, _profile.  The stage counts keep their meaning - counts[2] = the final hits
 * after the redundancy filter, BEFORE the selection - so counts[2] minus the number of hits returned (prb_hitset_size;
 * the sum of prb_pair_summary.hits) is the number of hits the selection dropped.
 * A top-N pair table, a top-N hit table and a profile table each hold pages searched with one value of distinct_sites:
 * prb_search_page_top / _tophits / _profile refuse a second value (PRB_ERR_ARG, the table untouched), and the three
 * prb_*_merge refuse two tables of different values unless one of them has merged no page. */
/* ---- best co-linear chain of sites (opts->chain_sites = 1, `ris -j`) ----
 * Neither the plain list nor the distinct sites say which sites of a pair can bind AT THE SAME TIME: the former holds
 * copies shifted by a few bases, the latter keeps sites that cross - two duplexes in an order that no single
 * arrangement of the two strands allows.  With chain_sites the final hits of every pair are thinned, at the same point
 * as for distinct_sites, to the set of sites that increases in both coordinates and has the lowest summed energy:
 *   pair, extent, output order   as above.  db_sp is a coordinate of the page's reversed text, so both coordinates grow
 *              along a duplex
 *   precedes   hit i PRECEDES hit j when q_sp[i] + q_len[i] - 1 < q_sp[j] and db_sp[i] + db_len[i] - 1 < db_sp[j]: both
 *              gaps are strict, the two extents share no row and no column
 *   score      S(j) = P(j) + e_tot[j], in double.  P(j) = S(i*) of the chosen predecessor, or 0.0 when none is taken.
 *              i* is the hit of lowest S among the hits that precede j, doubles compared with -0.0 == +0.0, equal
 *              values going to the lowest place in the list; it is taken only if S(i*) < 0.0
 *   chain      ends at the hit of lowest S (equal values: the lowest place); its members are found by following the
 *              chosen predecessors back.  They are kept, every other hit of the pair is dropped.  Kept hits stay in
 *              output order
 * The search's list is sorted by db_sp inside a pair, so a hit's predecessors come before it and the chain's order is the
 * output order: over the kept hits, prb_pair_summary.e_sum (the left-to-right sum) is bit for bit the chain's score S,
 * and .hits its length.  Every pair keeps at least one hit; a hit with e_tot >= 0 is never chained onto and never
 * extended - it is kept only as the one hit of its pair's chain.  As for distinct_sites: a kept hit is the plain search's hit field
 * for field and base pair for base pair (only bp_offset may differ), the result depends neither on PRB_BATCH,
 * PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS, PRB_SPLIT, PRB_DEVICES nor on page residency, every mode takes the thinned
 * list, counts[2] stays the number of final hits BEFORE the selection, and each of the result tables holds pages of
 * one value of chain_sites (a second one is PRB_ERR_ARG with the field's name, the table untouched; prb_*_merge refuse
 * two tables of different values unless one has merged no page). */

/* ---- searching only listed pairs (opts->allowed_pairs, `ris -L`) ----
 * A prb_pairmask holds one bit per (query of a batch, target of a database), targets numbered page by page as
 * prb_targetset numbers them; on the device a bit matrix in HBM, its rows padded to whole 32-bit words, uploaded once - at
 * the first search that uses it - and independent of which pages are resident.  The seeds of pairs that are not allowed
 * are dropped right behind the seed expansion (one-pass form: the (query entry, database entry) pairs are compacted in
 * front of their sort; list form: a row of a disallowed pair counts no seed), so the sort, both redundancy filters, the
 * gapped stage and the traceback see the allowed pairs' hits only, and counts[0] counts their seeds only.  Nothing behind
 * the seeds mixes hits of two pairs, so the hits are, field for field, the hits of the unrestricted search for the allowed
 * pairs - with one exception: the base pairs of the FIRST hit of a query's list stay in found order, and
 * under a mask that is the first hit of the restricted list; the pairs are the same set.  With allowed_pairs = NULL
 * nothing is launched or branched on that was not before.
 *   prb_pairmask_create   no pair allowed
 *   prb_pairmask_allow    allows n pairs (query[i], page[i], db_id[i]); query[i] == -1: every query of the batch.  Only
 *                         before the first search that uses the mask (afterwards PRB_ERR_STATE); an index out of range is
 *                         PRB_ERR_ARG with the entry named, and nothing of the call is applied
 *   prb_pairmask_count    the allowed pairs (-1 for NULL)
 *   prb_pairmask_row_words   the 32-bit words of a row, (targets + 31) / 32 (-1 for NULL)
 *   prb_pairmask_words    out[0, n) = the first n words of the mask, row by row, as a search reads them - from the device
 *                         once the mask is used; bit (t & 31) of word t >> 5 of row q = the pair (q, target t).  For tests
 *   prb_pairmask_create_live   the mask of a batch dqb of ndq decoys from the LIVE pairs of a null table (prb_nullset, below):
 *                         row k holds, for every target, whether the pair (owner[k], target) of the table still takes decoys.
 *                         It is built on the device from the table's live bytes - a wavefront per 64 targets of an owner's
 *                         row, one coalesced byte per lane, the ballot stored as two 32-bit words, an owner's words written
 *                         to all of its rows; bits at or beyond the number of targets are 0 - and no bit ever exists on the
 *                         host.  The mask is born used: prb_pairmask_allow on it is PRB_ERR_STATE.  prb_pairmask_count is
 *                         the popcount of the device words, reduced on the device.  It shows the live pairs as they are at
 *                         the call: a later prb_nullset_retire does not change it.  PRB_ERR_ARG for an owner outside the
 *                         table's batch or ndq != the queries of dqb; PRB_ERR_STATE for a table that is finished or broken
 * A mask belongs to the batch and the database it was made for and must be freed before either: a search tells them by
 * their handles (and the batch's size and the database's page count), so a mask that outlives its batch may be taken
 * for the mask of a later batch of equal size at the same address.  Searches of several threads (contexts) may share a
 * mask - its first use is guarded -, prb_pairmask_allow may not run beside a search or another prb_pairmask_allow.
 * Stage timer "allow": the bit test and the compaction of the one-pass form's pairs (launches = 3 per chunk: test,
 * scan, scatter), for the chunks that are not issued ahead; and prb_pairmask_create_live's kernel (launches = 1). */
int prb_pairmask_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, prb_pairmask **out);
int prb_pairmask_allow(prb_pairmask *pm, int64_t n, const int32_t *query, const int32_t *page, const int32_t *db_id);
int64_t prb_pairmask_count(const prb_pairmask *pm);
int64_t prb_pairmask_row_words(const prb_pairmask *pm);
int prb_pairmask_words(const prb_pairmask *pm, uint32_t *out, int64_t n);
int prb_pairmask_create_live(prb_ctx *ctx, prb_nullset *ns, const prb_qbatch *dqb, const int32_t *owner, int32_t ndq,
                             prb_pairmask **out);
void prb_pairmask_free(prb_pairmask *pm);

typedef struct prb_hit {
  int32_t q_sp, db_sp;          /* start in the query / in the page's reversed db text */
  int32_t q_len, db_len;
  int32_t db_id, db_id_start;   /* sequence index in the page, forward start in it */
  double e_acc, e_hyb, e_tot;   /* kcal/mol */
  int32_t query;                /* index in the batch */
  int32_t bp_count;             /* base pairs in prb_hitset_basepairs, at bp_offset */
  int64_t bp_offset;
} prb_hit;

const char *prb_last_error(void);
const char *prb_version(void);
/* CPUs the process may keep busy (hardware threads, affinity mask, cgroup CPU quota) and the size the library gives
 * each of its pools of host threads by default (suffix arrays + seed DFS; result lines): half of that, at most 32;
 * PRB_HOST_THREADS overrides.  The reference sizes its one pool with OMP_NUM_THREADS (main.cpp / `-a`). */
int prb_cpu_budget(void);
int prb_host_threads_default(void);
void prb_ris_opts_default(prb_ris_opts *o);
/* How the one-pass seed path holds and sorts the (query SA entry, database SA entry) pairs of a chunk: the choice the
 * search makes for a page of `nchars` characters, a chunk whose queries span `query_span` (last - first) and the knobs
 * PRB_SEED_ROW_SHIFT, PRB_SEED_SORT_BITS, PRB_SEED_LOCAL_ORDER (0 / 1) and PRB_SEED_PAIR_WIDE (0 / 1), given as arguments,
 * not read from the environment.  No GPU is touched.  out[0] = 1: narrow pairs (32-bit key {query, position}, 32-bit
 * value), 0: wide ones; out[1] = bits of the key's position part, out[2] = bits of the whole key (0: row_shift < 0, no
 * pair sort), out[3] = the lowest key bit the radix sort covers, out[4] = the key bits below it that each 2048-pair tile
 * orders for itself, out[5] = 1: 64-bit keys. */
int prb_seed_pair_layout(int64_t nchars, int64_t query_span, int32_t row_shift, int32_t sort_bits, int32_t local_order,
                         int32_t pair_wide, int32_t out[6]);

/* ---- context ---- */
/* param_file: nearest-neighbour parameter data (priblast_amd/params/rna_andronescu2007.par);
 * NULL = the file next to the library. */
int prb_ctx_create(int device, const char *param_file, prb_ctx **out);
void prb_ctx_destroy(prb_ctx *ctx);
int prb_ctx_synchronize(prb_ctx *ctx);
/* device time (ms, HIP events on the library's stream) of the named stage since the last
 * reset, and launch counts: "raccess", "seed" (keys + sort of the candidates' pairs or rows - what of it is not issued
 * ahead, beside the sub-batch before), "ungapped" (one-pass form: k_seed_extend, seeds found and extended), "sort",
 * "filter", "gapped_front" (the kernel in front of the gapped cascade: the hits whose two directions find nothing;
 * "gapped_front_hits": launches = hits it completed), "gapped" (LDS tier 0; "gapped_tier0_hits": launches = hits that entered it),
 * "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow" (wavefront-per-hit kernel), "traceback", "traceback_slow",
 * "summary" (prb_search_page_summary: pair heads, segment starts and the per-pair fold; launches = 3 per sub-batch),
 * "top" (prb_search_page_top: the merge into the top-N table; launches = 1 per sub-batch; prb_topset_merge: 1),
 * "profile" (prb_search_page_profile: the merge into the per-position table, launches = 8 per sub-batch; and
 *   prb_profset_finish: the scans, the selection and the rows, launches = 3 or 4; prb_profset_merge: 1);
 * "tophits" (prb_search_page_tophits: the merge into the top-N hit table, the scan of the kept hits' pair counts and the
 *   gather of their lists; launches = 4 per sub-batch, and per prb_tophits_merge);
 * "targets" (prb_search_page_targets: the merge into the per-target table - the records' query identifiers and sort keys,
 *   the stable sort by target, the runs' keys and head flags, the selection of the heads and the merge; launches = 5 per
 *   sub-batch; prb_targetset_merge: 1);
 * "distinct" (opts->distinct_sites: the pairs' head flags, the two selection kernels and the selection of the kept hits,
 *   launches = 4 per sub-batch with final hits, and 2 more - the gathers of the records and of their pre-gapped
 *   indices - when a hit is dropped; nothing when the option is off; prb_distinct_sites: launches = 3);
 * "chain" (opts->chain_sites: the same count of launches for the chain selection - head flags, its two kernels, the
 *   selection of the kept hits, and the two gathers when a hit is dropped; prb_chain_sites: launches = 3);
 * "coverage" (prb_search_page_coverage and prb_covset_add_hits: the merge into the per-target coverage table - keys and
 *   places, the sort by (query, span start), the spans' ends, their running maximum, the difference arrays, and four
 *   launches for the best hits: minimum energy, minimum tie, take-over, scratch reset; launches = 9 per sub-batch with
 *   final hits and per prb_covset_add_hits; prb_covset_finish: the two scans, the selection of the regions' heads and the
 *   region kernel, launches = 4, or 3 when there is no region; prb_covset_merge: 1);
 * "null" (prb_search_page_observed / _decoys, prb_nullset_observe / _add_pairs: the scatter or the fold into the null
 *   table, launches = 1 per sub-batch with final hits; prb_nullset_finish: the selection and the gather, launches = 2);
 * "fdr" (prb_nullset_finish_fdr: the key pass, launches = 1, then the sort, the rank pass, the step-up pass and the scatter,
 *   launches = 4; nothing without observed pairs);
 * "group" (prb_search_page_groups / prb_groupset_add_pairs: the fold into the group table, launches = 3 per sub-batch with
 *   final hits; prb_groupset_merge: 1; prb_groupset_finish: the flags, the selections and the gather, launches = 2 to 5);
 * "grouprank" (prb_grouprank_add_groupset: the group table's occupied slots merged into the group ranking table - flags,
 *   compaction, sort keys, the stable sort by group, rank keys and heads, the selection of the heads, the merge; launches = 7,
 *   or 2 when the group table is empty; prb_grouprank_add_records: 5; prb_grouprank_merge: 1);
 * "gnull" (prb_gnullset_create: the kept records into the lookup, launches = 1; prb_search_page_gnull / prb_gnullset_add_pairs:
 *   the fold into the scratch, launches = 1 per sub-batch with final hits; prb_gnullset_end: the close, 1; prb_gnullset_finish:
 *   the gather, 1);
 * "eval" (prb_search_page_scored / _null_hits, prb_evalset_add_keys: the append of the keys, launches = 1 per sub-batch with
 *   final hits; prb_evalset_close: per list the sorts and gathers and the count, then the ranks and the suffix minima;
 *   prb_evalset_score: the look-up, 1);
 * "feature" (prb_search_page_features / prb_featset_add_hits: the fold into the feature table - the items per pair, their
 *   scan, the item kernel, its long-run form, the unassigned count, the selection of the items with a hit and the append;
 *   launches = 7 per sub-batch with final hits, or 3 - the counts, their scan and the unassigned count - when its targets
 *   have no feature, and 2 more - head flags and the selection of the runs' first hits - in front per prb_featset_add_hits
 *   with hits; prb_featset_merge: 1; prb_featset_finish: the cells' record counts, their scan and the gather, launches = 3,
 *   or none for a table without records; prb_featset_finish_top / prb_fnullset_create_top: those 3 and the ranked cut - the
 *   queries' chunk and kept counts, their two scans, the chunks' lists, the queries' folds and the gather of the kept
 *   records -, launches = 9, or none for a table without records);
 * "fnull" (prb_fnullset_create: the kept records with their lookup keys, the sort of the keys and the check of their order,
 *   launches = 3, or none without records; prb_search_page_fnull / prb_fnullset_add_hits: the fold into the scratch - the
 *   items per pair, their scan, the item kernel and its long-run form; launches = 4 per sub-batch with final hits, or 2 -
 *   the counts and their scan - when its targets have no feature, and 2 more - head flags and the selection of the runs'
 *   first hits - in front per prb_fnullset_add_hits with hits; prb_fnullset_end: the close, 1, or none for a batch without
 *   cells; prb_fnullset_finish: the gather, 1, or none without records);
 * "featrank" (prb_featrank_add_featset: the records of the feature table merged into the feature ranking table - sort
 *   keys, the stable sort by feature, rank keys and heads, the selection of the heads, the merge; launches = 5, or none when
 *   the feature table holds no record; prb_featrank_add_records: 5, or none for n = 0; prb_featrank_merge: 1);
 * host wall-clock pseudo stages: "host_dfs" (background seed DFS), "host_dfs_wait",
 * "host_search_range", "host_cands", "host_drain_tail", "host_download" (the synchronous copy of
 * the hits of last_stage 1 / 2). */
int prb_ctx_stage_ms(prb_ctx *ctx, const char *stage, double *ms, int64_t *launches);
void prb_ctx_reset_timers(prb_ctx *ctx);

/* ---- stage 1: accessibility (Raccess), batched over sequences ----
 * seqs: concatenated characters, sequence i = seqs[offsets[i] .. offsets[i+1]);
 * acc/cond: concatenated float outputs with the same offsets (L floats per sequence,
 * entries the reference leaves untouched are 0), host memory. */
int prb_accessibility(prb_ctx *ctx, int32_t nseq, const char *seqs, const int64_t *offsets,
                      int32_t maximal_span, int32_t min_accessible_length, float *acc, float *cond);

/* diagnostics: runs Raccess for ONE sequence and returns the DP tables in the reference's
 * own layout (raccess.hpp:89-103): alpha_outer/beta_outer hold L+1 doubles; tables[0..5] =
 * Alpha_{stem,stemend,multi,multibif,multi1,multi2}, tables[6..11] = Beta_ same order, each
 * (L+1)*(W+2) doubles, row-major [i][j-i]; NULL entries are skipped. */
int prb_accessibility_tables(prb_ctx *ctx, const char *seq, int32_t len, int32_t maximal_span,
                             int32_t min_accessible_length, float *acc, float *cond,
                             double *alpha_outer, double *beta_outer, double *const tables[12]);

/* ---- host helpers that are part of the seam (stage 2: encode + suffix array) ---- */
int prb_encode_query(const char *seq, int32_t len, int32_t repeat_flag, uint8_t *enc /* len+1 */);
int prb_suffix_array(const uint8_t *text, int32_t n, int32_t *sa);
/* A decoy of a query, for an empirical null of its interaction energies (no GPU): decoy `decoy` of the sequence
 * seq[0, len) that stands at place file_pos of its input file.  An Altschul-Erikson shuffle over the bytes as read - a
 * lower-case, soft-masked letter is a symbol of its own - that keeps the first byte, the last byte and the count of every
 * pair of adjacent bytes; out[0, len) (no NUL is added; `out` must not overlap `seq`).  len < 3 copies the input.
 *   successors   per symbol, the bytes that follow its occurrences, in order of occurrence
 *   last edges   for each symbol that occurs among seq[0, len - 1), other than seq[len - 1], in ascending byte value: one
 *                entry of its list, drawn uniformly; all are drawn again until every such symbol reaches seq[len - 1]
 *                through last edges
 *   lists        per symbol: the LAST occurrence of the chosen edge is taken out, the rest shuffled (Fisher-Yates: for
 *                i = k - 1 down to 1, j = draw(i + 1), swap i and j), the chosen edge put at the end; the symbol of
 *                seq[len - 1] shuffles its whole list; symbols in ascending byte value
 *   walk         from seq[0], every symbol's list consumed front to back
 * Draws: splitmix64 (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), draw(k) = next() % k.  The state starts at
 * mix(mix(mix(seed) ^ (uint64_t)file_pos) ^ (uint64_t)decoy), mix(x) = the splitmix64 output for state x (the increment
 * included): a decoy depends on the seed, its query and the query's place in its file only - not on how the queries are
 * cut into batches.  tests/shuffle_ref.py restates all of it.  PRB_ERR_ARG: a NULL pointer with len > 0; len, file_pos
 * or decoy below 0. */
int prb_shuffle_sequence(const char *seq, int32_t len, uint64_t seed, int64_t file_pos, int32_t decoy, char *out);

/* ---- database ---- */
int prb_db_open(prb_ctx *ctx, const char *prefix, prb_db **out);
/* The same with at most max_resident_pages of the database's pages in HBM at a time (0 = all, what
 * prb_db_open does unless PRB_DB_RESIDENT_PAGES says otherwise): prb_search_page uploads the page it is
 * asked for if it is not resident (the least recently used page makes room) and, with two pages or
 * more, uploads the next page on a copy stream of its own while this one is searched.  For databases
 * beyond HBM; results do not depend on it.  prb_db_page_uploads: pages uploaded so far. */
int prb_db_open_streaming(prb_ctx *ctx, const char *prefix, int32_t max_resident_pages, prb_db **out);
int64_t prb_db_page_uploads(const prb_db *db);
void prb_db_close(prb_db *db);
int prb_db_info(const prb_db *db, int32_t *hash_size, int32_t *repeat_flag, int32_t *maximal_span,
                int32_t *min_accessible_length, int32_t *npages);
int prb_db_page_info(const prb_db *db, int32_t page, int32_t *nseq, int64_t *nchars);
/* name / reference-style lengths of sequence `id` of `page` (db_reader.cpp:107-131) */
const char *prb_db_seq_name(const prb_db *db, int32_t page, int32_t id);
int prb_db_seq_lengths(const prb_db *db, int32_t page, int32_t id, int32_t *length,
                       int32_t *length_unmasked, int32_t *start_pos);
/* build a database from sequences (same files the reference's `db` step writes;
 * db_construction.cpp:37-83): accessibilities on the GPU, SA + k-mer table on the host. */
int prb_db_build(prb_ctx *ctx, const char *prefix, int32_t nseq, const char *const *names,
                 const char *seqs, const int64_t *offsets, int32_t repeat_flag, int32_t hash_size,
                 int32_t maximal_span, int32_t min_accessible_length, int32_t page_size);

/* ---- query batches ---- */
int prb_qbatch_create(prb_ctx *ctx, int32_t nq, const char *seqs, const int64_t *offsets,
                      int32_t repeat_flag, prb_qbatch **out);
void prb_qbatch_destroy(prb_qbatch *qb);
/* runs Raccess for every query of the batch; results stay in HBM for the search stages */
int prb_qbatch_accessibility(prb_ctx *ctx, prb_qbatch *qb, int32_t maximal_span,
                             int32_t min_accessible_length);
/* copies of the per-query arrays (NULL pointers are skipped) */
int prb_qbatch_get(prb_qbatch *qb, int32_t q, uint8_t *enc, int32_t *sa, float *acc, float *cond);
int32_t prb_qbatch_length_unmasked(const prb_qbatch *qb, int32_t q);
/* Optional: starts the seed search proper (the suffix-array DFS of SeedSearch::Run, seed_search.cpp:153-295; host
 * threads) of the batch against `page` in the background and returns at once.  A later prb_search_page with the
 * same database, page, -l and -e picks it up instead of starting its own - e.g. begun for the NEXT batch while
 * this one is searched.  It needs neither the accessibilities nor the GPU. */
int prb_qbatch_seed_search_begin(prb_ctx *ctx, prb_qbatch *qb, const prb_db *db, int32_t page, const prb_ris_opts *opts);

/* ---- stages 3-5: seed search, ungapped and gapped extension for all queries of a batch
 * against one page.  last_stage: 1 = seeds, 2 = after ungapped extension + filter,
 * 3 = final (after gapped extension + filter). ---- */
int prb_search_page(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                    int32_t last_stage, prb_hitset **out);
int64_t prb_hitset_size(const prb_hitset *hs);
const prb_hit *prb_hitset_hits(const prb_hitset *hs);
/* pairs (q, db) as int32[2], indexed by prb_hit.bp_offset.  With opts->output_style == 0
 * (simplified output, which prints only the two ends of an interaction,
 * rna_interaction_search.cpp:355-363) final hits carry exactly two pairs, the first and the
 * last of the reference's list; with output_style == 1 they carry every pair. */
const int32_t *prb_hitset_basepairs(const prb_hitset *hs, int64_t *count);
/* number of hits per stage for the whole call: seeds, after ungapped+filter, final */
void prb_hitset_counts(const prb_hitset *hs, int64_t counts[3]);
void prb_hitset_free(prb_hitset *hs);

/* The selection of opts->distinct_sites for a caller's own list of final hits in host memory (hit sets gathered from
 * several ranks, the records of a `ris -b` file ...), by the same kernels: keep[i] = 1 for the hits kept, else 0.  A pair
 * is a maximal run of consecutive records with equal (query, db_id); the order inside a run is e_tot, then the index.
 * The runs need not be sorted by db_sp.  n <= 2^31 - 1; n = 0 does nothing. */
int prb_distinct_sites(prb_ctx *ctx, const prb_hit *hits, int64_t n, uint8_t *keep);
/* The selection of opts->chain_sites for a caller's own list, likewise: keep[i] = 1 for the members of their pair's best
 * chain, else 0.  A pair is a maximal run of consecutive records with equal (query, db_id).  Inside a run db_sp must not
 * decrease (the search's order: a hit's predecessors then come before it); a record that breaks this is PRB_ERR_ARG
 * with its index in the message, and nothing is computed.  n <= 2^31 - 1; n = 0 does nothing. */
int prb_chain_sites(prb_ctx *ctx, const prb_hit *hits, int64_t n, uint8_t *keep);

/* Diagnostics: a caller's list of hit records, in any order, through the sort and the redundancy filter that every
 * search runs behind its ungapped and its gapped stage (the same code, with the PRB_SORT_* / PRB_FILTER_TILES switches
 * of the environment).  sorted[n]: the records in the stages' order (query, db_sp, q_sp, db_len and q_len descending,
 * e_tot, e_hyb, e_acc, place in the input), bp_count and bp_offset zero; keep[n]: 1 for the hits at those sorted places
 * that the filter leaves with `threshold`; *form: the form of the sort that gave the order.  The bounds of the one-key
 * sort come from the list itself (the one-length key: every hit has q_len == db_len).  query, q_sp and db_sp must not be
 * negative, q_sp + q_len and db_sp + db_len at most 2^31 - 1 (lengths count modulo 2^16, as in the search);
 * n <= 2^31 - 1; n = 0 does nothing. */
enum {
  PRB_SORT_PACKED_TWO_LENGTHS = 0, /* one packed key with both lengths */
  PRB_SORT_PACKED_ONE_LENGTH = 1,  /* one packed key with the length once */
  PRB_SORT_GENERAL_WIDTH = 2,      /* the sort field by field: the packed key needs more than 64 bits */
  PRB_SORT_GENERAL_TIE_RUN = 3,    /* ... : more hits with identical coordinates than the tie pass takes */
  PRB_SORT_GENERAL_FORCED = 4      /* ... : PRB_SORT_FOUR_KEYS is set */
};
int prb_sort_filter(prb_ctx *ctx, const prb_hit *hits, int64_t n, double threshold, prb_hit *sorted, uint8_t *keep,
                    int32_t *form);

/* ---- per-pair summaries (`ris -t`): the final hits reduced on the device, one record per (query, database
 * sequence) pair that has at least one final hit.  The hits are exactly those prb_search_page(..., 3, ...) returns
 * with the same options (any output_style); their order there is the "output order" below.
 *   hits      number of final hits of the pair
 *   e_min     smallest e_tot; the best hit is the FIRST hit in output order with that e_tot
 *   e_sum     sum of e_tot over the pair's hits, added left to right in output order, from 0.0
 *   e_acc / e_hyb, bp_first / bp_last   the best hit's energies and its first and last base pair, as
 *             prb_hitset_basepairs gives them with output_style 0 (the simplified form, SURVEY a17 quirk included)
 * Records come query by query (ascending), and within a query in the order of the pairs' first hits.  The hit
 * records and base pairs never leave the device.  Argument checks and option limits are those of prb_search_page;
 * the device time of the reduction is the stage "summary" of prb_ctx_stage_ms. */
typedef struct prb_pair_summary {
  int32_t query, db_id;            /* index in the batch, sequence index in the page */
  int64_t hits;
  double e_min, e_sum, e_acc, e_hyb;
  int32_t bp_first[2], bp_last[2]; /* (q, db) pairs; db in the page's reversed text, as in prb_hitset_basepairs */
} prb_pair_summary;
typedef struct prb_pairset prb_pairset;
int prb_search_page_summary(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                            prb_pairset **out);
int64_t prb_pairset_size(const prb_pairset *ps);
const prb_pair_summary *prb_pairset_pairs(const prb_pairset *ps);
/* the same stage counts as prb_hitset_counts: seeds, after ungapped+filter, final hits */
void prb_pairset_counts(const prb_pairset *ps, int64_t counts[3]);
void prb_pairset_free(prb_pairset *ps);

/* ---- the N best pairs per query (`ris -t -n N`): a top-N table on the device ----
 * A table holds, for each query of one batch, the N pairs with the lowest e_min among the per-pair summaries of the
 * pages merged into it (fewer when the query has fewer pairs).  Pairs of a query are ranked by e_min ascending,
 * compared as doubles (-0.0 == +0.0); equal values are ordered by the `-t` output order: page ascending, then the
 * pair's position among that query's records of that page (prb_pairset_pairs order).  It is a total order, so the
 * table does not depend on the order the pages are merged in, nor on how the batch is cut up.
 *   prb_topset_create   an empty table for qb (1 <= n <= 1024; nq * n slots of about 72 B in HBM)
 *   prb_search_page_top the search of prb_search_page_summary against `page`, its records merged into the table on
 *                       the device (nothing is copied to the host).  Argument checks and option limits are those of
 *                       prb_search_page_summary; the table must have been made with this context and this batch, and
 *                       holds pages of one database, each merged once.  A call refused by these checks leaves the
 *                       table as it was; a merge that fails part way leaves it unusable.
 *   prb_topset_finish   copies the table to the host (one copy) and releases its device memory: prb_topset_pairs
 *                       then returns the records by query ascending, then by rank; `rank` counts from 0 within the
 *                       query.  No page can be merged after it (a second call does nothing)
 *   prb_topset_counts   the stage counts of prb_pairset_counts, summed over the merged pages
 *   prb_topset_merge    two unfinished tables into one, on the device: dst (of ctx) then holds exactly - bit for bit -
 *                       the table that the union of the two page sets merged into one table gives, its counts are the
 *                       sums and its page set is the union; src is left empty but valid (it can be freed, or finished to
 *                       zero records).  src may belong to another context, on the same or on another device: its records
 *                       are then copied to dst's device first (a peer copy where hipDeviceCanAccessPeer allows it, else
 *                       through pinned host memory), and the caller's current device is restored.  Both tables were made
 *                       with the same n for batches of the same number of queries of the same lengths, and no page is
 *                       merged into both: anything else returns PRB_ERR_ARG and leaves both tables as they were.  This is
 *                       what lets several contexts share the pages of ONE batch (`ris` with PRB_SPLIT).  A dst that had
 *                       merged no page takes over src's database: pages of no other one can be searched into it.
 * The device time of the merges is the stage "top" of prb_ctx_stage_ms (prb_topset_merge: launches = 1). */
typedef struct prb_top_pair {
  prb_pair_summary s;
  int32_t page, rank; /* the page the pair was found in; its rank within its query */
} prb_top_pair;
typedef struct prb_topset prb_topset;
int prb_topset_create(prb_ctx *ctx, const prb_qbatch *qb, int32_t n, prb_topset **out);
int prb_search_page_top(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                        prb_topset *ts);
int prb_topset_merge(prb_ctx *ctx, prb_topset *dst, prb_topset *src);
int prb_topset_finish(prb_ctx *ctx, prb_topset *ts);
int64_t prb_topset_size(const prb_topset *ts);
const prb_top_pair *prb_topset_pairs(const prb_topset *ts);
void prb_topset_counts(const prb_topset *ts, int64_t counts[3]);
void prb_topset_free(prb_topset *ts);

/* ---- the N best interaction sites per query (`ris -k N`): a top-N table of hits, with their base pairs, on the device ----
 * A table holds, for each query of one batch, the N final hits of lowest e_tot among the hits of the pages merged into
 * it (fewer when the query has fewer hits).  The final hits are exactly those of prb_search_page(..., 3, ...) with the
 * same options.  Hits of a query are ranked by e_tot ascending, compared as doubles (-0.0 == +0.0); equal values are
 * ordered by the output order: page ascending, then the hit's place among that query's hits of that page as
 * prb_search_page returns them.  It is a total order, so the table does not depend on the order the pages are merged
 * in, on how the batch is cut up, on the chunks of the gapped stage, nor on page residency.
 *   prb_tophits_create       an empty table for qb (1 <= n <= 1024; nq * n slots of 72 B in HBM, and a pool of the kept
 *                            hits' base pairs that is sized by what is kept)
 *   prb_search_page_tophits  the search of prb_search_page against `page`, its final hits merged into the table on the
 *                            device, the base-pair lists of the kept ones gathered into the table's pool (nothing is
 *                            copied to the host).  Argument checks and option limits are those of prb_search_page; the
 *                            table must have been made with this context and this batch, and holds pages of one
 *                            database, each merged once, all with the same opts->output_style.  A call refused by these
 *                            checks leaves the table as it was; a merge that fails part way (PRB_ERR_NOMEM when the pool
 *                            cannot be allocated) leaves it unusable.
 *   prb_tophits_finish       copies the records and the pairs to the host (one copy each) and releases the device
 *                            memory: prb_tophits_hits then returns the records by query ascending, then by rank; `rank`
 *                            counts from 0 within the query.  No page can be merged after it (a second call does nothing)
 *   prb_tophits_hits         `h` equals, field for field, the record prb_search_page returns for that hit with the same
 *                            output_style - but for bp_offset, which indexes prb_tophits_basepairs: the kept hits' lists
 *                            in record order, without gaps, each equal to the hit's pairs in prb_hitset_basepairs (with
 *                            output_style 0 the two end pairs, SURVEY a17 quirk included; otherwise every pair)
 *   prb_tophits_counts       the stage counts of prb_hitset_counts, summed over the merged pages
 *   prb_tophits_merge        prb_topset_merge for two unfinished top-N hit tables, same contract; the kept hits' base-pair
 *                            lists are gathered from the two pools into a pool of exactly their size (the scan and the
 *                            gather of prb_search_page_tophits).  The two tables hold pages searched with the same
 *                            output_style, unless one of them has merged no page yet (else PRB_ERR_ARG, both untouched)
 * The device time of the merges (selection, scan, gather) is the stage "tophits" of prb_ctx_stage_ms (prb_tophits_merge:
 * launches = 4). */
typedef struct prb_top_hit {
  prb_hit h;
  int32_t page, rank; /* the page the hit was found in; its rank within its query */
} prb_top_hit;
typedef struct prb_tophits prb_tophits;
int prb_tophits_create(prb_ctx *ctx, const prb_qbatch *qb, int32_t n, prb_tophits **out);
int prb_search_page_tophits(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                            prb_tophits *th);
int prb_tophits_merge(prb_ctx *ctx, prb_tophits *dst, prb_tophits *src);
int prb_tophits_finish(prb_ctx *ctx, prb_tophits *th);
int64_t prb_tophits_size(const prb_tophits *th);
const prb_top_hit *prb_tophits_hits(const prb_tophits *th);
const int32_t *prb_tophits_basepairs(const prb_tophits *th, int64_t *npairs);
void prb_tophits_counts(const prb_tophits *th, int64_t counts[3]);
void prb_tophits_free(prb_tophits *th);

/* ---- per-position interaction profile (`ris -q`): a table of every query position on the device ----
 * For each query of one batch and each of its positions covered by at least one final hit (the hits of
 * prb_search_page(..., 3, ...) with the same options) of the pages merged in.  The span of a hit is the query positions
 * q0..qN (inclusive, 0-based) of its first and last base pair in the `-s 0` form (prb_pair_summary's bp_first /
 * bp_last); the reference sorts a hit's pairs, so q0 <= qN (the few unsorted ones, SURVEY a17, count as
 * min(q0, qN)..max(q0, qN)).  Per covered position:
 *   hits      the number of final hits whose span contains it
 *   targets   the number of distinct database sequences (page, db_id) with such a hit: two hits of one pair count once
 *   e_min     the smallest e_tot of those hits, compared as doubles (-0.0 == +0.0)
 *   page, db_id, bp_first / bp_last   the best hit: the FIRST hit with e_min in output order (page ascending, then its
 *             place in the page's result lines); its pairs as in prb_pair_summary
 * Every column is a count or a minimum over a total order, so the table does not depend on the order the pages are
 * merged in nor on how the batch is cut up.
 *   prb_profset_create       an empty table for qb: one slot per query position plus one per query, about 68 B each in
 *                            HBM (PRB_ERR_NOMEM when that cannot be allocated)
 *   prb_search_page_profile  the search of prb_search_page_summary against `page`, its final hits merged into the table
 *                            on the device.  Argument checks and option limits are those of prb_search_page_summary; the
 *                            table must have been made with this context and this batch, and holds pages of one
 *                            database, each merged once.  A call refused by these checks leaves the table as it was; a
 *                            merge that fails part way leaves it unusable.
 *   prb_profset_finish       the covered positions selected on the device and copied to the host (one copy); the device
 *                            table is released.  prb_profset_rows then returns them by query ascending, then by
 *                            position.  No page can be merged after it (a second call does nothing)
 *   prb_profset_counts       the stage counts of prb_pairset_counts, summed over the merged pages
 *   prb_profset_merge        prb_topset_merge for two unfinished profile tables, same contract (there is no n): per slot
 *                            the hits add, the targets add - no page is in both tables, so no (page, db_id) is counted
 *                            twice -, and the best hit is the one of lower e_min, equal values decided by (page, place)
 * The device time of the merges and of the finish is the stage "profile" of prb_ctx_stage_ms (prb_profset_merge:
 * launches = 1). */
typedef struct prb_profile_pos {
  int32_t query, pos;          /* index in the batch; 0-based position in the query (masked bases included) */
  int64_t hits;
  int32_t targets, page, db_id; /* page and sequence index in the page of the best hit */
  int32_t reserved;            /* 0 */
  double e_min;
  int32_t bp_first[2], bp_last[2]; /* the best hit's (q, db) end pairs; db in the page's reversed text */
} prb_profile_pos;
typedef struct prb_profset prb_profset;
int prb_profset_create(prb_ctx *ctx, const prb_qbatch *qb, prb_profset **out);
int prb_search_page_profile(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                            prb_profset *ps);
int prb_profset_merge(prb_ctx *ctx, prb_profset *dst, prb_profset *src);
int prb_profset_finish(prb_ctx *ctx, prb_profset *ps);
int64_t prb_profset_size(const prb_profset *ps);
const prb_profile_pos *prb_profset_rows(const prb_profset *ps);
void prb_profset_counts(const prb_profset *ps, int64_t counts[3]);
void prb_profset_free(prb_profset *ps);

/* ---- the N best queries per target (`ris -r N`): a top-N table per database sequence on the device ----
 * A target is a (page, db_id) of one database.  A table holds, for every target, the N pairs with the lowest e_min among
 * the per-pair summaries (exactly the records prb_search_page_summary returns) of all the calls merged into it, over
 * all their queries (fewer when the target has fewer pairs).  It lives as long as the caller likes - a whole run -, not
 * one batch: every call names its queries by caller-given identifiers, int32 >= 0, one per query of the batch (the
 * command line: the 0-based position in the input FASTA), and `s.query` of a record holds that identifier.  Pairs of a
 * target are ranked by e_min ascending, compared as doubles (-0.0 == +0.0); equal values are ordered by the query's
 * identifier ascending.  A (query id, page, db_id) triple occurs at most once - a (query id, page) is merged once -, so
 * it is a total order, and the table depends - bit for bit - neither on how the queries are cut into batches or
 * sub-batches, nor on the order of the batches or of the pages, nor on which context (worker) took what, nor on page
 * residency.
 *   prb_targetset_create     an empty table for db (1 <= n <= 1024): n slots of 72 B and n keys of 16 B per sequence of
 *                            every page of db, plus a fill count per target, in HBM; PRB_ERR_NOMEM when that cannot be
 *                            allocated
 *   prb_search_page_targets  the search of prb_search_page_summary of qb against `page`, its records merged into the
 *                            table on the device (nothing is copied to the host); query_ids[q] = the identifier of query q
 *                            of qb (qb's number of queries).  Argument checks and option limits are those of
 *                            prb_search_page_summary.  PRB_ERR_ARG, the table untouched: a table made with another
 *                            context or for another database; an identifier below 0, given twice in the call, or already
 *                            merged for this page; opts->distinct_sites other than that of the pages merged so far.  A
 *                            merge that fails part way leaves the table unusable.
 *   prb_targetset_merge      two unfinished tables into one, on the device: dst (of ctx) then holds exactly - bit for bit
 *                            - the table that all that was merged into either, merged into one table, gives; its counts
 *                            are the sums; src is left empty but valid (it can be freed, or finished to zero records).
 *                            src may belong to another context, on the same or on another device: its table is then
 *                            copied to dst's device first (a peer copy where hipDeviceCanAccessPeer allows it, else through
 *                            pinned host memory), and the caller's current device is restored.  Both were made with the
 *                            same n for the same database - the handles may differ (every context opens its own): the
 *                            same pages of the same numbers of sequences -, hold the same distinct_sites unless one is
 *                            empty, and no (query id, page) is merged into both: anything else returns PRB_ERR_ARG and
 *                            leaves both tables as they were.
 *   prb_targetset_finish     the filled slots compacted on the device (a scan over the fills, a gather in rank order)
 *                            and copied to the host in one copy; the device memory is released.  prb_targetset_pairs then
 *                            returns the records by page, then db_id, then rank; `rank` counts from 0 within the target.
 *                            Nothing can be merged after it (a second call does nothing)
 *   prb_targetset_counts     the stage counts of prb_pairset_counts, summed over the merged calls
 * The device time of the merges is the stage "targets" of prb_ctx_stage_ms (launches = 5 per sub-batch: identifiers and
 * sort keys, the stable sort by target, the runs' keys and heads, the selection of the heads, the merge;
 * prb_targetset_merge: 1). */
typedef struct prb_target_pair {
  prb_pair_summary s; /* s.query = the query's identifier */
  int32_t page, rank; /* the target's page; the pair's rank within its target */
} prb_target_pair;
typedef struct prb_targetset prb_targetset;
int prb_targetset_create(prb_ctx *ctx, prb_db *db, int32_t n, prb_targetset **out);
int prb_search_page_targets(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                            const int32_t *query_ids, prb_targetset *ts);
int prb_targetset_merge(prb_ctx *ctx, prb_targetset *dst, prb_targetset *src);
int prb_targetset_finish(prb_ctx *ctx, prb_targetset *ts);
int64_t prb_targetset_size(const prb_targetset *ts);
const prb_target_pair *prb_targetset_pairs(const prb_targetset *ts);
void prb_targetset_counts(const prb_targetset *ts, int64_t counts[3]);
void prb_targetset_free(prb_targetset *ts);

/* ---- the regions of each target bound by at least D queries (`ris -c D`): a per-position table of the database on the
 * device ----
 * A target is a (page, db_id) of one database.  The span of a final hit (the hits of prb_search_page(..., 3, ...) with the
 * same options; with distinct_sites the kept ones) on its target is [min(db0, dbN), max(db0, dbN)]: db0 and dbN are the
 * database coordinates of its first and last base pair in the `-s 0` form (prb_pair_summary's bp_first[1] / bp_last[1]),
 * positions in the page's text, which holds the sequences reversed.  A span that leaves its sequence [start_pos,
 * start_pos + length) raises the table's `bad` flag, is counted nowhere, and fails the call that sees it with
 * PRB_ERR_STATE: prb_covset_add_hits, which checks its list first and leaves the table untouched, or prb_covset_finish
 * (never for a consistent search).  Per position of a target, over everything merged into the table:
 *   hits      the number of final hits whose span contains it
 *   starts    the number of final hits whose span begins at it: at min(db0, dbN), a position of the page's text
 *   queries   the number of distinct query identifiers with such a hit: the union of each (query id, target)'s spans, two
 *             hits of one query count once
 *   e_min     the smallest e_tot of those hits, compared as doubles (-0.0 == +0.0), and the best hit: among the hits with
 *             e_min the one of the lowest (query id, place).  `place` is the hit's index among that query's hits against
 *             that page in output order (the list prb_search_page returns), not its index in a sub-batch's list
 * Query identifiers are the caller's, int32 >= 0, as in prb_search_page_targets; a (query id, page) is merged at most
 * once.  Every column is a sum, a maximum, a minimum or a lexicographic minimum of integers over a total order, so the
 * table depends - bit for bit - neither on how the queries are cut into batches or sub-batches, nor on the order of the
 * batches or of the pages, nor on which context (worker) took what, nor on page residency.
 * A REGION at depth D is a maximal run of consecutive positions of ONE sequence with queries >= D: two neighbouring
 * sequences that are both covered from end to end are two regions.  Its record:
 *   page, db_id   the target
 *   start, end    inclusive, start <= end, in the sequence's FORWARD coordinates - the numbers that the base-pair field of
 *                 a result line prints: length - 1 - (text position - start_pos)
 *   hits          the sum of `starts` over the region: for D = 1 every hit that touches it
 *   max_hits, max_queries   the maxima of the two per-position columns over the region
 *   peak          the lowest forward position with queries == max_queries
 *   e_min, query, bp_first / bp_last   the best hit over the region - the lowest (e_min, query id, place) of its positions
 *                 -: its e_tot, its query's identifier and its end pairs as in prb_pair_summary
 *   reserved      0 (the record has no uninitialised byte)
 * Records come by page, then db_id, then start.
 *   prb_covset_create         an empty table for db: a slot per character of every page's text, which holds a separator
 *                             behind every sequence - one slot per base plus one per sequence -, 72 B each in HBM (64 B
 *                             of columns and 8 B of scratch; 1e8 characters: 7.2 GB), plus 8 B per sequence.  PRB_ERR_NOMEM
 *                             when that cannot be allocated; PRB_ERR_ARG for a database of 2^32 slots or more
 *   prb_search_page_coverage  the search of prb_search_page_summary of qb against `page`, its final hits merged into the
 *                             table on the device (nothing is copied to the host); query_ids[q] = the identifier of query
 *                             q of qb.  Argument checks and option limits are those of prb_search_page_summary, the
 *                             refusals those of prb_search_page_targets (PRB_ERR_ARG, the table untouched): a table made
 *                             with another context or for another database; an identifier below 0, given twice in the
 *                             call, or already merged for this page; opts->distinct_sites other than that of the pages
 *                             merged so far.  A merge that fails part way leaves the table unusable.
 *   prb_covset_add_hits       the same merge for a caller's list of final hits of one page in host memory: prb_hit
 *                             records with their pair array as prb_hitset_hits / prb_hitset_basepairs or a `ris -b` file
 *                             hold them, ascending by `query` (0 <= query < nq), every hit with at least one pair (the
 *                             first and the last are its ends); query_ids[nq] as above.  Stage counts are not touched.
 *                             The refusals of prb_search_page_coverage but for the options; n = 0 only marks the
 *                             identifiers as merged
 *   prb_covset_merge          two unfinished tables into one, on the device, with the contract of prb_targetset_merge:
 *                             the difference and start arrays add, the best hit is the lower (e_min, query id, place); src
 *                             may live on another device (a peer copy, else through pinned host memory); both were made
 *                             for the same database (the handles may differ), hold the same distinct_sites unless one is
 *                             empty, and no (query id, page) is merged into both: anything else returns PRB_ERR_ARG and
 *                             leaves both tables as they were.  src is left empty but valid
 *   prb_covset_finish         1 <= min_queries <= 1000000: the scans of the difference arrays, the regions' first
 *                             positions and the reduction of every region to its record, all on the device; one copy to
 *                             the host, and the device memory is released.  Nothing can be merged after it (a second call
 *                             does nothing, whatever its min_queries)
 *   prb_covset_counts         the stage counts of prb_pairset_counts, summed over the merged searches
 * The device time of all this is the stage "coverage" of prb_ctx_stage_ms. */
typedef struct prb_target_region {
  int32_t page, db_id;
  int32_t start, end;
  int64_t hits, max_hits;
  int32_t max_queries, peak;
  double e_min;
  int32_t query, reserved;
  int32_t bp_first[2], bp_last[2]; /* the best hit's (q, db) end pairs; db in the page's reversed text */
} prb_target_region;
#ifdef __cplusplus
static_assert(sizeof(prb_target_region) == 72, "prb_target_region: no padding");
#endif
typedef struct prb_covset prb_covset;
int prb_covset_create(prb_ctx *ctx, prb_db *db, prb_covset **out);
int prb_search_page_coverage(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts,
                             const int32_t *query_ids, prb_covset *cs);
int prb_covset_add_hits(prb_ctx *ctx, prb_covset *cs, int32_t page, const int32_t *query_ids, int32_t nq, const prb_hit *hits,
                        int64_t nhits, const int32_t *basepairs, int64_t npairs);
int prb_covset_merge(prb_ctx *ctx, prb_covset *dst, prb_covset *src);
int prb_covset_finish(prb_ctx *ctx, prb_covset *cs, int32_t min_queries);
int64_t prb_covset_size(const prb_covset *cs);
const prb_target_region *prb_covset_regions(const prb_covset *cs);
void prb_covset_counts(const prb_covset *cs, int64_t counts[3]);
void prb_covset_free(prb_covset *cs);

/* ---- an empirical p-value per pair from shuffled decoys (`ris -t -z N`): a null table on the device ----
 * Raw energies are not comparable across queries - a long GC-rich query gets a low e_min against everything.  For one batch
 * of real queries, one database and N decoys per query, the decoys of a query are
 *     prb_shuffle_sequence(seq, len, seed, file_pos, decoy, out)   for decoy = 0 .. N - 1
 * and the table holds, over everything merged into it:
 *   observed   a pair (query q, target (page, db_id)) is OBSERVED when q has at least one final hit against the target; its
 *              record `s` is the prb_pair_summary that prb_search_page_summary returns for it, field for field
 *   null_hits  the number of decoys of q that have at least one final hit against the target
 *   null_le    the number of those decoys whose e_min against the target is <= the observed e_min, compared as doubles
 *              (-0.0 == +0.0); a decoy without a hit counts as +infinity, that is, nowhere
 *   null_min   the smallest decoy e_min against the target (of -0.0 and +0.0 the latter is reported); +infinity when
 *              null_hits == 0.  An integer atomic minimum over the order-preserving 64-bit key of the energy
 *   decoys     per pair: the decoys the pair has seen - N, or, for a pair that prb_nullset_retire retired, the `upto` of that
 *              call; null_hits, null_le and null_min are taken over the decoys 0 .. decoys - 1 only.  The p-value is
 *              p = (null_le + 1) / (decoys + 1), computed in double on the host (prb_write_null_lines)
 * Decoy pairs whose (owner, target) is not observed are counted nowhere.  Records come by query, then page, then db_id: an
 * order of this mode's own, not the `-t` order.  Every column is an integer sum or a minimum over a total order, so the
 * table is - bit for bit - independent of how the decoys are cut into batches and sub-batches, of the order of the pages
 * and of the decoy batches, of PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS and page residency, and of whether the decoys were
 * searched under a pair mask that allows (at least) the observed targets of their owners.
 *   prb_nullset_create        an empty table for qb and db, 1 <= ndecoys <= 100000 (else PRB_ERR_ARG): one dense slot per
 *                             (query, target of every page) of 96 B - the 64 B record, three 8 B counters, a flag, the
 *                             decoys seen - and 2 B of selection and live flags, in HBM; PRB_ERR_NOMEM when that cannot be allocated, PRB_ERR_ARG for
 *                             2^32 slots or more.  The table owns all its device memory and must be freed before its
 *                             context, its batch and its database
 *   prb_search_page_observed  the search of prb_search_page_summary of the real batch against `page`, its records
 *                             scattered into the table on the device (nothing is copied to the host).  Argument checks and
 *                             option limits are those of prb_search_page_summary.  The table was made with this context
 *                             for this batch and this database; a page is observed once (else PRB_ERR_ARG)
 *   prb_search_page_decoys    the same search of a batch dqb of decoys, its records folded into the counters on the
 *                             device, one thread per record, integer atomics: owner[q] = the real query's index in the
 *                             table's batch, decoy[q] = the decoy's number, 0 <= decoy[q] < ndecoys, for every query q of
 *                             dqb.  The page must be observed first (else PRB_ERR_STATE); a (owner, decoy, page) triple is
 *                             merged once, and an (owner, decoy) comes once per call (else PRB_ERR_ARG).  It honours
 *                             opts->allowed_pairs (a mask made for dqb) like every search entry
 *   prb_nullset_observe       the scatter of prb_search_page_observed for a caller's records of `page` in host memory
 *   prb_nullset_add_pairs     the fold of prb_search_page_decoys for a caller's records (their `query` indexes owner[nq]
 *                             and decoy[nq]); n = 0 only marks the decoys as merged.  Both take the refusals of the two
 *                             search entries but for the options, and refuse (PRB_ERR_ARG) a record whose query or db_id is
 *                             out of range, whose hits are below 1, or whose (query, db_id) comes twice in the list
 *   prb_nullset_retire        sequential Monte-Carlo p-values (Besag & Clifford 1991; `ris -t -z N -H H`): between two batches
 *                             of decoys, one pass over the slots retires every live pair - an observed pair that has not
 *                             retired - with null_le >= min_le: it takes no further decoy (a record that arrives for it is
 *                             counted nowhere), and its `decoys` is `upto`, the number of decoys per query merged so far.  A
 *                             pair retired earlier keeps its `decoys`.  live_per_query[nq] (may be NULL) = the live pairs
 *                             left per query, counted on the device per wavefront (ballot, popcount, one atomic add per
 *                             wavefront and query).  Checked on the host before anything is enqueued: min_le >= 1; upto is
 *                             above that of the call before and at most ndecoys (PRB_ERR_ARG); every page is observed, and
 *                             every (query, decoy < upto, page) of every query that had live pairs before the call is merged
 *                             (PRB_ERR_STATE).  The caller decides what `upto` means by what it merges first: the result is
 *                             that of the plain table with `upto` decoys, for the pairs that retire here
 *   prb_nullset_finish        PRB_ERR_STATE unless every (query, decoy, page) has been merged - a p-value never rests on
 *                             fewer decoys than it says; with retired pairs, only the queries that still have live pairs
 *                             need all N decoys: for a query without, the decoys from the `upto` on of the
 *                             prb_nullset_retire that found it so are exempt.  The observed slots are selected on the device, their records
 *                             gathered there and copied to the host in one copy; the device memory is released.  Nothing
 *                             can be merged after it (a second call does nothing)
 *   prb_nullset_counts        the stage counts of prb_pairset_counts, summed over the observed pages;
 *   prb_nullset_decoy_counts  the same over the decoy searches (under a pair mask counts[0] counts the allowed pairs' seeds)
 * Every check of a call - owners, decoy numbers, the page, what is merged already - is made on the host before anything
 * is enqueued: a refused call leaves the table untouched; a merge that fails part way leaves it unusable.  On the device
 * every kernel checks its slot and each record's query, db_id, owner and decoy number against the table's ranges again;
 * a violation raises the table's `bad` flag and writes nothing, and the next call on the table returns PRB_ERR_STATE.
 * A table holds pages searched with one value of distinct_sites and of chain_sites (a second one is PRB_ERR_ARG).  There is
 * no prb_nullset_merge: a batch belongs to one worker.  Stage timer "null": the scatter or the fold (launches = 1 per
 * sub-batch with final hits, and per prb_nullset_observe / _add_pairs with records), and prb_nullset_finish: the selection
 * and the gather (launches = 2, or 1 when no pair is observed); prb_nullset_retire: its pass (launches = 1). */
typedef struct prb_null_pair {
  prb_pair_summary s;   /* the observed pair */
  int32_t page, decoys; /* the target's page; the decoys this pair has seen (N unless it retired) */
  int64_t null_hits, null_le;
  double null_min;
} prb_null_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_null_pair) == 96, "prb_null_pair: no padding");
#endif
int prb_nullset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t ndecoys, prb_nullset **out);
int prb_search_page_observed(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_nullset *ns);
int prb_search_page_decoys(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *owner,
                           const int32_t *decoy, prb_nullset *ns);
int prb_nullset_observe(prb_ctx *ctx, prb_nullset *ns, int32_t page, const prb_pair_summary *pairs, int64_t n);
int prb_nullset_add_pairs(prb_ctx *ctx, prb_nullset *ns, int32_t page, const int32_t *owner, const int32_t *decoy, int32_t nq,
                          const prb_pair_summary *pairs, int64_t n);
int prb_nullset_retire(prb_ctx *ctx, prb_nullset *ns, int64_t min_le, int32_t upto, int64_t *live_per_query);
int prb_nullset_finish(prb_ctx *ctx, prb_nullset *ns);
int64_t prb_nullset_size(const prb_nullset *ns);
const prb_null_pair *prb_nullset_pairs(const prb_nullset *ns);
void prb_nullset_counts(const prb_nullset *ns, int64_t counts[3]);
void prb_nullset_decoy_counts(const prb_nullset *ns, int64_t counts[3]);
void prb_nullset_free(prb_nullset *ns);

/* ---- a Benjamini-Hochberg q-value per pair of the null table (`ris -t -z N -Q`), ranked on the device ----
 * A query is searched against every target, so the p-values of a null table are read many at a time: which pairs survive
 * that many tests?  Sequential Monte-Carlo p-values (prb_nullset_retire) followed by the step-up procedure is the form the
 * false-discovery-rate correction was worked out for (Besag & Clifford 1991; Benjamini & Hochberg 1995).  All in integers:
 * take one query q.  Its observed pairs are a with num_a = null_le_a + 1 and den_a = decoys_a + 1 (decoys_a: N, or the
 * `upto` at which the pair retired); the p-value is the exact rational p_a = num_a / den_a.  tests_q is the number of
 * hypotheses of q - the targets it was searched against; an unobserved target has p = 1 and takes part through tests_q
 * only.
 *   rank_a    the observed pairs b of q with p_b <= p_a, a itself among them; equal rationals share it (1/2 and 2/4)
 *   FDR_a     tests_q * num_a / (den_a * rank_a)
 *   QValue_a  min(1, the minimum of FDR_b over the observed pairs b of q with p_b >= p_a), kept as the minimising pair's
 *             triple (q_num, q_den, q_rank) = (num_g, den_g, rank_g): among equal fractions the g of lowest rank, among
 *             those - which share their p - the one of lowest den.  A minimum above 1 is the triple (0, 0, 0).
 * A host prints 1 for (0, 0, 0) and else (double)(tests * q_num) / (double)((uint64_t)q_den * q_rank): both operands are
 * exact in double, so one division rounds it (prb_write_null_fdr_lines).  No float decides an order: p-values are ordered
 * by the 41-bit key (num << 40) / den, which is exact for denominators up to 100001, FDR fractions by cross-multiplication
 * in 64 bits (DESIGN.md has both arguments).  Every figure is a count over a total order or a minimum under one, so they
 * are - bit for bit - independent of everything the null table's records are independent of, and of the order in which
 * the sort leaves equal keys.
 *   prb_nullset_finish_fdr  prb_nullset_finish - every check and every refusal of it, the same records in the same order,
 *                           byte for byte - with the figures beside them.  tests[nq] = tests_q per query, or NULL: every
 *                           target of the database.  PRB_ERR_ARG, checked on the host before anything is enqueued, when a
 *                           tests[q] is below 1 or 2^31 or more, when the database has 2^30 targets or more (the cross
 *                           products would leave 64 bits) or the batch more than 2^23 queries (the sort key would).  The
 *                           observed pairs per query are known on the device only: they are counted there by the key
 *                           pass, behind the selection, and a tests[q] below its query's count is PRB_ERR_ARG before the
 *                           ranking is enqueued.  A call refused with PRB_ERR_ARG leaves the table as it was - unfinished,
 *                           to be finished by either entry.  A slot whose null_le exceeds its decoys (decoys beyond `upto`
 *                           were merged before prb_nullset_retire) has no p-value: it raises the table's `bad` flag
 *                           (PRB_ERR_STATE, the table is unusable, nothing is written; so is a table whose counts and selection disagree).  After a plain prb_nullset_finish the call does nothing,
 *                           like a second finish
 *   prb_nullset_fdr         the figures, parallel to prb_nullset_pairs; NULL after a plain finish
 *   prb_fdr_chunk           the entries of a query's sorted segment that the step-up pass scans at a time (tests place
 *                           segments across its multiples)
 * Stage timer "fdr": the key pass (launches = 1), then the sort by (query, p-key), the rank pass, the step-up pass and the
 * scatter (launches = 4); nothing for a table without observed pairs.  The selection and the gather stay under "null". */
typedef struct prb_null_fdr {
  int64_t tests;                       /* tests_q of the pair's query */
  uint32_t rank, q_rank, q_num, q_den; /* rank_a; the triple of QValue_a */
} prb_null_fdr;
#ifdef __cplusplus
static_assert(sizeof(prb_null_fdr) == 24, "prb_null_fdr: no padding");
#endif
int prb_nullset_finish_fdr(prb_ctx *ctx, prb_nullset *ns, const int64_t *tests);
const prb_null_fdr *prb_nullset_fdr(const prb_nullset *ns);
int32_t prb_fdr_chunk(void);

/* ---- one record per (query, group of targets) (`ris -t -G FILE`): a group table on the device ----
 * A transcriptome lists isoforms that share most of their exons, so a strong interaction comes back once per isoform.  A
 * GROUP MAP gives every database sequence (page, db_id) a group index g in [0, G), 1 <= G <= the number of sequences (a
 * gene, say).  For one batch of queries and one database the table holds, over everything merged into it, one record per
 * (query, group) that has at least one member pair with a final hit:
 *   s         the group's BEST member pair: field for field the prb_pair_summary that prb_search_page_summary returns for
 *             it.  Best = the lowest e_min, compared as doubles (-0.0 == +0.0; the stored record keeps the bits it came
 *             with); ties go to the lower page, then the lower db_id.  This is a total order that the record itself
 *             carries.  It is NOT the tie rule of the top-N table (prb_topset), which orders equal energies by the pair's
 *             position in its page's list: a dense fold has no such position
 *   page      the best member's page;  group: g
 *   members   the member targets with at least one final hit
 *   hits      the sum of the members' s.hits.  No energy is summed across members: isoforms share exons, so such a sum
 *             would count one site several times, and a floating-point sum would depend on the merge order.  s.e_sum and
 *             s.hits are the best member's own
 *   rank      the record's rank within its query under a top-N selection, else 0
 * Every column is an integer sum or a minimum over a total order, so the table is - bit for bit - independent of the
 * order of the pages, of how a batch is cut into sub-batches and chunks (PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS, page
 * residency) and of how the pages are shared between tables that are merged later.
 *   prb_groupset_create     an empty table for qb and db; group_of_page[p][db_id] = the group of sequence db_id of page p,
 *                           every value in [0, ngroups) (checked on the host, else PRB_ERR_ARG; uploaded once per page).
 *                           The table is dense: one slot of 96 B per (query, group) - the 64 B record, its two 8 B keys,
 *                           the two counters - in HBM, plus 4 B per database sequence for the map; PRB_ERR_ARG for 2^32
 *                           slots or more, PRB_ERR_NOMEM when the table cannot be allocated.  It owns all its device
 *                           memory and must be freed before its context, its batch and its database
 *   prb_search_page_groups  the search of prb_search_page_summary against `page`, its records folded into the table on the
 *                           device (nothing is copied to the host): integer atomics for the counters, staged 64-bit atomic
 *                           minima for the best member (energy key, then page << 32 | db_id among the records that hold the
 *                           slot's energy; the one winner writes its record).  Argument checks and option limits are those
 *                           of prb_search_page_summary; it honours distinct_sites, chain_sites and allowed_pairs.  The
 *                           table was made with this context for this batch and this database; a page is merged once
 *   prb_groupset_add_pairs  the same fold for a caller's records of `page` in host memory.  PRB_ERR_ARG, table untouched,
 *                           for a record whose query or db_id is out of range or whose hits are below 1, a (query, db_id)
 *                           that comes twice in the list, and a page already merged
 *   prb_groupset_merge      two unfinished tables over disjoint page sets into one, on the device, under the rules of
 *                           prb_topset_merge; the two maps must be equal.  dst then holds - bit for bit - the table of the
 *                           union; src is left empty: it can be freed, or finished to zero records
 *   prb_groupset_finish     n = 0: the occupied slots are selected on the device, their records gathered there and copied
 *                           to the host in one copy: by query ascending, then group ascending, rank = 0.  1 <= n <= 1024:
 *                           only each query's n groups of lowest s.e_min, ties by (page, s.db_id) of the best member, by
 *                           query, then rank (a workgroup per query selects in LDS).  Any other n is PRB_ERR_ARG.  The
 *                           device memory is released; nothing can be merged after it (a second call does nothing)
 *   prb_groupset_counts     the stage counts of prb_pairset_counts, summed over the searched pages
 * A call refused by its checks leaves the table as it was; a merge that fails part way leaves it unusable.  On the device
 * every kernel checks query, db_id, page and group against the table's ranges again; a violation raises the table's `bad`
 * flag and writes nothing, and the next call on the table returns PRB_ERR_STATE.  A table holds pages searched with one
 * value of distinct_sites and of chain_sites.  Stage timer "group": the fold (launches = 3 per sub-batch with final hits
 * and per prb_groupset_add_pairs with records), prb_groupset_merge (1), and prb_groupset_finish: the flags, the selection
 * and the gather (launches = 3, or 2 when the table is empty; with n > 0 two more, the per-query selection and the
 * selection of the kept ranks). */
typedef struct prb_group_pair {
  prb_pair_summary s;    /* the group's best member pair */
  int32_t page, group;   /* the best member's page; the group index */
  int32_t members, rank; /* member targets with >= 1 final hit; rank within the query (0 without a top-N selection) */
  int64_t hits;          /* sum of the members' s.hits */
} prb_group_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_group_pair) == 88, "prb_group_pair: no padding");
#endif
typedef struct prb_groupset prb_groupset;
int prb_groupset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, const int32_t *const *group_of_page, int32_t ngroups,
                        prb_groupset **out);
int prb_search_page_groups(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_groupset *gs);
int prb_groupset_add_pairs(prb_ctx *ctx, prb_groupset *gs, int32_t page, const prb_pair_summary *pairs, int64_t n);
int prb_groupset_merge(prb_ctx *ctx, prb_groupset *dst, prb_groupset *src);
int prb_groupset_finish(prb_ctx *ctx, prb_groupset *gs, int32_t n);
int64_t prb_groupset_size(const prb_groupset *gs);
const prb_group_pair *prb_groupset_pairs(const prb_groupset *gs);
void prb_groupset_counts(const prb_groupset *gs, int64_t counts[3]);
void prb_groupset_free(prb_groupset *gs);
/* The lines of `ris -t -G FILE` for one batch: per record the `-t` line of the best member (prb_write_summary_lines'
 * columns, numbered from id0 on) followed by ",<group name>,<members>,<targets in the group>,<hits>"; group_names[g] and
 * group_sizes[g] for every group of the table.  Arguments and results as prb_write_top_lines. */
int prb_write_group_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_group_pair *recs,
                          int64_t nrecs, const char *const *group_names, const int32_t *group_sizes, int32_t ngroups, int64_t id0, int fd,
                          int64_t *nlines, int64_t *nbytes);

/* ---- the N best queries per group (`ris -t -G FILE -R N`): a group ranking table on the device ----
 * prb_targetset ranks the queries of a run per database sequence, and so returns a gene once per isoform; a group table
 * lives for one batch.  A group ranking table holds, for every group g in [0, ngroups), the N records of lowest s.e_min
 * among all the (query, group) records merged into it over a whole run (fewer when the group has fewer).  A record is a
 * prb_group_pair exactly as prb_groupset_finish(gs, 0) returns it, but `s.query` holds a caller-given identifier, int32
 * >= 0, as in prb_search_page_targets (the command line: the 0-based position in the input FASTA), and `rank` the rank
 * within the group.  Records of a group are ranked by s.e_min ascending, compared as doubles (-0.0 == +0.0; the stored
 * record keeps the bits it came with); equal values are ordered by the identifier ascending.  An (identifier, group)
 * occurs at most once, so it is a total order, and the finished table depends - bit for bit - neither on how the queries
 * are cut into batches or sub-batches, nor on the order of the batches, nor on which context (worker) took what.
 *   prb_grouprank_create        an empty table (1 <= n <= 1024, ngroups >= 1, else PRB_ERR_ARG): n slots of 88 B and n
 *                               keys of 16 B per group, plus a fill count per group, in HBM; PRB_ERR_NOMEM when that
 *                               cannot be allocated
 *   prb_grouprank_add_groupset  every occupied slot of the UNFINISHED group table gs merged into the table, on the
 *                               device: nothing is copied to the host, and gs is left untouched - it can still be
 *                               finished or merged.  query_ids[q] = the identifier of query q of gs's batch.  Refused,
 *                               the table untouched: gs or the table made with another context, a gs with another
 *                               number of groups, an identifier below 0, given twice in the call or already merged into
 *                               the table, distinct_sites or chain_sites other than those the table holds (PRB_ERR_ARG);
 *                               a gs that is finished, broken or bad, and a gs that has NOT had every page of its
 *                               database merged - a group's minimum over some of its members is never ranked -
 *                               (PRB_ERR_STATE).  The stage counts of gs are added to the table's
 *   prb_grouprank_add_records   the same merge for a caller's records in host memory whose s.query holds the identifier
 *                               already (tests; callers with a fold of their own).  PRB_ERR_ARG, table untouched: a group
 *                               outside the table, an identifier below 0, an (identifier, group) given twice in the call,
 *                               an identifier merged by an earlier call - every identifier of a call is marked as merged,
 *                               so all the records of one identifier come in one call.  n = 0 does nothing
 *   prb_grouprank_merge         two unfinished tables into one, on the device, under the contract of prb_targetset_merge:
 *                               src may live on another device; both have the same n and ngroups, hold the same
 *                               distinct_sites and chain_sites unless one is empty, and no identifier is merged into
 *                               both: anything else returns PRB_ERR_ARG and leaves both tables as they were.  dst then
 *                               holds - bit for bit - the table of all that was merged into either; src is left empty but
 *                               valid
 *   prb_grouprank_finish        the filled slots compacted on the device (a scan over the fills, a gather in rank order)
 *                               and copied to the host in one copy; the device memory is released.  prb_grouprank_pairs
 *                               then returns the records by group ascending, then rank; `rank` counts from 0 within the
 *                               group.  Nothing can be merged after it (a second call does nothing)
 *   prb_grouprank_counts        the stage counts of prb_groupset_counts, summed over the group tables merged
 * A merge works in one linear pass over the group table's dense slots - the flags of the occupied ones and their
 * compaction - plus work in proportion to the occupied ones: their groups as sort keys, a stable sort by group, the rank
 * keys (the monotone 64-bit key of e_min, the identifier) and the heads of the groups' runs, and a wavefront per run that
 * merges it into the group's ranked list in LDS - the lists, the merge and the gather of the per-target table.  No
 * floating-point atomics, and nothing depends on the order in which threads arrive.  On the device every kernel checks
 * slot, group, query and identifier against the tables' ranges again; a violation raises the table's `bad` flag and
 * writes nothing, and this and every later call on the table returns PRB_ERR_STATE.  A merge that fails part way leaves
 * the table unusable.  Stage timer "grouprank": prb_grouprank_add_groupset (launches = 7: flags, compaction, sort keys,
 * sort, rank keys and heads, selection of the heads, merge; 2 when the group table is empty), prb_grouprank_add_records
 * (5), prb_grouprank_merge (1); the launches booked to "group" are those of the group table's own calls, as ever. */
typedef struct prb_grouprank prb_grouprank;
int prb_grouprank_create(prb_ctx *ctx, int32_t ngroups, int32_t n, prb_grouprank **out);
int prb_grouprank_add_groupset(prb_ctx *ctx, prb_grouprank *gr, const prb_groupset *gs, const int32_t *query_ids);
int prb_grouprank_add_records(prb_ctx *ctx, prb_grouprank *gr, const prb_group_pair *recs, int64_t n);
int prb_grouprank_merge(prb_ctx *ctx, prb_grouprank *dst, prb_grouprank *src);
int prb_grouprank_finish(prb_ctx *ctx, prb_grouprank *gr);
int64_t prb_grouprank_size(const prb_grouprank *gr);
const prb_group_pair *prb_grouprank_pairs(const prb_grouprank *gr);
void prb_grouprank_counts(const prb_grouprank *gr, int64_t counts[3]);
void prb_grouprank_free(prb_grouprank *gr);
/* The lines of `ris -t -G FILE -R N`: recs[0, nrecs) as prb_grouprank_pairs returns them (by group, then rank), one line
 * each in that order, numbered from id0 on; every line is the prb_write_group_lines line of its record.  qnames and
 * qlen_unmasked are indexed by the query's identifier (nq_total of them: every s.query lies below it). */
int prb_write_grouprank_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                              const prb_group_pair *recs, int64_t nrecs, const char *const *group_names, const int32_t *group_sizes,
                              int32_t ngroups, int64_t id0, int fd, int64_t *nlines, int64_t *nbytes);

/* ---- an empirical p-value per (query, group) from shuffled decoys (`ris -t -G FILE -P N`): a group null table ----
 * A group's record reports the minimum e_min over its members, so its null is the distribution of the DECOYS' minimum over
 * the same members - members the real query never hit included, and a decoy that beats the observed energy on two isoforms
 * counting once.  No fold of the per-pair columns of prb_nullset yields that count, and the best member's pair-level p-value
 * is anti-conservative, more so the more members a group has.  For one batch of real queries, one database, a group map as
 * prb_groupset_create takes it and N decoys per query - prb_shuffle_sequence(seq, len, seed, file_pos, decoy, out) for
 * decoy = 0 .. N - 1, as for prb_nullset -:
 *   kept       the KEPT groups of query q are the records prb_groupset_finish(gs, n) returns for it: every occupied (q, group)
 *              for n = 0, else its n best.  g = such a record, field for field; e_obs = g.s.e_min
 *   m(q, d, g) for a kept (q, g) and decoy d of q: the minimum of the decoy's pair e_min over all targets of group g, of every
 *              page, whether or not q itself has a hit against the target; +infinity when the decoy has no final hit in g
 *   null_hits  the number of decoys d with m < +infinity
 *   null_le    the number of decoys d with m <= e_obs, compared as doubles (-0.0 == +0.0)
 *   null_min   the minimum of m over d (of -0.0 and +0.0 the latter is reported); +infinity when null_hits == 0
 *   decoys     N; the p-value is p = (null_le + 1) / (N + 1), computed in double on the host (prb_write_gnull_lines)
 * Decoy pairs of a group that is not kept for their owner are counted nowhere.  Every column is an integer sum or a minimum
 * over a total order, so the table is - bit for bit - independent of how the decoys are cut into batches and sub-batches, of
 * the order of the pages and of the decoy batches, of PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS and page residency, and of
 * whether the decoys were searched under a pair mask that allows (at least) the members of their owners' kept groups.
 *   prb_gnullset_create      finishes gs exactly as prb_groupset_finish(ctx, gs, n) does - the records are then to be had
 *                            from prb_groupset_pairs(gs) - and keeps on the device what the decoys need: the kept records,
 *                            a dense lookup of 4 B per (query, group), 32 B of key and counters per record, the page maps.
 *                            PRB_ERR_STATE unless every page is merged into gs (and for a finished, broken or bad gs);
 *                            PRB_ERR_ARG unless 1 <= ndecoys <= 100000, and for any n that prb_groupset_finish refuses.  The
 *                            table owns all its device memory and must be freed before its context
 *   prb_gnullset_begin       opens a batch of ndq >= 1 decoys: owner[k] = the real query's index in the group table's batch,
 *                            decoy[k] = the decoy's number.  PRB_ERR_ARG when an (owner, decoy) is out of range, comes twice
 *                            or belongs to a batch closed before; PRB_ERR_STATE when a batch is open; PRB_ERR_NOMEM, with the
 *                            size in the message, when the scratch of 8 B x ndq x groups cannot be had
 *   prb_search_page_gnull    the search of prb_search_page_summary of the batch dqb of decoys (dqb's queries are the open
 *                            batch's, in its order: else PRB_ERR_ARG) against `page`, its records folded on the device into
 *                            the scratch: an atomic minimum of the energy key per (decoy, group), a thread per record.  A page
 *                            comes once per open batch.  It honours allowed_pairs (a mask made for dqb), distinct_sites and
 *                            chain_sites; of the latter two a table takes one value, the one gs was searched with
 *   prb_gnullset_add_pairs   the same fold for a caller's records of `page` in host memory (their `query` indexes the open
 *                            batch); n = 0 only marks the page as merged.  PRB_ERR_ARG for a record whose query or db_id is
 *                            out of range, whose hits are below 1, or whose (query, db_id) comes twice in the list
 *   prb_gnullset_end         PRB_ERR_STATE unless every page is merged in the open batch.  Every scratch cell that holds a
 *                            minimum is counted into its record and emptied, a thread per cell; the batch's (owner, decoy)
 *                            pairs are closed
 *   prb_gnullset_finish      PRB_ERR_STATE unless every (query, decoy) is closed and no batch is open - a p-value never rests
 *                            on fewer decoys than it says.  The records are gathered on the device and copied to the host in
 *                            one copy; the device memory is released (a second call does nothing)
 *   prb_gnullset_pairs       the records, in the order and number of prb_groupset_pairs(gs)
 *   prb_gnullset_decoy_counts  the stage counts of prb_pairset_counts, summed over the decoy searches
 * Every check of a call is made on the host before anything is enqueued: a refused call leaves the table untouched; a merge
 * that fails part way leaves it unusable.  On the device every kernel checks query, db_id, page, group, owner and decoy
 * against the table's ranges again; a violation raises the table's `bad` flag and writes nothing, and the next call on the
 * table returns PRB_ERR_STATE.  There is no prb_gnullset_merge: a batch belongs to one worker.  Stage timer "gnull":
 * launches = 1 for prb_gnullset_create with records to keep, 1 per sub-batch with final hits and per prb_gnullset_add_pairs
 * with records (the fold), 1 per prb_gnullset_end (the close), 1 for prb_gnullset_finish with records (the gather). */
typedef struct prb_gnull_pair {
  prb_group_pair g;      /* the kept (query, group) record */
  int32_t decoys, pad;   /* N; 0 */
  int64_t null_hits, null_le;
  double null_min;
} prb_gnull_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_gnull_pair) == 120, "prb_gnull_pair: no padding");
#endif
typedef struct prb_gnullset prb_gnullset;
int prb_gnullset_create(prb_ctx *ctx, prb_groupset *gs, int32_t n, int32_t ndecoys, prb_gnullset **out);
int prb_gnullset_begin(prb_ctx *ctx, prb_gnullset *gn, const int32_t *owner, const int32_t *decoy, int32_t ndq);
int prb_search_page_gnull(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_gnullset *gn);
int prb_gnullset_add_pairs(prb_ctx *ctx, prb_gnullset *gn, int32_t page, const prb_pair_summary *pairs, int64_t n);
int prb_gnullset_end(prb_ctx *ctx, prb_gnullset *gn);
int prb_gnullset_finish(prb_ctx *ctx, prb_gnullset *gn);
int64_t prb_gnullset_size(const prb_gnullset *gn);
const prb_gnull_pair *prb_gnullset_pairs(const prb_gnullset *gn);
void prb_gnullset_decoy_counts(const prb_gnullset *gn, int64_t counts[3]);
void prb_gnullset_free(prb_gnullset *gn);
/* The lines of `ris -t -G FILE -P N` for one batch: per record the line of prb_write_group_lines, and behind it the five
 * columns that prb_write_null_lines puts behind a `-t` line: ,Decoys,NullHits,NullLE,NullMin,PValue - in the same forms. */
int prb_write_gnull_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_gnull_pair *recs,
                          int64_t nrecs, const char *const *group_names, const int32_t *group_sizes, int32_t ngroups, int64_t id0, int fd,
                          int64_t *nlines, int64_t *nbytes);

/* ---- an E-value and an FDR q-value per interaction site from pooled decoys (`ris -k N -E M`): an evalset on the device ----
 * The null tables above score a PAIR and resolve no p-value below 1 / (N + 1).  Here the decoys' hits against the WHOLE
 * database are pooled into one null distribution of hit energies per query, and every real hit is placed in it.  For one
 * batch of real queries, one database and M decoys per query - made as for the null table, prb_shuffle_sequence with decoy =
 * 0 .. M - 1 - the table holds two lists of (query, energy key): the final hits (after distinct_sites / chain_sites) of the
 * real batch, and those of the decoys under their owners.  The key is the order-preserving 64-bit key of the hit's e_tot
 * (-0.0 == +0.0).  For a real hit h of query q, all in integers:
 *   rank      the number of real hits of q with key <= key(h) (h included; equal energies share the value)
 *   null_le   the number of hits of q's M decoys with key <= key(h)
 *   EValue    null_le / M: the decoy hits this good that one search yields by chance
 *   FDR_g     null_le_g / (M * rank_g)
 *   QValue    min(1, the minimum of FDR_g over the real hits g of q with key(g) >= key(h)), kept as the minimising g's pair
 *             (q_num, q_den) = (null_le_g, rank_g) - among equal fractions that of the g of lowest key; (M, 1) when the minimum
 *             exceeds 1.  The host prints q_num / (M * q_den)
 * Fractions are compared exactly by cross-multiplication: a list holds at most 2^32 - 1 keys (more is refused), so every
 * product fits 64 bits; no floating point takes part on the device.  Every figure is a count over a total order: the table
 * is - bit for bit - independent of how the batches are cut, of the order of pages and decoy batches and of the order of
 * the lists.
 *   prb_evalset_create          an empty table for qb and db, 1 <= ndecoys <= 100000 (else PRB_ERR_ARG).  It owns all its
 *                               device memory - 12 B per real hit and per decoy hit while the lists grow - and must be
 *                               freed before its context, its batch and its database
 *   prb_search_page_scored      the real batch's search of `page`, once: the final hits' keys appended to the real list
 *                               (nothing leaves the device).  With tophits != NULL the same sub-batches are handed on to
 *                               that top-N hit table, which ends up byte for byte as prb_search_page_tophits fills it, and
 *                               takes all its refusals (its context, batch, pages, output_style and selection); a page is
 *                               searched once (else PRB_ERR_ARG)
 *   prb_search_page_null_hits   the same search of a batch dqb of decoys, its final hits' keys appended to the decoy list
 *                               under owner[q], for every query q of dqb: no hit records are packed and no base pairs
 *                               gathered.  owner / decoy as for prb_search_page_decoys; an (owner, decoy, page) is accepted
 *                               once, an (owner, decoy) once per call (else PRB_ERR_ARG).  It honours opts->allowed_pairs
 *   prb_evalset_add_keys        the append for a caller's list: energy[i] under query_or_owner[i], into the real list
 *                               (is_decoy == 0) or the decoy list
 *   prb_evalset_close           PRB_ERR_STATE unless - when anything was merged by a search - every page of the real batch and
 *                               every (query, decoy, page) is merged; lists given through prb_evalset_add_keys alone close
 *                               as they are.  Both lists are sorted by (query, key), every real hit gets its rank, null_le
 *                               and the pair of its q-value.  Nothing can be merged after it (a second call does nothing)
 *   prb_evalset_score           after the close: out[i] for the real hit (query[i], energy[i]), looked up by its key on the
 *                               device, one copy back.  A key that the query's real list does not hold is an error
 *   prb_evalset_sizes           the keys in the real and in the decoy list
 *   prb_evalset_counts          the stage counts of prb_hitset_counts summed over the real batch's pages;
 *   prb_evalset_decoy_counts    the same over the decoy searches
 * Every check of a call is made on the host before anything is enqueued: a refused call leaves the table untouched; a merge
 * that fails part way leaves it unusable.  On the device every kernel checks each record's query, owner and decoy number
 * against the table's ranges again; a violation - and a looked-up key that is not there - raises the table's `bad` flag,
 * writes nothing, and this and every later call on the table returns PRB_ERR_STATE.  A table holds pages searched with one
 * value of distinct_sites and of chain_sites (a second one is PRB_ERR_ARG).  There is no merge of two evalsets: a batch
 * belongs to one worker.  Stage timer "eval": the appends (launches = 1 per sub-batch with final hits and per
 * prb_evalset_add_keys with keys), the close (sorts, counts, ranks, suffix minima) and the look-ups. */
typedef struct prb_eval_score {
  int32_t decoys, reserved; /* M; 0 */
  int64_t null_le, rank;
  uint32_t q_num, q_den;
} prb_eval_score;
#ifdef __cplusplus
static_assert(sizeof(prb_eval_score) == 32, "prb_eval_score: no padding");
#endif
typedef struct prb_evalset prb_evalset;
int prb_evalset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_db *db, int32_t ndecoys, prb_evalset **out);
int prb_search_page_scored(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_tophits *tophits,
                           prb_evalset *es);
int prb_search_page_null_hits(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, const int32_t *owner,
                              const int32_t *decoy, prb_evalset *es);
int prb_evalset_add_keys(prb_ctx *ctx, prb_evalset *es, int32_t is_decoy, const int32_t *query_or_owner, const double *energy, int64_t n);
int prb_evalset_close(prb_ctx *ctx, prb_evalset *es);
int prb_evalset_score(prb_ctx *ctx, prb_evalset *es, const int32_t *query, const double *energy, int64_t n, prb_eval_score *out);
void prb_evalset_sizes(const prb_evalset *es, int64_t *nreal, int64_t *ndecoy);
void prb_evalset_counts(const prb_evalset *es, int64_t counts[3]);
void prb_evalset_decoy_counts(const prb_evalset *es, int64_t counts[3]);
void prb_evalset_free(prb_evalset *es);

/* ---- one record per (query, annotated feature of a target) (`ris -t -A FILE`): a feature table on the device ----
 * `-t` answers "which targets", `-G` folds targets into genes; this table looks one level below the target: WHERE on a
 * transcript a query binds, in the terms transcripts are annotated with (5'UTR, CDS, 3'UTR, an exon, a motif).
 * An ANNOTATION is a list of features; feature i is (page, db_id, start, end): start <= end, inclusive, in the target's
 * FORWARD coordinates - the numbers that the base-pair field of a result line prints, the convention of
 * prb_target_region.start / end: length - 1 - (text position - start_pos).  Features of one target may overlap, nest or
 * repeat; a target may have none.
 * The SPAN of a final hit on its target is prb_covset's: [min(db0, dbN), max(db0, dbN)] of its first and last base pair in
 * the `-s 0` form, in forward coordinates.  A hit BELONGS to every feature of its target that its span shares at least
 * one position with; it is INSIDE a feature when its span lies wholly within it.  A hit that belongs to no feature is
 * UNASSIGNED: it is counted (prb_featset_unassigned) and appears in no record.
 * One record per (query, feature) with at least one hit:
 *   s         a prb_pair_summary over the feature's hits under exactly the rules of prb_search_page_summary: hits; e_min
 *             with strict `<`, so the first hit in output order with that e_tot is the best hit; e_sum added left to right
 *             in output order from 0.0; the best hit's e_acc, e_hyb, bp_first, bp_last; s.db_id = the target
 *   page      the target's page;  feature: the caller's index i
 *   inside    the hits among s.hits whose span lies wholly within the feature
 * The finished records come by query ascending, then page, then - within a page - in the order of the (query, target)
 * runs of the merged lists, which for a search is db_id ascending; a target's features come by (start, end, index).
 * A feature lies in one page, a (query, target) run lies in one sub-batch, and every column is a count or a left-to-right
 * fold in output order: the records depend - bit for bit - neither on how the batch is cut into sub-batches and chunks
 * (PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS), nor on page residency, nor on the order of the pages, nor on how the pages
 * are shared between tables that are merged later.
 *   prb_annot_create           n >= 0 features of db checked one by one - page and db_id in range, 0 <= start <= end <
 *                              the target's length; the first bad entry is PRB_ERR_ARG with its index in the message, and
 *                              nothing is made -, sorted by (page, db_id, start, end, index) on the host and uploaded as
 *                              one CSR per page: the first feature of every sequence, then the features' two ends - as
 *                              positions of the page's text - and their indices, beside the sequences' start positions
 *                              and lengths.  It belongs to `db` (as a prb_pairmask does) and must be freed before it,
 *                              and after every table made with it
 *   prb_featset_create         an empty table for qb and the annotation (of a database on ctx's device)
 *   prb_search_page_features   the search of prb_search_page_summary against `page`, every sub-batch's final hits folded
 *                              on the device; nothing leaves it.  Argument checks and option limits are those of
 *                              prb_search_page_summary; it honours distinct_sites, chain_sites (the kept hits are folded)
 *                              and allowed_pairs.  Refusals (PRB_ERR_ARG, or PRB_ERR_STATE for a finished or broken table;
 *                              the table untouched) as prb_search_page_groups: another context, batch or database, a
 *                              page merged twice, a second value of distinct_sites or chain_sites
 *   prb_featset_add_hits       the same fold for a caller's list of final hits of one page in host memory: prb_hit records
 *                              with their pair array as prb_covset_add_hits takes them, ascending by `query` (0 <= query <
 *                              the batch's queries); the (query, db_id) runs are the maximal runs of consecutive records.
 *                              The list is checked on the host first (PRB_ERR_ARG for an inconsistent record); a span that
 *                              leaves its sequence fails with PRB_ERR_STATE - before anything is merged here; the kernels
 *                              check again and raise the table's `bad` flag.  Stage counts are not touched
 *   prb_featset_merge          two unfinished tables over disjoint page sets into one, on the device, with the contract of
 *                              prb_topset_merge: src may live on another device (a peer copy, else through pinned host
 *                              memory; the caller's device is restored); both were made for the same queries and for equal
 *                              annotations (the handles may differ).  src is left empty but valid
 *   prb_featset_finish         the per-(page, query) record counts scanned by query, then page, the records gathered in
 *                              that order on the device and copied to the host in one copy; the device memory is released,
 *                              and nothing can be merged after it (a second call does nothing)
 *   prb_featset_finish_top     prb_featset_finish - its guards and its effects -, but only each query's n best records
 *                              leave the device, ranked there (below).  PRB_ERR_ARG unless 1 <= n <= 1024, the table
 *                              untouched.  On a finished table: PRB_OK and nothing done if it was finished by this call
 *                              with the same n; PRB_ERR_STATE otherwise - after prb_featset_finish, and with another n -,
 *                              as is prb_featset_finish on a table finished by this call: a silent unranked result would
 *                              be worse than a refusal.  prb_featset_size / _records then give the ranked records
 *   prb_featset_unassigned     the final hits merged so far that belong to no feature
 *   prb_featset_counts         the stage counts of prb_pairset_counts, summed over the searched pages
 * THE RANKED CUT (prb_featset_finish_top, prb_fnullset_create_top; `ris -t -A FILE -N K`).  For a query q take the
 * records that prb_featset_finish would return for q, in that order - page, then the (query, target) runs in list order,
 * then a target's features by (start, end, index) -, and let p be a record's place in that order.  The rank key of a
 * record is (energy_key(s.e_min), p), ascending; energy_key is the total order of doubles in which -0.0 == +0.0 that the
 * other ranked tables use.  Ties in e_min are common - a nested feature and its outer feature share their best hit - and
 * are decided by p, so no two records of a query have the same key.  With n given the table keeps the min(n, count)
 * records of lowest key per query; the kept records come by query ascending, then rank, and are field for field the
 * records of the full finish (there is no rank field: the rank is the place within the query's run).  Every quantity is
 * a count or a comparison over a total order, so the result depends - bit for bit - neither on how the batch is cut
 * into sub-batches and chunks (PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS), nor on the order of the pages, nor on page
 * residency, nor on how the pages were shared between tables that were merged (prb_featset_merge).
 * On the device the cut works on the gathered records: a query's records are one segment of them, the segments are cut
 * into chunks of 2048 records, a workgroup per (query, chunk) orders its chunk's keys in LDS and writes the chunk's
 * min(n, length) lowest; a workgroup per query folds its chunks' lists into the final n; a lane per kept record gathers
 * it in (query, rank) order into a second buffer, from which the one host copy is made.
 * On the device a sub-batch's work items are (pair run, feature of its target): a count per run from the CSR, an exclusive
 * scan, and an item kernel - a lane per item, which finds its run by binary search and walks it in list order; items of
 * runs longer than 128 hits go to a wavefront each, which tests 64 hits at a time and adds the members' energies one by
 * one in list order (the same sum, bit for bit).  Items without a hit are compacted out; the survivors are appended to the
 * table's block, which grows geometrically.  Stage timer "feature" (launch counts: prb_ctx_stage_ms). */
typedef struct prb_feature_pair {
  prb_pair_summary s;     /* over the feature's hits; s.db_id = the target */
  int32_t page, feature;  /* the target's page; the feature's index in the caller's list */
  int64_t inside;         /* hits whose span lies wholly within the feature */
} prb_feature_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_feature_pair) == 80, "prb_feature_pair: no padding");
#endif
/* a record of the feature ranking table (prb_featrank_*, below): f.s.query holds the query's identifier */
typedef struct prb_featrank_pair {
  prb_feature_pair f;
  int32_t rank, reserved; /* the rank within the feature, from 0; always 0 */
} prb_featrank_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_featrank_pair) == 88, "prb_featrank_pair: no padding");
#endif
typedef struct prb_annot prb_annot;
typedef struct prb_featset prb_featset;
int prb_annot_create(prb_ctx *ctx, const prb_db *db, int64_t n, const int32_t *page, const int32_t *db_id, const int32_t *start,
                     const int32_t *end, prb_annot **out);
int64_t prb_annot_count(const prb_annot *an);
void prb_annot_free(prb_annot *an);
int prb_featset_create(prb_ctx *ctx, const prb_qbatch *qb, const prb_annot *an, prb_featset **out);
int prb_search_page_features(prb_ctx *ctx, prb_qbatch *qb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_featset *fs);
int prb_featset_add_hits(prb_ctx *ctx, prb_featset *fs, int32_t page, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                         int64_t npairs);
int prb_featset_merge(prb_ctx *ctx, prb_featset *dst, prb_featset *src);
int prb_featset_finish(prb_ctx *ctx, prb_featset *fs);
int prb_featset_finish_top(prb_ctx *ctx, prb_featset *fs, int32_t n);
int64_t prb_featset_size(const prb_featset *fs);
const prb_feature_pair *prb_featset_records(const prb_featset *fs);
void prb_featset_counts(const prb_featset *fs, int64_t counts[3]);
int64_t prb_featset_unassigned(const prb_featset *fs);
void prb_featset_free(prb_featset *fs);
/* The lines of `ris -t -A FILE` for one batch: recs[0, nrecs) as prb_featset_records returns them, one line each in that
 * order, numbered from id0 on: the `-t` line of s (prb_write_summary_lines' columns), and behind it
 *   ,<feature name>,<start>-<end>,<inside>
 * feat_names[i], feat_start[i], feat_end[i] for every feature i of the annotation (nfeat of them).  Arguments and results
 * as prb_write_top_lines. */
int prb_write_feature_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_feature_pair *recs, int64_t nrecs, const char *const *feat_names, const int32_t *feat_start,
                            const int32_t *feat_end, int64_t nfeat, int64_t id0, int fd, int64_t *nlines, int64_t *nbytes);

/* ---- the feature null table: an empirical p-value per (query, feature) record (`ris -t -A FILE -F N`) ----
 * For one batch of real queries, one annotation and N decoys per query, made by prb_shuffle_sequence exactly as for
 * prb_nullset.  No fold of the columns of the other tables yields the counts (as for prb_gnullset): a decoy's hits have
 * to be looked at feature by feature.
 *   kept       the records prb_featset_finish returns for the real batch, field for field and in that order; e_obs = f.s.e_min
 *   m(q, d, f) for a kept (q, f) and decoy d of q: the minimum e_tot over decoy d's final hits against f's target whose
 *              span - prb_featset's: min / max of the first and the last base pair - shares a position with f; +infinity
 *              without such a hit.  It is the s.e_min of the record that a prb_search_page_features run of the decoy
 *              gives for f.
 *   null_hits  the decoys d with m < +infinity
 *   null_le    the decoys d with m <= e_obs, compared as doubles (-0.0 == +0.0)
 *   null_min   the minimum of m over d (+0.0 for +-0.0); +infinity when null_hits == 0
 *   decoys     N; the p-value is p = (null_le + 1) / (N + 1), computed in double on the host (prb_write_fnull_lines)
 * A decoy hit that touches two overlapping features counts once in each; one that touches only features without a kept
 * record for its owner, or no feature, counts nowhere.  The table is bit for bit independent of how the decoys are cut
 * into batches, sub-batches and chunks (PRB_SEARCH_PAIRS, PRB_GAPPED_CHUNK_HITS), of the order of the pages and of the
 * decoy batches, of page residency, and of whether the decoys ran under a pair mask that allows at least the targets of
 * their owners' kept records: every column is an integer count or a minimum over a total order.
 *   prb_fnullset_create      finishes fs exactly as prb_featset_finish does - the records are then to be had from
 *                            prb_featset_records(fs) - and keeps on the device the kept records, a lookup (the records'
 *                            keys (query << 32 | feature) sorted once, 12 B per record, searched by bisection: a dense
 *                            queries x features array is not affordable) and 32 B of key and counters per record.
 *                            PRB_ERR_STATE unless every page is merged into fs, and for a finished, broken or bad fs;
 *                            PRB_ERR_ARG unless 1 <= ndecoys <= 100000.
 *   prb_fnullset_create_top  prb_fnullset_create over the ranked cut: fs is finished exactly as prb_featset_finish_top(fs,
 *                            n) does, and the kept records, the lookup, the counters and every later scratch are sized
 *                            by each query's n best records only; a decoy hit that touches only features cut away counts
 *                            nowhere.  A kept record's counters are those of the same record in the uncut table.
 *                            PRB_ERR_ARG also unless 1 <= n <= 1024.
 *   prb_fnullset_begin       opens a batch of ndq >= 1 decoys: owner[k] = the real query's index in the feature table's
 *                            batch, decoy[k] in [0, ndecoys); the checks of prb_gnullset_begin.  The scratch is 8 B per
 *                            (decoy of the batch, kept record of its owner), addressed through a prefix sum over the
 *                            batch's decoys - not a dense decoy x feature array; PRB_ERR_NOMEM with the size in the message.
 *   prb_search_page_fnull    the search of prb_search_page_features of the batch dqb of decoys (dqb's queries are the open
 *                            batch's decoys, in its order), every sub-batch's final hits folded on the device.  It honours
 *                            allowed_pairs, distinct_sites and chain_sites - of the latter two only the value fs was
 *                            searched with.  A page comes once per open batch.
 *   prb_fnullset_add_hits    the same fold for a caller's list of decoy hits of `page` in host memory (their `query` = the
 *                            place in the open batch), with the host checks of prb_featset_add_hits; nhits = 0 only marks
 *                            the page as merged.
 *   prb_fnullset_end         PRB_ERR_STATE unless every page is merged in the open batch.  Every scratch cell that holds a
 *                            minimum is counted into its record, once, and emptied.
 *   prb_fnullset_finish      PRB_ERR_STATE unless every (query, decoy) is closed and no batch is open.  The records are
 *                            gathered on the device with their counters, and copied once.
 *   prb_fnullset_records     the records, in the order and number of prb_featset_records(fs) (behind
 *                            prb_fnullset_create_top: by query, then rank)
 *   prb_fnullset_decoy_counts  the stage counts of prb_pairset_counts, summed over the decoy searches
 * Every check of a call is made on the host before anything is enqueued: a refused call leaves the table as it was.  The
 * kernels check their ranges again and raise a flag; a table whose flag is raised returns PRB_ERR_STATE.  There is no
 * prb_fnullset_merge: a batch belongs to one worker.  Stage timer "fnull" (launch counts: prb_ctx_stage_ms). */
typedef struct prb_fnull_pair {
  prb_feature_pair f; /* the kept record */
  int32_t decoys, pad;
  int64_t null_hits, null_le;
  double null_min;
} prb_fnull_pair;
#ifdef __cplusplus
static_assert(sizeof(prb_fnull_pair) == 112, "prb_fnull_pair: no padding");
#endif
typedef struct prb_fnullset prb_fnullset;
int prb_fnullset_create(prb_ctx *ctx, prb_featset *fs, int32_t ndecoys, prb_fnullset **out);
int prb_fnullset_create_top(prb_ctx *ctx, prb_featset *fs, int32_t ndecoys, int32_t n, prb_fnullset **out);
int prb_fnullset_begin(prb_ctx *ctx, prb_fnullset *fn, const int32_t *owner, const int32_t *decoy, int32_t ndq);
int prb_search_page_fnull(prb_ctx *ctx, prb_qbatch *dqb, prb_db *db, int32_t page, const prb_ris_opts *opts, prb_fnullset *fn);
int prb_fnullset_add_hits(prb_ctx *ctx, prb_fnullset *fn, int32_t page, const prb_hit *hits, int64_t nhits, const int32_t *basepairs,
                          int64_t npairs);
int prb_fnullset_end(prb_ctx *ctx, prb_fnullset *fn);
int prb_fnullset_finish(prb_ctx *ctx, prb_fnullset *fn);
int64_t prb_fnullset_size(const prb_fnullset *fn);
const prb_fnull_pair *prb_fnullset_records(const prb_fnullset *fn);
void prb_fnullset_decoy_counts(const prb_fnullset *fn, int64_t counts[3]);
void prb_fnullset_free(prb_fnullset *fn);
/* The lines of `ris -t -A FILE -F N` for one batch: the line of prb_write_feature_lines for every record, in the records'
 * order, with the null columns of prb_write_gnull_lines behind it:
 *   ,<decoys>,<null_hits>,<null_le>,<null_min, or NA when null_hits == 0>,<(null_le + 1) / (decoys + 1)>
 * Arguments and results as prb_write_feature_lines. */
int prb_write_fnull_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                          const prb_fnull_pair *recs, int64_t nrecs, const char *const *feat_names, const int32_t *feat_start,
                          const int32_t *feat_end, int64_t nfeat, int64_t id0, int fd, int64_t *nlines, int64_t *nbytes);

/* ---- the N best queries per feature (`ris -t -A FILE -B N`): a feature ranking table on the device ----
 * A feature table lives for one batch, and prb_featset_finish_top ranks features per query.  A feature ranking table
 * holds, for every feature i of the annotation, the N records of lowest s.e_min among all the (query, feature) records
 * merged into it over a whole run (fewer when the feature has fewer).  A record is a prb_featrank_pair: f = the
 * prb_feature_pair exactly as prb_featset_finish returns it, but `f.s.query` holds a caller-given identifier, int32 >= 0,
 * as in prb_search_page_targets (the command line: the 0-based position in the input FASTA); `rank` = the rank within
 * the feature, `reserved` = 0.  Records of a feature are ranked by s.e_min ascending, compared as doubles (-0.0 == +0.0;
 * the stored record keeps the bits it came with); equal values are ordered by the identifier ascending.  A feature lies
 * in one page and a (query, target) run in one sub-batch (above), so a (query, feature) has at most one record, no two
 * keys of a feature's list are equal, and the finished table depends - bit for bit - neither on how the queries are cut
 * into batches or sub-batches, nor on the order of the batches, nor on which context (worker) took what.
 *   prb_featrank_create       an empty table for the annotation (1 <= n <= 1024 and an annotation of at least one feature,
 *                             else PRB_ERR_ARG).  The table is dense: n slots of 88 B and n keys of 16 B per feature,
 *                             plus a fill count per feature, in HBM; PRB_ERR_NOMEM when that cannot be allocated.  The
 *                             annotation must outlive the table
 *   prb_featrank_add_featset  every record of the UNFINISHED feature table fs merged into the table, on the device:
 *                             nothing is copied to the host, and fs is left untouched - it can still be finished or
 *                             merged.  query_ids[q] = the identifier of query q of fs's batch.  Refused, the table
 *                             untouched: fs or the table made with another context, an fs made with another annotation
 *                             (the handles may differ where the annotations are equal), an identifier below 0, given
 *                             twice in the call or already merged into the table, distinct_sites or chain_sites other
 *                             than those the table holds (PRB_ERR_ARG); an fs that is finished, broken or bad, and an fs
 *                             that has NOT had every page of its database merged - every identifier is merged exactly
 *                             once, so half a batch cannot be ranked - (PRB_ERR_STATE).  A complete fs without records
 *                             marks its identifiers and launches nothing.  The stage counts and the unassigned hits of
 *                             fs are added to the table's
 *   prb_featrank_add_records  the same merge for a caller's records in host memory whose f.s.query holds the identifier
 *                             already (tests; callers with a fold of their own); rank and reserved are ignored.
 *                             PRB_ERR_ARG, table untouched: a feature outside the annotation, an identifier below 0, an
 *                             (identifier, feature) given twice in the call, an identifier merged by an earlier call -
 *                             every identifier of a call is marked as merged, so all the records of one identifier come
 *                             in one call.  n = 0 does nothing
 *   prb_featrank_merge        two unfinished tables into one, on the device, under the contract of prb_targetset_merge:
 *                             src may live on another device; both have the same n and the same number of features,
 *                             hold the same distinct_sites and chain_sites unless one is empty, and no identifier is
 *                             merged into both: anything else returns PRB_ERR_ARG and leaves both tables as they were.
 *                             dst then holds - bit for bit - the table of all that was merged into either, and the sums
 *                             of their stage counts and unassigned hits; src is left empty but valid
 *   prb_featrank_finish       the filled slots compacted on the device (a scan over the fills, a gather in rank order)
 *                             and copied to the host in one copy; the device memory is released.  prb_featrank_records
 *                             then returns the records by feature index ascending, then rank; `rank` counts from 0
 *                             within the feature.  Nothing can be merged after it (a second call does nothing)
 *   prb_featrank_counts       the stage counts of prb_featset_counts, summed over the feature tables merged
 *   prb_featrank_unassigned   the unassigned hits of prb_featset_unassigned, summed likewise
 * A merge does work in proportion to the feature table's records: their features as sort keys, a stable sort by feature,
 * the rank keys (the monotone 64-bit key of e_min, the identifier) and the heads of the features' runs, and a wavefront
 * per run that merges it into the feature's ranked list in LDS - the lists, the merge and the gather of the per-target
 * table.  No floating-point atomics, and nothing depends on the order in which threads arrive.  On the device every kernel
 * checks feature, query and identifier against the tables' ranges again; a violation raises the table's `bad` flag and
 * writes nothing, and this and every later call on the table returns PRB_ERR_STATE.  A merge that fails part way leaves
 * the table unusable.  Stage timer "featrank": prb_featrank_add_featset (launches = 5: sort keys, sort, rank keys and
 * heads, selection of the heads, merge; none when fs holds no record), prb_featrank_add_records (5; none for n = 0),
 * prb_featrank_merge (1); the launches booked to "feature" are those of the feature table's own calls, as ever. */
typedef struct prb_featrank prb_featrank;
int prb_featrank_create(prb_ctx *ctx, const prb_annot *an, int32_t n, prb_featrank **out);
int prb_featrank_add_featset(prb_ctx *ctx, prb_featrank *fr, const prb_featset *fs, const int32_t *query_ids);
int prb_featrank_add_records(prb_ctx *ctx, prb_featrank *fr, const prb_featrank_pair *recs, int64_t n);
int prb_featrank_merge(prb_ctx *ctx, prb_featrank *dst, prb_featrank *src);
int prb_featrank_finish(prb_ctx *ctx, prb_featrank *fr);
int64_t prb_featrank_size(const prb_featrank *fr);
const prb_featrank_pair *prb_featrank_records(const prb_featrank *fr);
void prb_featrank_counts(const prb_featrank *fr, int64_t counts[3]);
int64_t prb_featrank_unassigned(const prb_featrank *fr);
void prb_featrank_free(prb_featrank *fr);
/* The lines of `ris -t -A FILE -B N`: recs[0, nrecs) as prb_featrank_records returns them (by feature, then rank), one
 * line each in that order, numbered from id0 on; every line is the prb_write_feature_lines line of its record's f.
 * qnames and qlen_unmasked are indexed by the query's identifier (nq_total of them: every f.s.query lies below it); the
 * other arguments and the results as prb_write_feature_lines. */
int prb_write_featrank_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                             const prb_featrank_pair *recs, int64_t nrecs, const char *const *feat_names, const int32_t *feat_start,
                             const int32_t *feat_end, int64_t nfeat, int64_t id0, int fd, int64_t *nlines, int64_t *nbytes);

/* ---- output: SaveMyResults (rna_interaction_search.cpp:322-369) ----
 * The result lines of one batch of queries, grouped query by query and page by page and numbered
 * from id0 on (the `Id` column; MergeOutput, rna_interaction_search.cpp:464-476), written to the file
 * descriptor `fd` (fd < 0: formatted and counted only).  pages[p] = the hits of the batch against
 * page p with their pair array, as prb_hitset_hits / prb_hitset_basepairs return them (or as they
 * arrived from another rank); hits ascending by `query`.  Host threads format in parallel. */
typedef struct prb_page_hits {
  const prb_hit *hits;
  int64_t nhits;
  const int32_t *basepairs; /* int32[2 * npairs] */
  int64_t npairs;
} prb_page_hits;
int prb_write_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                    const prb_page_hits *pages, int32_t npages, int32_t output_style, int64_t id0, int fd,
                    int64_t *lines, int64_t *bytes);
/* The summary lines of one batch (`ris -t`), grouped and numbered as prb_write_lines groups and numbers result lines:
 *   Id,qname,qlen,dbname,dblen,Hits,MinEnergy,SumEnergy,Eacc,Ehyb,(q0-qN:db0-dbN)
 * energies in the result lines' form, the base-pair field the best hit's `-s 0` field.  pages[p] = the records of the
 * batch against page p as prb_pairset_pairs returns them (ascending by `query`). */
typedef struct prb_page_pairs {
  const prb_pair_summary *pairs;
  int64_t npairs;
} prb_page_pairs;
int prb_write_summary_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_page_pairs *pages, int32_t npages, int64_t id0, int fd, int64_t *lines,
                            int64_t *bytes);
/* The lines of `ris -t -n N` for one batch: pairs[0, n) as prb_topset_pairs returns them (ascending by query, then by
 * rank), one line each in that order, numbered from id0 on; every line is the `-t` line of its pair. */
int prb_write_top_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                        const prb_top_pair *pairs, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes);
/* The lines of `ris -r N`: pairs[0, n) as prb_targetset_pairs returns them (by page, then db_id, then rank), one line
 * each in that order, numbered from id0 on; every line is the `-t` line of its pair.  qnames and qlen_unmasked are indexed
 * by the query's identifier (nq_total of them: every s.query lies below it). */
int prb_write_target_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                           const prb_target_pair *pairs, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes);
/* The lines of `ris -q` for one batch: rows[0, n) as prb_profset_rows returns them (ascending by query, then by
 * position), one line each in that order, numbered from id0 on:
 *   Id,qname,qlen,Position,Hits,Targets,MinEnergy,dbname,dblen,(q0-qN:db0-dbN)
 * qlen is the result lines' Query Length (the unmasked bases: with repeat masking a position can exceed it), the
 * energy in the result lines' form, the last three fields those of the best hit's result line in the `-s 0` form. */
int prb_write_profile_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_profile_pos *rows, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes);
/* The lines of `ris -c D`: regions[0, n) as prb_covset_regions returns them (by page, then db_id, then start), one line
 * each in that order, numbered from id0 on:
 *   Id,dbname,dblen,Start,End,Hits,MaxHits,MaxQueries,Peak,MinEnergy,qname,qlen,(q0-qN:db0-dbN)
 * the energy and the best hit's base-pair field in the result lines' form.  qnames and qlen_unmasked are indexed by the
 * query's identifier (nq_total of them: every `query` lies below it). */
int prb_write_region_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                           const prb_target_region *regions, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes);
/* The lines of `ris -t -z N` for one batch: recs[0, n) as prb_nullset_pairs returns them (by query, then page, then
 * db_id), one line each in that order, numbered from id0 on: the `-t` line of the observed pair, and behind it
 *   ,Decoys,NullHits,NullLE,NullMin,PValue
 * NullMin in the result lines' energy form, or NA when NullHits is 0; PValue = (NullLE + 1) / (Decoys + 1) in double,
 * printed as %.6g. */
int prb_write_null_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_null_pair *recs,
                         int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes);
/* The lines of `ris -t -z N -Q` for one batch: the lines of prb_write_null_lines for recs[0, n), and behind each one the
 * figures of fdr[0, n) (prb_nullset_fdr, parallel to recs):
 *   ,Tests,Rank,QValue
 * QValue = 1 for the triple (0, 0, 0), else (Tests * q_num) / (q_den * q_rank): two exact doubles, one division, printed
 * as %.6g like PValue.  PRB_ERR_ARG for a figure with tests or rank below 1, or whose triple is neither (0, 0, 0) nor
 * three positive numbers. */
int prb_write_null_fdr_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                             const prb_null_pair *recs, const prb_null_fdr *fdr, int64_t n, int64_t id0, int fd, int64_t *lines,
                             int64_t *bytes);

/* ---- multi-GPU: one process per GPU, the final hit gather over RCCL (xGMI) ----
 * Replaces MergeOutput's MPI token ring (rna_interaction_search.cpp:426-487) and, with the caller
 * dealing batches to ranks, the area / dynamic schedulers (rna_interaction_search.cpp:143-160,
 * 202-230).  Queries are independent end to end: this gather is the only exchange of the `ris` step.
 *   rank 0: prb_comm_unique_id(id); the 128 bytes reach the other ranks by any side channel (a file,
 *   torch.distributed, MPI ...); every rank: prb_comm_create(ctx, nranks, rank, id, &comm).
 * From then on the final hit sets of `ctx` also keep their packed records in HBM, and
 * prb_gather_hits - a collective, called by every rank once per (batch round, database page) -
 * moves them device to device: on `root`, *out is a new hit set with the hits of all ranks in rank
 * order, `query` shifted by the number of queries of the lower ranks and pair offsets rebased;
 * prb_hitset_gathered_queries gives every rank's batch size and the unmasked lengths of all the
 * queries in the same order.  Elsewhere *out = NULL.  A rank without a batch in this round passes mine = NULL,
 * nq = 0.  The gathered hit set borrows a pinned buffer of the communicator until it is
 * freed with prb_hitset_free (from any thread; the buffer outlives prb_comm_destroy if it has to).  The gather works on a stream of
 * its own, so one host thread may gather (and print) batch k while another one searches batch k + 1 on the
 * context - as long as every rank issues its gathers in the same order. */
typedef struct prb_comm prb_comm;
#define PRB_COMM_ID_BYTES 128
int prb_comm_unique_id(char id[PRB_COMM_ID_BYTES]);
int prb_comm_create(prb_ctx *ctx, int32_t nranks, int32_t rank, const char id[PRB_COMM_ID_BYTES], prb_comm **out);
void prb_comm_destroy(prb_comm *comm);
int prb_gather_hits(prb_comm *comm, const prb_hitset *mine, int32_t nq, const int32_t *qlen_unmasked, int32_t root,
                    prb_hitset **out);
int prb_hitset_gathered_queries(const prb_hitset *hs, int32_t *nranks, const int32_t **nq_of_rank,
                                const int32_t **qlen_unmasked);
/* The placement rule of prb_gather_hits as a pure host function (no GPU, no communicator): counts[3 * k + {0, 1, 2}] =
 * hits, pair-array ints and queries rank k brings; bases[3 * k + j] = where rank k's share of kind j starts in the
 * gathered arrays (k = 0 .. nranks; entry nranks = the totals).  The root receives rank k's records at bases[3k],
 * adds bases[3k + 2] to their `query` and bases[3k + 1] / 2 to their `bp_offset`.  This is what replaces the order
 * in which the reference's ranks append their temporary files (rna_interaction_search.cpp:426-487). */
int prb_gather_plan(int32_t nranks, const int64_t *counts /* 3 * nranks */, int64_t *bases /* 3 * (nranks + 1) */);
/* keep (on != 0) the packed records of later final hit sets in HBM without a communicator (tests) */
void prb_ctx_keep_device_records(prb_ctx *ctx, int32_t on);

#ifdef __cplusplus
}
#endif
#endif
