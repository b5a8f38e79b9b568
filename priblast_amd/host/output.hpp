// Result lines of `ris` (SaveMyResults, rna_interaction_search.cpp:322-369): one text line per hit,
//   Id,qname,qlen,dbname,dblen,Eacc,Ehyb,Etotal,(q0-qN:db0-dbN)          -s 0
//   Id,qname,qlen,dbname,dblen,Eacc,Ehyb,Etotal,(q:db) (q:db) ...        -s 1
// doubles as `ostream << double` prints them (6 significant digits, "%g"), database coordinates
// turned from the reversed page text back into forward sequence coordinates (:352-363).
// Shared by the library (prb_write_lines) and the command line (`ris`, `txt`).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/priblast_hip.h"

namespace prb {

// What the output needs to know about the sequences of one database page.
struct SeqTable {
  std::vector<std::string> names;
  std::vector<int32_t> len, len_unmasked, start_pos;
};

// The hits of one batch against one page, and a batch: plain arrays, wherever they live (hit sets
// of the library, or a binary hit file read back).
struct PageHits {
  const prb_hit *h = nullptr;
  int64_t n = 0;
  const int32_t *bp = nullptr;
  int64_t nbp = 0; // pairs
};
// The queries of a batch, which every view of its results starts with.
struct QueryView {
  size_t nq = 0;
  const std::string *names = nullptr; // [nq]
  const int32_t *qlen_unmasked = nullptr;
};
struct BatchView : QueryView {
  std::vector<PageHits> pages;
};

struct LineSink {
  int fd = -1; // -1: the lines are formatted and counted, not written
  int64_t lines = 0, bytes = 0;
};

// Lines of one batch, query by query and page by page as the reference groups them, numbered from
// `id0` on; returns the next id, or -1 when a write failed.  The hits of a page arrive grouped by
// query in ascending order, so a query's hits are one contiguous range per page; ranges are cut
// into pieces that host threads format in parallel.
int64_t format_batch(const BatchView &v, const std::vector<SeqTable> &tabs, int output_style, int64_t id0, LineSink &sink,
                     int threads);

// Lines of `ris -k N -E M`: the lines of format_batch, and behind each one the five columns of its hit's score
// (prb_evalset_score; scores[p][i] belongs to pages[p].h[i]):
//   ... ,Decoys,NullLE,Rank,EValue,QValue
// EValue = NullLE / Decoys and QValue = q_num / (Decoys * q_den), in double, six significant digits.
struct ScoredView : BatchView {
  std::vector<const prb_eval_score *> scores;
};
int64_t format_scored_batch(const ScoredView &v, const std::vector<SeqTable> &tabs, int output_style, int64_t id0, LineSink &sink,
                            int threads);

// Summary lines of `ris -t` (one per query-target pair, prb_search_page_summary), grouped and numbered the same way:
//   Id,qname,qlen,dbname,dblen,Hits,MinE,SumE,Eacc,Ehyb,(q0-qN:db0-dbN)
// energies and the best hit's base-pair field formatted exactly as in the result lines (-s 0 form).
struct PagePairs {
  const prb_pair_summary *r = nullptr;
  int64_t n = 0;
};
struct SummaryView : QueryView {
  std::vector<PagePairs> pages;
};
int64_t format_summary_batch(const SummaryView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -t -n N` (prb_topset_pairs): the same lines, for ranked records that carry their page, in the records'
// order (ascending by query, then by rank), numbered from id0 on.
struct TopView : QueryView {
  const prb_top_pair *r = nullptr;
  int64_t n = 0;
};
int64_t format_top_batch(const TopView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -t -z N` (prb_nullset_pairs): the `-t` line of every observed pair with the null columns behind it, in
// the records' order (by query, then page, then db_id), numbered from id0 on:
//   Id,qname,qlen,dbname,dblen,Hits,MinE,SumE,Eacc,Ehyb,(q0-qN:db0-dbN) ,Decoys,NullHits,NullLE,NullMin,PValue
// NullMin in the energies' form, or NA when no decoy has a hit; PValue = (NullLE + 1) / (Decoys + 1), six significant digits.
struct NullView : QueryView {
  const prb_null_pair *r = nullptr;
  int64_t n = 0;
};
int64_t format_null_batch(const NullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);
// Lines of `ris -t -z N -Q` (prb_nullset_pairs with prb_nullset_fdr beside them): the `-z` line of every record, and
// behind it the Benjamini-Hochberg figures of its pair:
//   ... ,Decoys,NullHits,NullLE,NullMin,PValue ,Tests,Rank,QValue
// Tests = the hypotheses of the query, Rank = the query's pairs whose p-value is not above the line's, QValue = 1 for the
// triple (0, 0, 0), else (Tests * q_num) / (q_den * q_rank) - two integers that are exact in double, one division -, six
// significant digits like PValue.
struct NullFdrView : NullView {
  const prb_null_fdr *f = nullptr; // [n], parallel to r
};
int64_t format_null_fdr_batch(const NullFdrView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -t -G FILE` (prb_groupset_pairs): the `-t` line of every group's best member with the group columns behind
// it, in the records' order (by query, then group or rank), numbered from id0 on:
//   Id,qname,qlen,dbname,dblen,Hits,MinE,SumE,Eacc,Ehyb,(q0-qN:db0-dbN) ,Group,Members,GroupSize,GroupHits
// group_names / group_sizes are indexed by the records' group.
struct GroupView : QueryView {
  const prb_group_pair *r = nullptr;
  int64_t n = 0;
  const char *const *group_names = nullptr;
  const int32_t *group_sizes = nullptr;
};
int64_t format_group_batch(const GroupView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);
// Lines of `ris -t -A FILE` (prb_featset_records): the `-t` line of every record's s with the feature columns behind it, in
// the records' order, numbered from id0 on:
//   Id,qname,qlen,dbname,dblen,Hits,MinE,SumE,Eacc,Ehyb,(q0-qN:db0-dbN) ,Feature,Start-End,Inside
// feat_names / feat_start / feat_end are indexed by the records' feature.
struct FeatureView : QueryView {
  const prb_feature_pair *r = nullptr;
  int64_t n = 0;
  const char *const *feat_names = nullptr;
  const int32_t *feat_start = nullptr, *feat_end = nullptr;
};
int64_t format_feature_batch(const FeatureView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);
// Lines of `ris -t -A FILE -F N` (prb_fnullset_records): the line of `-t -A` for every kept record, in the records' order,
// with the null columns of `-t -z` behind it:
//   ... ,Feature,Start-End,Inside ,Decoys,NullHits,NullLE,NullMin,PValue
struct FNullView : QueryView {
  const prb_fnull_pair *r = nullptr;
  int64_t n = 0;
  const char *const *feat_names = nullptr;
  const int32_t *feat_start = nullptr, *feat_end = nullptr;
};
int64_t format_fnull_batch(const FNullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);
// Lines of `ris -t -G FILE -R N` (prb_grouprank_pairs): the same line for every record, in the records' order (by group,
// then by rank - not grouped by query): names and qlen_unmasked are indexed by the records' s.query, an identifier.
int64_t format_grouprank_batch(const GroupView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -t -A FILE -B N` (prb_featrank_records): the `-t -A` line of every record's f, in the records' order (by
// feature, then by rank - not grouped by query): names and qlen_unmasked are indexed by the records' f.s.query, an identifier.
struct FeatRankView : QueryView {
  const prb_featrank_pair *r = nullptr;
  int64_t n = 0;
  const char *const *feat_names = nullptr;
  const int32_t *feat_start = nullptr, *feat_end = nullptr;
};
int64_t format_featrank_batch(const FeatRankView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -t -G FILE -P N` (prb_gnullset_pairs): the line of `-t -G` for every kept record, in the records' order,
// with the null columns of `-t -z` behind it:
//   ... ,Group,Members,GroupSize,GroupHits ,Decoys,NullHits,NullLE,NullMin,PValue
struct GNullView : QueryView {
  const prb_gnull_pair *r = nullptr;
  int64_t n = 0;
  const char *const *group_names = nullptr;
  const int32_t *group_sizes = nullptr;
};
int64_t format_gnull_batch(const GNullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -r N` (prb_targetset_pairs): the same lines again, in the records' order (by page, target and rank),
// numbered from id0 on.  The queries are those of the whole run: `names` and `qlen_unmasked` are indexed by the
// records' query identifiers.
struct TargetView : QueryView {
  const prb_target_pair *r = nullptr;
  int64_t n = 0;
};
int64_t format_target_batch(const TargetView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -q` (prb_profset_rows), one per covered query position, in the rows' order (ascending by query, then by
// position), numbered from id0 on:
//   Id,qname,qlen,Position,Hits,Targets,MinE,dbname,dblen,(q0-qN:db0-dbN)
// the energy and the best hit's base-pair field formatted as in the result lines (-s 0 form).
struct ProfileView : QueryView {
  const prb_profile_pos *r = nullptr;
  int64_t n = 0;
};
int64_t format_profile_batch(const ProfileView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

// Lines of `ris -c D` (prb_covset_regions), one per region, in the records' order (by page, db_id, start), numbered from
// id0 on; names / qlen_unmasked are indexed by the query's identifier:
//   Id,dbname,dblen,Start,End,Hits,MaxHits,MaxQueries,Peak,MinEnergy,qname,qlen,(q0-qN:db0-dbN)
struct RegionView : QueryView {
  const prb_target_region *r = nullptr;
  int64_t n = 0;
};
int64_t format_region_batch(const RegionView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads);

int format_threads(); // PRB_HOST_THREADS, else min(32, hardware threads)

} // namespace prb
