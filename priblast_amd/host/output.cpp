// Result lines of `ris` (SaveMyResults, rna_interaction_search.cpp:322-369).  See output.hpp.
#include "output.hpp"

#include "cpu_budget.hpp"

#include <unistd.h>

#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace prb {

int format_threads() {
  // (its own knob first: with one process per GPU only rank 0 writes lines - for all ranks - while every rank runs a seed DFS)
  if (const char *e = std::getenv("PRB_FORMAT_THREADS")) return std::max(1, std::atoi(e));
  if (const char *e = std::getenv("PRB_HOST_THREADS")) return std::max(1, std::atoi(e));
  return default_host_threads();
}

namespace {

// A piece of one query's hits against one page: hits [i0, i1), the first of them numbered id.
struct Piece {
  uint32_t q, p;
  int64_t i0, i1, id;
};
constexpr int64_t kPieceLines = 8192;

// Text buffer that grows by doubling; the formatters write through raw pointers.
struct Buf {
  std::vector<char> v;
  size_t n = 0;
  char *room(size_t want) {
    if (n + want > v.size()) v.resize(std::max(v.size() * 2, n + want + 4096));
    return v.data() + n;
  }
};

inline char *put_int(char *p, long long x) { return std::to_chars(p, p + 24, x).ptr; }
// `ostream << double` with the default precision = printf("%g"): std::to_chars in the general
// format with precision 6 is specified as exactly that conversion (tests/test_host.py compares).
inline char *put_g(char *p, double x) { return std::to_chars(p, p + 40, x, std::chars_format::general, 6).ptr; }

// reversed page text -> forward coordinate of sequence `id` (:352-363)
inline int32_t fwd_pos(const SeqTable &tab, int32_t id, int32_t dbpos) { return (tab.len[id] - 1) - (dbpos - tab.start_pos[id]); }

// `-s 0` base-pair field "(q0-qN:db0-dbN) " from the first and the last pair of a hit
inline char *put_ends(char *p, const SeqTable &tab, int32_t id, const int32_t first[2], const int32_t last[2]) {
  *p++ = '(';
  p = put_int(p, first[0]);
  *p++ = '-';
  p = put_int(p, last[0]);
  *p++ = ':';
  p = put_int(p, fwd_pos(tab, id, first[1]));
  *p++ = '-';
  p = put_int(p, fwd_pos(tab, id, last[1]));
  *p++ = ')';
  *p++ = ' ';
  return p;
}

// "Id,qname,qlen,dbname,dblen," - the columns every line starts with
inline char *put_names(char *p, int64_t id, const std::string &qname, int32_t qlen, const SeqTable &tab, int32_t db_id) {
  const std::string &dname = tab.names[db_id];
  p = put_int(p, id);
  *p++ = ',';
  std::memcpy(p, qname.data(), qname.size());
  p += qname.size();
  *p++ = ',';
  p = put_int(p, qlen);
  *p++ = ',';
  std::memcpy(p, dname.data(), dname.size());
  p += dname.size();
  *p++ = ',';
  p = put_int(p, tab.len_unmasked[db_id]);
  *p++ = ',';
  return p;
}

// in place of a line's newline: ,Decoys,NullLE,Rank,EValue,QValue and the newline (`ris -k N -E M`)
void put_eval_columns(Buf &b, const prb_eval_score &x) {
  b.n--; // (the newline)
  char *p = b.room(200);
  char *const p0 = p;
  for (long long f : {(long long)x.decoys, (long long)x.null_le, (long long)x.rank}) {
    *p++ = ',';
    p = put_int(p, f);
  }
  *p++ = ',';
  p = put_g(p, (double)x.null_le / (double)x.decoys);
  *p++ = ',';
  p = put_g(p, (double)x.q_num / ((double)x.decoys * (double)x.q_den));
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

// scores (may be null): per page, the score of every hit, printed behind its line
void format_piece(const Piece &pc, const BatchView &v, const std::vector<SeqTable> &tabs, int output_style, Buf &b,
                  const std::vector<const prb_eval_score *> *scores = nullptr) {
  const PageHits &ph = v.pages[pc.p];
  const SeqTable &tab = tabs[pc.p];
  const std::string &qname = v.names[pc.q];
  const int32_t qlen = v.qlen_unmasked[pc.q];
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_hit &x = ph.h[i];
    const int32_t npairs = output_style == 1 ? x.bp_count : (x.bp_count > 0 ? 1 : 0);
    char *p = b.room(qname.size() + tab.names[x.db_id].size() + 200 + (size_t)npairs * 48);
    char *const p0 = p;
    p = put_names(p, id++, qname, qlen, tab, x.db_id);
    p = put_g(p, x.e_acc);
    *p++ = ',';
    p = put_g(p, x.e_hyb);
    *p++ = ',';
    p = put_g(p, x.e_tot);
    *p++ = ',';
    const int32_t *pp = ph.bp + 2 * x.bp_offset;
    if (output_style == 1) {
      for (int32_t j = 0; j < x.bp_count; j++) {
        *p++ = '(';
        p = put_int(p, pp[2 * j]);
        *p++ = ':';
        p = put_int(p, fwd_pos(tab, x.db_id, pp[2 * j + 1]));
        *p++ = ')';
        *p++ = ' ';
      }
    } else if (x.bp_count > 0) {
      p = put_ends(p, tab, x.db_id, pp, pp + 2 * (x.bp_count - 1));
    }
    *p++ = '\n';
    b.n += (size_t)(p - p0);
    if (scores) put_eval_columns(b, (*scores)[pc.p][i]);
  }
}

bool write_all(int fd, const char *p, size_t n) {
  while (n) {
    const ssize_t k = ::write(fd, p, n);
    if (k < 0) return false;
    p += k;
    n -= (size_t)k;
  }
  return true;
}

// rounds of pieces: formatted in parallel, then written in order; false when a write failed
template <class Fmt> bool write_pieces(const std::vector<Piece> &pieces, Fmt fmt, LineSink &sink, int threads) {
  const size_t per_round = (size_t)std::max(1, threads) * 4;
  std::vector<Buf> bufs(std::min(per_round, std::max<size_t>(pieces.size(), 1)));
  bool ok = true;
  for (size_t r0 = 0; r0 < pieces.size() && ok; r0 += per_round) {
    const size_t r1 = std::min(pieces.size(), r0 + per_round);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, threads))
    for (size_t k = r0; k < r1; k++) {
      Buf &b = bufs[k - r0];
      b.n = 0;
      fmt(pieces[k], b);
    }
    for (size_t k = r0; k < r1 && ok; k++) {
      const Buf &b = bufs[k - r0];
      if (sink.fd >= 0 && b.n) ok = write_all(sink.fd, b.v.data(), b.n);
      sink.bytes += (int64_t)b.n;
      sink.lines += pieces[k].i1 - pieces[k].i0;
    }
  }
  return ok;
}

// Records of one batch (per page, ascending by query) as lines, query by query and page by page, numbered from id0 on:
// n_of(p) = records of page p, query_of(p, i) = the query of record i, fmt(piece, buf) formats a piece.
template <class NOf, class QueryOf, class Fmt>
int64_t format_records(size_t nq, size_t np, NOf n_of, QueryOf query_of, Fmt fmt, int64_t id0, LineSink &sink, int threads) {
  std::vector<std::vector<int64_t>> first(np, std::vector<int64_t>(nq + 1, 0)); // first[p][q] = first record of query q
  for (size_t p = 0; p < np; p++) {
    const int64_t n = n_of(p);
    size_t q = 0;
    for (int64_t i = 0; i < n; i++)
      while (q < nq && (int64_t)q <= query_of(p, i)) first[p][q++] = i;
    while (q <= nq) first[p][q++] = n;
  }
  std::vector<Piece> pieces;
  int64_t id = id0;
  for (size_t q = 0; q < nq; q++)
    for (size_t p = 0; p < np; p++)
      for (int64_t i = first[p][q]; i < first[p][q + 1]; i += kPieceLines) {
        const int64_t e = std::min(first[p][q + 1], i + kPieceLines);
        pieces.push_back(Piece{(uint32_t)q, (uint32_t)p, i, e, id});
        id += e - i;
      }
  return write_pieces(pieces, fmt, sink, threads) ? id : -1;
}

// one summary line (`ris -t`) of pair x, found in the page whose table is `tab`
void put_summary_line(Buf &b, int64_t id, const std::string &qname, int32_t qlen, const SeqTable &tab, const prb_pair_summary &x) {
  char *p = b.room(qname.size() + tab.names[x.db_id].size() + 320);
  char *const p0 = p;
  p = put_names(p, id, qname, qlen, tab, x.db_id);
  p = put_int(p, x.hits);
  *p++ = ',';
  p = put_g(p, x.e_min);
  *p++ = ',';
  p = put_g(p, x.e_sum);
  *p++ = ',';
  p = put_g(p, x.e_acc);
  *p++ = ',';
  p = put_g(p, x.e_hyb);
  *p++ = ',';
  p = put_ends(p, tab, x.db_id, x.bp_first, x.bp_last);
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

void format_summary_piece(const Piece &pc, const SummaryView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  const PagePairs &pp = v.pages[pc.p];
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) put_summary_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs[pc.p], pp.r[i]);
}

void format_top_piece(const Piece &pc, const TopView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++)
    put_summary_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs[v.r[i].page], v.r[i].s);
}

void format_target_piece(const Piece &pc, const TargetView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++)
    put_summary_line(b, id++, v.names[v.r[i].s.query], v.qlen_unmasked[v.r[i].s.query], tabs[v.r[i].page], v.r[i].s);
}

// in place of a line's newline: the null columns and the newline
void put_null_columns(Buf &b, int32_t decoys, int64_t null_hits, int64_t null_le, double null_min) {
  b.n--; // (the newline)
  char *p = b.room(200);
  char *const p0 = p;
  for (long long f : {(long long)decoys, (long long)null_hits, (long long)null_le}) {
    *p++ = ',';
    p = put_int(p, f);
  }
  *p++ = ',';
  if (null_hits > 0) {
    p = put_g(p, null_min);
  } else {
    *p++ = 'N';
    *p++ = 'A';
  }
  *p++ = ',';
  p = put_g(p, ((double)null_le + 1.0) / ((double)decoys + 1.0));
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

// the `-t` line of the observed pair, then the null columns
void format_null_piece(const Piece &pc, const NullView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_null_pair &x = v.r[i];
    put_summary_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs[x.page], x.s);
    put_null_columns(b, x.decoys, x.null_hits, x.null_le, x.null_min);
  }
}

// in place of a line's newline: the Benjamini-Hochberg columns and the newline
void put_fdr_columns(Buf &b, const prb_null_fdr &x) {
  b.n--; // (the newline)
  char *p = b.room(120);
  char *const p0 = p;
  for (long long f : {(long long)x.tests, (long long)x.rank}) {
    *p++ = ',';
    p = put_int(p, f);
  }
  *p++ = ',';
  // (both operands are integers below 2^53: one rounding, the division's)
  p = put_g(p, x.q_den == 0 ? 1.0 : (double)((uint64_t)x.tests * x.q_num) / (double)((uint64_t)x.q_den * x.q_rank));
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

// the `-z` line, then the Benjamini-Hochberg columns
void format_null_fdr_piece(const Piece &pc, const NullFdrView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_null_pair &x = v.r[i];
    put_summary_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs[x.page], x.s);
    put_null_columns(b, x.decoys, x.null_hits, x.null_le, x.null_min);
    put_fdr_columns(b, v.f[i]);
  }
}

// the `-t` line of the group's best member x, then - in place of its newline - the group columns
void put_group_line(Buf &b, int64_t id, const std::string &qname, int32_t qlen, const std::vector<SeqTable> &tabs, const prb_group_pair &x,
                    const char *const *group_names, const int32_t *group_sizes) {
  put_summary_line(b, id, qname, qlen, tabs[x.page], x.s);
  b.n--; // (the newline)
  const size_t len = std::strlen(group_names[x.group]);
  char *p = b.room(len + 100);
  char *const p0 = p;
  *p++ = ',';
  std::memcpy(p, group_names[x.group], len);
  p += len;
  for (long long f : {(long long)x.members, (long long)group_sizes[x.group], (long long)x.hits}) {
    *p++ = ',';
    p = put_int(p, f);
  }
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

void format_group_piece(const Piece &pc, const GroupView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) put_group_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs, v.r[i], v.group_names, v.group_sizes);
}

// the `-t` line of the record's s, then - in place of its newline - the feature columns
void put_feature_line(Buf &b, int64_t id, const std::string &qname, int32_t qlen, const std::vector<SeqTable> &tabs, const prb_feature_pair &x,
                      const char *const *feat_names, const int32_t *feat_start, const int32_t *feat_end) {
  put_summary_line(b, id, qname, qlen, tabs[x.page], x.s);
  b.n--; // (the newline)
  const size_t len = std::strlen(feat_names[x.feature]);
  char *p = b.room(len + 100);
  char *const p0 = p;
  *p++ = ',';
  std::memcpy(p, feat_names[x.feature], len);
  p += len;
  *p++ = ',';
  p = put_int(p, (long long)feat_start[x.feature]);
  *p++ = '-';
  p = put_int(p, (long long)feat_end[x.feature]);
  *p++ = ',';
  p = put_int(p, (long long)x.inside);
  *p++ = '\n';
  b.n += (size_t)(p - p0);
}

void format_feature_piece(const Piece &pc, const FeatureView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++)
    put_feature_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs, v.r[i], v.feat_names, v.feat_start, v.feat_end);
}

// the feature line, then the null columns
void format_fnull_piece(const Piece &pc, const FNullView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_fnull_pair &x = v.r[i];
    put_feature_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs, x.f, v.feat_names, v.feat_start, v.feat_end);
    put_null_columns(b, x.decoys, x.null_hits, x.null_le, x.null_min);
  }
}

// ... of records that are not grouped by query: s.query is the query's identifier
void format_grouprank_piece(const Piece &pc, const GroupView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++)
    put_group_line(b, id++, v.names[v.r[i].s.query], v.qlen_unmasked[v.r[i].s.query], tabs, v.r[i], v.group_names, v.group_sizes);
}

// the feature line of records that are not grouped by query: f.s.query is the query's identifier
void format_featrank_piece(const Piece &pc, const FeatRankView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++)
    put_feature_line(b, id++, v.names[v.r[i].f.s.query], v.qlen_unmasked[v.r[i].f.s.query], tabs, v.r[i].f, v.feat_names, v.feat_start, v.feat_end);
}

// the group line, then the null columns
void format_gnull_piece(const Piece &pc, const GNullView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_gnull_pair &x = v.r[i];
    put_group_line(b, id++, v.names[pc.q], v.qlen_unmasked[pc.q], tabs, x.g, v.group_names, v.group_sizes);
    put_null_columns(b, x.decoys, x.null_hits, x.null_le, x.null_min);
  }
}

void format_profile_piece(const Piece &pc, const ProfileView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  const std::string &qname = v.names[pc.q];
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_profile_pos &x = v.r[i];
    const SeqTable &tab = tabs[x.page];
    const std::string &dname = tab.names[x.db_id];
    char *p = b.room(qname.size() + dname.size() + 240);
    char *const p0 = p;
    p = put_int(p, id++);
    *p++ = ',';
    std::memcpy(p, qname.data(), qname.size());
    p += qname.size();
    *p++ = ',';
    p = put_int(p, v.qlen_unmasked[pc.q]);
    *p++ = ',';
    p = put_int(p, x.pos);
    *p++ = ',';
    p = put_int(p, x.hits);
    *p++ = ',';
    p = put_int(p, x.targets);
    *p++ = ',';
    p = put_g(p, x.e_min);
    *p++ = ',';
    std::memcpy(p, dname.data(), dname.size());
    p += dname.size();
    *p++ = ',';
    p = put_int(p, tab.len_unmasked[x.db_id]);
    *p++ = ',';
    p = put_ends(p, tab, x.db_id, x.bp_first, x.bp_last);
    *p++ = '\n';
    b.n += (size_t)(p - p0);
  }
}

void format_region_piece(const Piece &pc, const RegionView &v, const std::vector<SeqTable> &tabs, Buf &b) {
  int64_t id = pc.id;
  for (int64_t i = pc.i0; i < pc.i1; i++) {
    const prb_target_region &x = v.r[i];
    const SeqTable &tab = tabs[x.page];
    const std::string &dname = tab.names[x.db_id], &qname = v.names[x.query];
    char *p = b.room(qname.size() + dname.size() + 400);
    char *const p0 = p;
    p = put_int(p, id++);
    *p++ = ',';
    std::memcpy(p, dname.data(), dname.size());
    p += dname.size();
    *p++ = ',';
    p = put_int(p, tab.len_unmasked[x.db_id]);
    for (long long f : {(long long)x.start, (long long)x.end, (long long)x.hits, (long long)x.max_hits, (long long)x.max_queries, (long long)x.peak}) {
      *p++ = ',';
      p = put_int(p, f);
    }
    *p++ = ',';
    p = put_g(p, x.e_min);
    *p++ = ',';
    std::memcpy(p, qname.data(), qname.size());
    p += qname.size();
    *p++ = ',';
    p = put_int(p, v.qlen_unmasked[x.query]);
    *p++ = ',';
    p = put_ends(p, tab, x.db_id, x.bp_first, x.bp_last);
    *p++ = '\n';
    b.n += (size_t)(p - p0);
  }
}

} // namespace

int64_t format_batch(const BatchView &v, const std::vector<SeqTable> &tabs, int output_style, int64_t id0, LineSink &sink,
                     int threads) {
  return format_records(
      v.nq, v.pages.size(), [&](size_t p) { return v.pages[p].n; }, [&](size_t p, int64_t i) { return v.pages[p].h[i].query; },
      [&](const Piece &pc, Buf &b) { format_piece(pc, v, tabs, output_style, b); }, id0, sink, threads);
}

int64_t format_scored_batch(const ScoredView &v, const std::vector<SeqTable> &tabs, int output_style, int64_t id0, LineSink &sink,
                            int threads) {
  return format_records(
      v.nq, v.pages.size(), [&](size_t p) { return v.pages[p].n; }, [&](size_t p, int64_t i) { return v.pages[p].h[i].query; },
      [&](const Piece &pc, Buf &b) { format_piece(pc, v, tabs, output_style, b, &v.scores); }, id0, sink, threads);
}

int64_t format_summary_batch(const SummaryView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  return format_records(
      v.nq, v.pages.size(), [&](size_t p) { return v.pages[p].n; }, [&](size_t p, int64_t i) { return v.pages[p].r[i].query; },
      [&](const Piece &pc, Buf &b) { format_summary_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_profile_batch(const ProfileView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page": the rows are in output order already, and each carries its best hit's page)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].query; },
      [&](const Piece &pc, Buf &b) { format_profile_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_top_batch(const TopView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page": the records are in output order already, and each carries its own)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].s.query; },
      [&](const Piece &pc, Buf &b) { format_top_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_null_batch(const NullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the top-N records: in output order already, each with its own page)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].s.query; },
      [&](const Piece &pc, Buf &b) { format_null_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_null_fdr_batch(const NullFdrView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the null records)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].s.query; },
      [&](const Piece &pc, Buf &b) { format_null_fdr_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_group_batch(const GroupView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the top-N records: in output order already, each with its own page)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].s.query; },
      [&](const Piece &pc, Buf &b) { format_group_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_feature_batch(const FeatureView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the top-N records: in output order already, each with its own page)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].s.query; },
      [&](const Piece &pc, Buf &b) { format_feature_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_fnull_batch(const FNullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the feature records)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].f.s.query; },
      [&](const Piece &pc, Buf &b) { format_fnull_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_gnull_batch(const GNullView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (one "page", as for the group records)
  return format_records(
      v.nq, 1, [&](size_t) { return v.n; }, [&](size_t, int64_t i) { return v.r[i].g.s.query; },
      [&](const Piece &pc, Buf &b) { format_gnull_piece(pc, v, tabs, b); }, id0, sink, threads);
}

int64_t format_target_batch(const TargetView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (the records are in output order, and not grouped by query: pieces of consecutive records)
  std::vector<Piece> pieces;
  for (int64_t i = 0; i < v.n; i += kPieceLines) pieces.push_back(Piece{0, 0, i, std::min(v.n, i + kPieceLines), id0 + i});
  return write_pieces(pieces, [&](const Piece &pc, Buf &b) { format_target_piece(pc, v, tabs, b); }, sink, threads) ? id0 + v.n : -1;
}

int64_t format_grouprank_batch(const GroupView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (as the per-target records: in output order, not grouped by query)
  std::vector<Piece> pieces;
  for (int64_t i = 0; i < v.n; i += kPieceLines) pieces.push_back(Piece{0, 0, i, std::min(v.n, i + kPieceLines), id0 + i});
  return write_pieces(pieces, [&](const Piece &pc, Buf &b) { format_grouprank_piece(pc, v, tabs, b); }, sink, threads) ? id0 + v.n : -1;
}

int64_t format_featrank_batch(const FeatRankView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (as the per-target records: in output order, not grouped by query)
  std::vector<Piece> pieces;
  for (int64_t i = 0; i < v.n; i += kPieceLines) pieces.push_back(Piece{0, 0, i, std::min(v.n, i + kPieceLines), id0 + i});
  return write_pieces(pieces, [&](const Piece &pc, Buf &b) { format_featrank_piece(pc, v, tabs, b); }, sink, threads) ? id0 + v.n : -1;
}

int64_t format_region_batch(const RegionView &v, const std::vector<SeqTable> &tabs, int64_t id0, LineSink &sink, int threads) {
  // (as the per-target records: in output order, not grouped by query)
  std::vector<Piece> pieces;
  for (int64_t i = 0; i < v.n; i += kPieceLines) pieces.push_back(Piece{0, 0, i, std::min(v.n, i + kPieceLines), id0 + i});
  return write_pieces(pieces, [&](const Piece &pc, Buf &b) { format_region_piece(pc, v, tabs, b); }, sink, threads) ? id0 + v.n : -1;
}

} // namespace prb
