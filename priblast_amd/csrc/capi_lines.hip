// C ABI, part 5: result lines from records (prb_write_*_lines).  The records may come from another process - a
// gathered hit set, a file read back - so every one is checked before anything is indexed with it.
#include <string>
#include <vector>

#include "search_host.hpp"

using namespace prb;

namespace {
// The body the six writers share.  `View` is the formatter's view of a batch (output.hpp); `kind_ok` = the checks of
// the arguments only this kind has; `fill(v)` checks the records and puts them into the view (it sets the error text
// and returns the code when one is inconsistent); `format(v, sink)` is the formatter's call, returning the next id or -1.
template <class View, class Fill, class Format>
int write_lines(const char *fn, bool kind_ok, const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                int64_t *lines, int64_t *bytes, int fd, Fill &&fill, Format &&format) {
  if (!kind_ok || !db || nq < 0 || (nq && (!qnames || !qlen_unmasked))) {
    set_error(std::string(fn) + ": bad argument");
    return PRB_ERR_ARG;
  }
  try {
    View v;
    std::vector<std::string> names((size_t)nq);
    for (int32_t q = 0; q < nq; q++) names[q] = qnames[q];
    v.nq = (size_t)nq;
    v.names = names.data();
    v.qlen_unmasked = qlen_unmasked;
    if (int rc = fill(v)) return rc;
    LineSink sink;
    sink.fd = fd;
    const int64_t next = format(v, sink);
    if (lines) *lines = sink.lines;
    if (bytes) *bytes = sink.bytes;
    if (next < 0) {
      set_error(std::string(fn) + ": write failed");
      return PRB_ERR_IO;
    }
  } catch (const std::exception &e) {
    set_error(std::string(fn) + ": " + e.what());
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}
int bad_record(const std::string &msg) {
  set_error(msg);
  return PRB_ERR_ARG;
}
} // namespace

extern "C" {

int prb_write_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                    const prb_page_hits *pages, int32_t npages, int32_t output_style, int64_t id0, int fd, int64_t *lines,
                    int64_t *bytes) {
  const bool ok = db && pages && npages == (int32_t)db->pages.size() && output_style >= 0 && output_style <= 1;
  return write_lines<BatchView>(
      "prb_write_lines", ok, db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](BatchView &v) {
        for (int32_t p = 0; p < npages; p++) {
          const prb_page_hits &ph = pages[p];
          if (ph.nhits < 0 || ph.npairs < 0 || (ph.nhits && !ph.hits)) return bad_record("prb_write_lines: bad page");
          const int32_t nseq = db->pages[p].nseq;
          for (int64_t i = 0; i < ph.nhits; i++) {
            const prb_hit &x = ph.hits[i];
            if (x.query < 0 || x.query >= nq || x.db_id < 0 || x.db_id >= nseq || x.bp_count < 0 || x.bp_offset < 0 ||
                x.bp_offset + x.bp_count > ph.npairs || (i && x.query < ph.hits[i - 1].query))
              return bad_record("prb_write_lines: hit record " + std::to_string(i) + " of page " + std::to_string(p) + " is inconsistent");
          }
          v.pages.push_back(PageHits{ph.hits, ph.nhits, ph.basepairs, ph.npairs});
        }
        return (int)PRB_OK;
      },
      [&](const BatchView &v, LineSink &sink) { return format_batch(v, db->tabs, output_style, id0, sink, format_threads()); });
}

int prb_write_summary_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_page_pairs *pages, int32_t npages, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  const bool ok = db && pages && npages == (int32_t)db->pages.size();
  return write_lines<SummaryView>(
      "prb_write_summary_lines", ok, db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](SummaryView &v) {
        for (int32_t p = 0; p < npages; p++) {
          const prb_page_pairs &pp = pages[p];
          if (pp.npairs < 0 || (pp.npairs && !pp.pairs)) return bad_record("prb_write_summary_lines: bad page");
          const int32_t nseq = db->pages[p].nseq;
          for (int64_t i = 0; i < pp.npairs; i++) {
            const prb_pair_summary &x = pp.pairs[i];
            if (x.query < 0 || x.query >= nq || x.db_id < 0 || x.db_id >= nseq || x.hits < 1 || (i && x.query < pp.pairs[i - 1].query))
              return bad_record("prb_write_summary_lines: pair record " + std::to_string(i) + " of page " + std::to_string(p) +
                                " is inconsistent");
          }
          v.pages.push_back(PagePairs{pp.pairs, pp.npairs});
        }
        return (int)PRB_OK;
      },
      [&](const SummaryView &v, LineSink &sink) { return format_summary_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_top_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                        const prb_top_pair *pairs, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<TopView>(
      "prb_write_top_lines", n >= 0 && (!n || pairs), db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](TopView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_top_pair &x = pairs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || (i && x.s.query < pairs[i - 1].s.query))
            return bad_record("prb_write_top_lines: pair record " + std::to_string(i) + " is inconsistent");
        }
        v.r = pairs;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const TopView &v, LineSink &sink) { return format_top_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_null_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_null_pair *recs,
                         int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<NullView>(
      "prb_write_null_lines", n >= 0 && (!n || recs), db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](NullView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_null_pair &x = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.decoys < 1 || x.null_hits < 0 || x.null_hits > x.decoys ||
              x.null_le < 0 || x.null_le > x.null_hits || (i && x.s.query < recs[i - 1].s.query))
            return bad_record("prb_write_null_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const NullView &v, LineSink &sink) { return format_null_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_null_fdr_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_null_pair *recs,
                             const prb_null_fdr *fdr, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<NullFdrView>(
      "prb_write_null_fdr_lines", n >= 0 && (!n || (recs && fdr)), db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](NullFdrView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_null_pair &x = recs[i];
          const prb_null_fdr &f = fdr[i];
          const bool capped = !f.q_num && !f.q_den && !f.q_rank, triple = f.q_num && f.q_den && f.q_rank;
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.decoys < 1 || x.null_hits < 0 || x.null_hits > x.decoys ||
              x.null_le < 0 || x.null_le > x.null_hits || (i && x.s.query < recs[i - 1].s.query) || f.tests < 1 || f.tests >= (int64_t)1 << 31 ||
              f.rank < 1 || !(capped || triple))
            return bad_record("prb_write_null_fdr_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.f = fdr;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const NullFdrView &v, LineSink &sink) { return format_null_fdr_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_group_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_group_pair *recs,
                          int64_t n, const char *const *group_names, const int32_t *group_sizes, int32_t ngroups, int64_t id0, int fd,
                          int64_t *lines, int64_t *bytes) {
  return write_lines<GroupView>(
      "prb_write_group_lines", n >= 0 && (!n || recs) && ngroups >= 0 && (!ngroups || (group_names && group_sizes)), db, nq, qnames,
      qlen_unmasked, lines, bytes, fd,
      [&](GroupView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_group_pair &x = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.group < 0 || x.group >= ngroups || !group_names[x.group] ||
              x.members < 1 || x.hits < x.s.hits || (i && x.s.query < recs[i - 1].s.query))
            return bad_record("prb_write_group_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.group_names = group_names;
        v.group_sizes = group_sizes;
        return (int)PRB_OK;
      },
      [&](const GroupView &v, LineSink &sink) { return format_group_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_feature_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_feature_pair *recs, int64_t n, const char *const *feat_names, const int32_t *feat_start,
                            const int32_t *feat_end, int64_t nfeat, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<FeatureView>(
      "prb_write_feature_lines", n >= 0 && (!n || recs) && nfeat >= 0 && (!nfeat || (feat_names && feat_start && feat_end)), db, nq, qnames,
      qlen_unmasked, lines, bytes, fd,
      [&](FeatureView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_feature_pair &x = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.feature < 0 || x.feature >= nfeat || !feat_names[x.feature] ||
              x.inside < 0 || x.inside > x.s.hits || (i && x.s.query < recs[i - 1].s.query))
            return bad_record("prb_write_feature_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.feat_names = feat_names;
        v.feat_start = feat_start;
        v.feat_end = feat_end;
        return (int)PRB_OK;
      },
      [&](const FeatureView &v, LineSink &sink) { return format_feature_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_fnull_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_fnull_pair *recs,
                          int64_t n, const char *const *feat_names, const int32_t *feat_start, const int32_t *feat_end, int64_t nfeat, int64_t id0,
                          int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<FNullView>(
      "prb_write_fnull_lines", n >= 0 && (!n || recs) && nfeat >= 0 && (!nfeat || (feat_names && feat_start && feat_end)), db, nq, qnames,
      qlen_unmasked, lines, bytes, fd,
      [&](FNullView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_feature_pair &x = recs[i].f;
          const prb_fnull_pair &y = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.feature < 0 || x.feature >= nfeat || !feat_names[x.feature] ||
              x.inside < 0 || x.inside > x.s.hits || y.decoys < 1 || y.null_hits < 0 || y.null_hits > y.decoys || y.null_le < 0 ||
              y.null_le > y.null_hits || (i && x.s.query < recs[i - 1].f.s.query))
            return bad_record("prb_write_fnull_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.feat_names = feat_names;
        v.feat_start = feat_start;
        v.feat_end = feat_end;
        return (int)PRB_OK;
      },
      [&](const FNullView &v, LineSink &sink) { return format_fnull_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_featrank_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                             const prb_featrank_pair *recs, int64_t n, const char *const *feat_names, const int32_t *feat_start,
                             const int32_t *feat_end, int64_t nfeat, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<FeatRankView>(
      "prb_write_featrank_lines", n >= 0 && (!n || recs) && nfeat >= 0 && (!nfeat || (feat_names && feat_start && feat_end)), db, nq_total,
      qnames, qlen_unmasked, lines, bytes, fd,
      [&](FeatRankView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_feature_pair &x = recs[i].f;
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq_total || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.feature < 0 || x.feature >= nfeat || !feat_names[x.feature] ||
              x.inside < 0 || x.inside > x.s.hits)
            return bad_record("prb_write_featrank_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.feat_names = feat_names;
        v.feat_start = feat_start;
        v.feat_end = feat_end;
        return (int)PRB_OK;
      },
      [&](const FeatRankView &v, LineSink &sink) { return format_featrank_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_grouprank_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                              const prb_group_pair *recs, int64_t n, const char *const *group_names, const int32_t *group_sizes,
                              int32_t ngroups, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<GroupView>(
      "prb_write_grouprank_lines", n >= 0 && (!n || recs) && ngroups >= 0 && (!ngroups || (group_names && group_sizes)), db, nq_total, qnames,
      qlen_unmasked, lines, bytes, fd,
      [&](GroupView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_group_pair &x = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq_total || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.group < 0 || x.group >= ngroups || !group_names[x.group] ||
              x.members < 1 || x.hits < x.s.hits)
            return bad_record("prb_write_grouprank_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.group_names = group_names;
        v.group_sizes = group_sizes;
        return (int)PRB_OK;
      },
      [&](const GroupView &v, LineSink &sink) { return format_grouprank_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_gnull_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked, const prb_gnull_pair *recs,
                          int64_t n, const char *const *group_names, const int32_t *group_sizes, int32_t ngroups, int64_t id0, int fd,
                          int64_t *lines, int64_t *bytes) {
  return write_lines<GNullView>(
      "prb_write_gnull_lines", n >= 0 && (!n || recs) && ngroups >= 0 && (!ngroups || (group_names && group_sizes)), db, nq, qnames,
      qlen_unmasked, lines, bytes, fd,
      [&](GNullView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_group_pair &x = recs[i].g;
          const prb_gnull_pair &y = recs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1 || x.group < 0 || x.group >= ngroups || !group_names[x.group] ||
              x.members < 1 || x.hits < x.s.hits || y.decoys < 1 || y.null_hits < 0 || y.null_hits > y.decoys || y.null_le < 0 ||
              y.null_le > y.null_hits || (i && x.s.query < recs[i - 1].g.s.query))
            return bad_record("prb_write_gnull_lines: record " + std::to_string(i) + " is inconsistent");
        }
        v.r = recs;
        v.n = n;
        v.group_names = group_names;
        v.group_sizes = group_sizes;
        return (int)PRB_OK;
      },
      [&](const GNullView &v, LineSink &sink) { return format_gnull_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_target_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                           const prb_target_pair *pairs, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<TargetView>(
      "prb_write_target_lines", n >= 0 && (!n || pairs), db, nq_total, qnames, qlen_unmasked, lines, bytes, fd,
      [&](TargetView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_target_pair &x = pairs[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.s.query < 0 || x.s.query >= nq_total || x.s.db_id < 0 ||
              x.s.db_id >= db->pages[(size_t)x.page].nseq || x.s.hits < 1)
            return bad_record("prb_write_target_lines: pair record " + std::to_string(i) + " is inconsistent");
        }
        v.r = pairs;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const TargetView &v, LineSink &sink) { return format_target_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_profile_lines(const prb_db *db, int32_t nq, const char *const *qnames, const int32_t *qlen_unmasked,
                            const prb_profile_pos *rows, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<ProfileView>(
      "prb_write_profile_lines", n >= 0 && (!n || rows), db, nq, qnames, qlen_unmasked, lines, bytes, fd,
      [&](ProfileView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_profile_pos &x = rows[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.query < 0 || x.query >= nq || x.db_id < 0 ||
              x.db_id >= db->pages[(size_t)x.page].nseq || x.hits < 1 || x.targets < 1 || x.pos < 0 ||
              (i && (x.query < rows[i - 1].query || (x.query == rows[i - 1].query && x.pos <= rows[i - 1].pos))))
            return bad_record("prb_write_profile_lines: row " + std::to_string(i) + " is inconsistent");
        }
        v.r = rows;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const ProfileView &v, LineSink &sink) { return format_profile_batch(v, db->tabs, id0, sink, format_threads()); });
}

int prb_write_region_lines(const prb_db *db, int32_t nq_total, const char *const *qnames, const int32_t *qlen_unmasked,
                           const prb_target_region *regions, int64_t n, int64_t id0, int fd, int64_t *lines, int64_t *bytes) {
  return write_lines<RegionView>(
      "prb_write_region_lines", n >= 0 && (!n || regions), db, nq_total, qnames, qlen_unmasked, lines, bytes, fd,
      [&](RegionView &v) {
        for (int64_t i = 0; i < n; i++) {
          const prb_target_region &x = regions[i];
          if (x.page < 0 || x.page >= (int32_t)db->pages.size() || x.query < 0 || x.query >= nq_total || x.db_id < 0 ||
              x.db_id >= db->pages[(size_t)x.page].nseq || x.start < 0 || x.end < x.start || x.hits < 0 || x.max_hits < 1 || x.max_queries < 1)
            return bad_record("prb_write_region_lines: region record " + std::to_string(i) + " is inconsistent");
        }
        v.r = regions;
        v.n = n;
        return (int)PRB_OK;
      },
      [&](const RegionView &v, LineSink &sink) { return format_region_batch(v, db->tabs, id0, sink, format_threads()); });
}

} // extern "C"
