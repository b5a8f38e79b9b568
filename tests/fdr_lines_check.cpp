// A stand-alone caller of the host line writers of `ris -t -z N` and `ris -t -z N -Q` (priblast_amd/host/output.cpp) on
// hand-made records, for tests/test_fdr_host.py - and for a sanitizer build of the host code, which needs a main of its
// own.  Every argument is one record, query:db_id:decoys:null_hits:null_le:tests:rank:q_num:q_den:q_rank, ascending by
// query; the records' lines are written to standard output twice: first without the three columns, then with them.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "output.hpp"

int main(int argc, char **argv) {
  std::vector<prb_null_pair> recs;
  std::vector<prb_null_fdr> figs;
  for (int i = 1; i < argc; i++) {
    long long v[10];
    if (std::sscanf(argv[i], "%lld:%lld:%lld:%lld:%lld:%lld:%lld:%lld:%lld:%lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8],
                    &v[9]) != 10) {
      std::fprintf(stderr, "bad record %s\n", argv[i]);
      return 2;
    }
    prb_null_pair r{};
    r.s.query = (int32_t)v[0];
    r.s.db_id = (int32_t)v[1];
    r.s.hits = 1 + i % 3;
    r.s.e_min = -10.5 - i;
    r.s.e_sum = -12.25 - i;
    r.s.e_acc = 1.5;
    r.s.e_hyb = -12.0 - i;
    r.page = 0;
    r.decoys = (int32_t)v[2];
    r.null_hits = v[3];
    r.null_le = v[4];
    r.null_min = -11.0;
    recs.push_back(r);
    prb_null_fdr f{};
    f.tests = v[5];
    f.rank = (uint32_t)v[6];
    f.q_num = (uint32_t)v[7];
    f.q_den = (uint32_t)v[8];
    f.q_rank = (uint32_t)v[9];
    figs.push_back(f);
  }
  prb::SeqTable tab;
  for (int t = 0; t < 4; t++) {
    tab.names.push_back("target" + std::to_string(t));
    tab.len.push_back(50);
    tab.len_unmasked.push_back(50);
    tab.start_pos.push_back(51 * t);
  }
  const std::vector<prb::SeqTable> tabs{tab};
  const std::vector<std::string> names{"qa", "qb", "qc"};
  const std::vector<int32_t> qlen{30, 31, 32};
  prb::NullFdrView v;
  v.nq = names.size();
  v.names = names.data();
  v.qlen_unmasked = qlen.data();
  v.r = recs.data();
  v.f = figs.data();
  v.n = (int64_t)recs.size();
  prb::LineSink plain, fdr;
  plain.fd = fdr.fd = 1;
  if (prb::format_null_batch(v, tabs, 0, plain, 2) < 0 || prb::format_null_fdr_batch(v, tabs, 0, fdr, 2) < 0) return 1;
  return plain.lines == v.n && fdr.lines == v.n ? 0 : 3;
}
