// prb_ctx: one GPU's state behind the C ABI (include/priblast_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "energy.hpp"
#include "raccess_device.hpp"

namespace prb {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what); // records the error text, returns PRB_ERR_HIP

#define PRB_HIP(call)                                   \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return prb::hip_fail(e_, #call); \
  } while (0)

// Device buffer that only grows.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes);
  void release();
  template <class T> T *as() const { return static_cast<T *>(p); }
};

struct StageTimer {
  double ms = 0;
  int64_t launches = 0;
};

// The stages outside the full-output search (prb_ctx::mode_timers): one row each, the value and - in the same order -
// the name that prb_ctx_stage_ms answers to
enum class ModeTimer { kSummary, kTop, kProfile, kTopHits, kTargets, kDistinct, kChain, kAllow, kCoverage, kNull, kGroup, kGnull, kEval, kGroupRank, kFeature, kFnull, kFeatRank, kFdr, kCount };
inline constexpr const char *kModeTimerName[(int)ModeTimer::kCount] = {"summary", "top",   "profile",  "tophits", "targets", "distinct",
                                                                       "chain",   "allow", "coverage", "null",    "group",   "gnull",
                                                                       "eval",    "grouprank", "feature", "fnull",
                                                                       "featrank", "fdr"};

} // namespace prb

struct prb_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  prb::EnergyParams params;
  prb::RaccessTables ra_tables;
  prb::FmathTables fm_tables;
  prb::RaConst ra_const{};
  // int tables for the search stages (SearchConst, search_kernels.hpp)
  void *search_const = nullptr;
  void *search_ws = nullptr;   // prb::SearchWs, search_host.hpp
  int64_t slow_hits = 0;       // extensions that went through the HBM-scratch fallback kernel
  int max_gap_caps = 128;      // largest diagonal capacity any gapped extension has needed
  bool keep_device_records = false; // final hit sets also keep their packed records in HBM (for prb_gather_hits)
  size_t keep_hint_hits = 0, keep_hint_bp = 0; // bytes the last such hit set ended up with (KeepBuf::hint)
  size_t host_hint_hits = 0, host_hint_bp = 0; // hits / pair ints of the last final hit set (its vectors' first reserve)
  prb::DevBuf d_expd, d_log, d_small, d_big;
  // Raccess workspaces
  prb::DevBuf ra_band, ra_vec, ra_codes, ra_desc, ra_acc, ra_cond;
  prb::DevBuf ra_watchdog; // one int: RaBatch::watchdog of this context's launches
  size_t ra_budget_bytes = 0;
  std::map<std::string, prb::StageTimer> timers;
  // What is not a stage of the full-output search - the per-pair reduction ("summary"), the merges, joins and finishes of
  // the result tables (a stage per table), the selections of opts->distinct_sites / chain_sites and the pairs' test under
  // opts->allowed_pairs - is kept apart from `timers`: every name that is written as time_end("...", n), HostTimer x(ctx,
  // "...") or timers["..."] has to be a stage that bench.py reports (tests/test_host.py), and these are not.  So they are passed as
  // prb::ModeTimer values and never spelled in one of those three forms; prb::kModeTimerName has their names.
  prb::StageTimer mode_timers[(int)prb::ModeTimer::kCount];

  int time_begin();
  int time_end(const char *stage, int64_t launches);
  int time_end(prb::ModeTimer t, int64_t launches) { return time_end(mode_timers[(int)t], launches); }
  int time_end(prb::StageTimer &t, int64_t launches);
};
