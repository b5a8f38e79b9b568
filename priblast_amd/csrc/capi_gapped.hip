// C ABI, part 3b: the gapped stage of the search of one sub-batch (ExtendWithGap, rna_interaction_search.cpp:302-320;
// gapped_stage, which search_range of capi_search.hip calls between its sort + filter stages) and the second
// extension of the few final hits whose base pairs the first one left no record of (retrace_tier, for traceback).
// Everything that launches a gapped kernel is here: the launches fill a GapArgs (search_kernels.hpp) by name.
#include <algorithm>
#include <cstdio>

#include "search_stages.hpp"

namespace prb {

// The cascade of kernels a hit goes through until one has the capacity for it: the front kernel (gapped_front.hip),
// LDS tiers 0 and 1 (8 lanes per hit), tier 2 (16 lanes), tier 3 (a wavefront per hit), then the wave-per-hit kernel
// with HBM scratch of any size.
static const char *const kTierTimer[5] = {"gapped", "gapped_t1", "gapped_t2", "gapped_t3", "gapped_slow"};

// The hits of the view that no kernel has completed yet, on their way down the cascade
struct WorkList {
  const uint32_t *cur = nullptr; // indices into U (nullptr: all of 0..m-1)
  int64_t m = 0;
  uint32_t *bufs[2];             // where the next, shorter list is written, in turns
  int nb = 0;
  uint32_t *spare() const { return bufs[nb]; }
};
// and what the cascade of one chunk carries along
struct Cascade {
  WorkList l;
  GapResume rs[kLdsTiers - 1]; // rs[t] = the state dumps of the hits that outgrow tier t
  int skip_mask = 0;
};

// What every launch on the sub-batch's view (s.U, s.G, s.first) shares, for the extension (mode 0) or the base pairs
// of a list (mode 2); the call sites name the rest: n, subset, rin / rout, handover, lt, bp_off, acc_scratch
static GapArgs view_args(const SubSearch &s, int mode) {
  SearchWs &w = s.w;
  GapArgs a;
  a.in = s.U;
  a.out = s.G;
  a.qb = s.qb->view;
  a.pg = s.pd;
  a.sc = s.sc;
  a.o = s.eo;
  a.first_flag = s.first;
  a.bp_out = w.bpOut.as<int32_t>();
  a.next_work = w.count.as<unsigned long long>() + 1;
  if (mode == 0) {
    a.overflow = w.overflow.as<uint8_t>();
    a.tier_out = w.tierOf.as<uint8_t>();
    a.bp_count = w.ntrace.as<int32_t>();
    a.trace = w.trace.as<uint16_t>();
  }
  return a;
}

static int scratch_for(SubSearch &s, int64_t n, int cap_diag, int cap_rec, GapScratch &gs) {
  gs.cap_diag = cap_diag;
  gs.cap_rec = cap_rec;
  gs.bytes_per_wave = gapped_wave_scratch_bytes(cap_diag, cap_rec);
  if (gs.bytes_per_wave <= kGapWaveLdsBytes && !s.k.wave_hbm) { // the state fits the LDS of a workgroup
    gs.base = nullptr;
    gs.nwaves = (int32_t)std::min<int64_t>(n, 4096);
    return PRB_OK;
  }
  int64_t nw = std::min<int64_t>(n, 4096);
  while (nw > 64 && (size_t)nw * gs.bytes_per_wave > ((size_t)4 << 30)) nw /= 2;
  gs.nwaves = (int32_t)nw;
  int r = s.w.gapScratch.ensure((size_t)nw * gs.bytes_per_wave);
  gs.base = s.w.gapScratch.as<uint8_t>();
  return r;
}

// next = the entries of the work list `cur` (nullptr: 0..m-1) whose overflow flag is set
static int select_overflow(SubSearch &s, const uint32_t *cur, int64_t m, uint32_t *next, int64_t *mout) {
  return select_flagged(s.ctx, s.w, cur, s.w.overflow.as<uint8_t>(), next, (size_t)m, mout);
}
// the same for the list of a cascade, which the selection then is
static int advance(SubSearch &s, WorkList &l, int64_t *rest) {
  if (int rc = select_overflow(s, l.cur, l.m, l.spare(), rest)) return rc;
  l.cur = l.spare();
  l.nb ^= 1;
  return PRB_OK;
}

// Wave-per-hit kernel with its state in HBM scratch, for the device list `cur` (indices into U;
// nullptr = all) of m hits.  mode 0 writes G and retries hits that still overflow with a 4x
// larger scratch; mode 2 writes base pairs at off_dev (indexed by list position).
// (long traces, search_kernels.hpp: not when the stage runs in chunks - the kept lists renumber the hits -, not for a
// list that is every hit - PRB_GAPPED_FIRST_TIER=4 -; PRB_TRACE_NO_LONG / PRB_TRACE_LONG_CAP are for the tests)
static int run_wave(SubSearch &s, int mode, const uint32_t *cur, int64_t m, uint32_t *spare, const int64_t *off_dev, int handover = 0) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  int rc;
  const bool long_traces = mode == 0 && !s.chunked && m <= 65536 && !s.k.trace_no_long;
  if (long_traces && cur == nullptr) { // (every hit, as a list)
    if ((rc = w.slowList.ensure((size_t)m * 4))) return rc;
    PRB_HIP(launch_iota_u32(w.slowList.as<uint32_t>(), m, ctx->stream));
    cur = w.slowList.as<uint32_t>();
  }
  if (long_traces) {
    const int32_t cap = s.k.trace_long_cap;
    if (s.lt_used == 0) {
      if ((rc = w.slowSlot.ensure((size_t)s.nmax * 4))) return rc;
      PRB_HIP(hipMemsetAsync(w.slowSlot.p, 0xFF, (size_t)s.nmax * 4, ctx->stream));
    }
    const size_t have = (size_t)s.lt_used, need = have + (size_t)m;
    if ((rc = grow_keep(ctx, w.slowCnt, have * 8, need * 8)) || (rc = grow_keep(ctx, w.slowTrace, have * 8 * cap, need * 8 * cap))) return rc;
    PRB_HIP(hipMemsetAsync(w.slowCnt.as<int32_t>() + have * 2, 0xFF, (size_t)m * 8, ctx->stream));
    PRB_HIP(launch_assign_slots(cur, m, s.lt_used, w.slowSlot.as<int32_t>(), ctx->stream));
    s.lt_used += (int32_t)m;
    s.lt = LongTrace{w.slowTrace.as<uint32_t>(), w.slowCnt.as<int32_t>(), w.slowSlot.as<int32_t>(), cap};
  }
  int cap_diag = 512, cap_rec = 2048;
  if (mode != 0) { // caps known to suffice for every hit seen so far
    cap_diag = std::max(512, ctx->max_gap_caps);
    cap_rec = cap_diag * 4;
  }
  GapArgs a = view_args(s, mode);
  a.bp_off = off_dev;
  a.handover = handover;
  a.lt = s.lt;
  uint32_t *other = spare;
  while (m > 0) {
    GapScratch gs;
    if ((rc = scratch_for(s, m, cap_diag, cap_rec, gs))) return rc;
    a.n = m;
    a.subset = cur;
    PRB_HIP(launch_gapped_wave(a, gs, mode, ctx->stream));
    if (mode != 0) break;
    int64_t again = 0;
    if ((rc = select_overflow(s, cur, m, other, &again))) return rc;
    uint32_t *done_list = const_cast<uint32_t *>(cur);
    cur = other;
    other = done_list ? done_list : (other == w.listA.as<uint32_t>() ? w.listB.as<uint32_t>() : w.listA.as<uint32_t>());
    m = again;
    if (m == 0) break;
    cap_diag *= 4;
    cap_rec *= 4;
    if (cap_diag > 32768) {
      set_error("gapped extension exceeds the supported extension length (32768)");
      return PRB_ERR_STATE;
    }
    ctx->max_gap_caps = std::max(ctx->max_gap_caps, cap_diag);
  }
  return PRB_OK;
}
// the whole list `l` through it, as the cascade's last kernel (the next sub-batch's front goes out first: these few,
// longest extensions run nearly alone)
static int run_slow(SubSearch &s, WorkList &l, int handover) {
  int rc;
  if (!handover) call_front_free(s);
  if ((rc = s.ctx->time_begin())) return rc;
  s.hs->slow_hits += l.m;
  s.ctx->slow_hits += l.m;
  if ((rc = run_wave(s, 0, l.cur, l.m, l.spare(), nullptr, handover))) return rc;
  l.m = 0;
  return s.ctx->time_end(kTierTimer[kWaveTier], 1);
}

// the front kernel on the list: what it completes leaves the list
static int run_front(SubSearch &s, Cascade &c, bool second_only = false) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  WorkList &l = c.l;
  int rc;
  if ((rc = w.frontScratch.ensure(gapped_front_scratch_bytes()))) return rc;
  if ((rc = ctx->time_begin())) return rc;
  GapArgs a = view_args(s, 0);
  a.n = l.m;
  a.subset = l.cur;
  a.tier_id = 0; // what it completes counts as tier 0's
  PRB_HIP(launch_gapped_front(a, w.frontScratch.p, second_only && !s.k.front_paired, ctx->stream));
  int64_t rest = 0;
  if ((rc = advance(s, l, &rest))) return rc;
  if (s.k.debug_rows) fprintf(stderr, "[front] hits %lld, go on %lld\n", (long long)l.m, (long long)rest);
  ctx->timers["gapped_front_hits"].launches += l.m - rest; // (a counter, not a time: hits completed by the front kernel)
  l.m = rest;
  return ctx->time_end("gapped_front", 1);
}

// the LDS tiers and the wavefront-per-hit kernel on the list, each taking what the one before it could not hold
// (hold_wave: the list is handed back before the wavefront-per-hit kernel instead)
static int run_cascade(SubSearch &s, Cascade &c, int handover, bool hold_wave) {
  prb_ctx *ctx = s.ctx;
  WorkList &l = c.l;
  int rc;
  for (int tier = s.k.first_tier; tier <= kWaveTier && l.m > 0; tier++) {
    if (tier < kLdsTiers - 1 && ((c.skip_mask >> tier) & 1)) continue;
    if (tier == kWaveTier) {
      if (hold_wave) break;
      if ((rc = run_slow(s, l, handover))) return rc;
      continue;
    }
    if ((rc = ctx->time_begin())) return rc;
    if (tier == 0) ctx->timers["gapped_tier0_hits"].launches += l.m; // (a counter, not a time: hits that entered tier 0)
    GapArgs a = view_args(s, 0);
    a.n = l.m;
    a.subset = l.cur;
    if (tier >= 1) a.rin = c.rs[tier - 1];
    if (tier < kLdsTiers - 1) a.rout = c.rs[tier];
    a.handover = handover;
    a.acc_scratch = s.w.accScratch.as<double>();
    PRB_HIP(launch_gapped_lds(a, 0, tier, s.k.tiers, ctx->stream));
    int64_t rest = 0;
    if ((rc = advance(s, l, &rest))) return rc;
    if (s.k.debug_rows)
      fprintf(stderr, "[tier %d%s] hits %lld, go on %lld\n", tier, handover ? ", first direction" : "", (long long)l.m, (long long)rest);
    l.m = rest;
    if ((rc = ctx->time_end(kTierTimer[tier], 1))) return rc;
  }
  return PRB_OK;
}

// state dumps for the hits that outgrow tier 0 (~15 %: room for one hit in four, at most 4 M), tier 1
// (~4 %: one in eight, at most 2 M) and tier 2 (~0.7 %: one in 32, at most 1 M)
static const struct {
  int one_in;
  int32_t at_most;
} kResumeRoom[kLdsTiers - 1] = {{4, 4 << 20}, {8, 2 << 20}, {32, 1 << 20}};
static_assert(kLdsTiers == 4, "one capacity rule per LDS tier but the last");
static int prepare_resume(SubSearch &s, Cascade &c) {
  SearchWs &w = s.w;
  int rc;
  if ((rc = w.resumeSlot.ensure((size_t)s.nch * 4 * (kLdsTiers - 1))) || (rc = w.resumeCount.ensure(16))) return rc;
  for (int t = 0; t < kLdsTiers - 1; t++) {
    const auto &room = kResumeRoom[t];
    c.rs[t].cap = s.k.resume_cap > 0 ? s.k.resume_cap : (int32_t)std::min<int64_t>(s.nch / room.one_in + 1024, room.at_most);
    if ((rc = w.resumePool[t].ensure((size_t)c.rs[t].cap * gapped_resume_bytes(t)))) return rc;
    c.rs[t].slot = w.resumeSlot.as<int32_t>() + (size_t)t * s.nch;
    c.rs[t].pool = w.resumePool[t].as<uint8_t>();
    c.rs[t].count = w.resumeCount.as<uint32_t>() + t;
  }
  return PRB_OK;
}
static int clear_resume(SubSearch &s) {
  PRB_HIP(hipMemsetAsync(s.w.resumeCount.p, 0, 16, s.ctx->stream));
  PRB_HIP(hipMemsetAsync(s.w.resumeSlot.p, 0xFF, (size_t)s.nch * 4 * (kLdsTiers - 1), s.ctx->stream));
  return PRB_OK;
}

// The hits that the front kernel leaves have a direction that finds something - or had too many cells for it.  Nine
// SECOND directions in ten still find nothing, and a tier pays for proving that what it pays for 16 anti-diagonals of
// any extension (8 - 40 ns per hit, against the front kernel's 0.6 per direction).  So the cascade first runs FIRST
// directions only (GapArgs::handover; a hit whose first direction the front kernel completed runs its second one, as
// ever), the front kernel then looks at the second directions of what the tiers stopped behind, and only the hits
// whose second direction finds something too come back to the cascade, for that direction.
static int run_handover(SubSearch &s, Cascade &c) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  WorkList &l = c.l;
  int rc;
  const int64_t m_first = l.m;
  if ((rc = w.listC.ensure((size_t)m_first * 4))) return rc;
  PRB_HIP(hipMemcpyAsync(w.listC.p, l.cur, (size_t)m_first * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = run_cascade(s, c, 1, true))) return rc;
  // What outgrew the last LDS tier - ~150 extensions per configs[2] query, a wavefront each for 2 ms on a GPU that is
  // otherwise idle - waits for the second pass's: ONE launch of the wavefront-per-hit kernel for both (a launch lasts
  // as long as its longest extension; these hits run both their directions there).
  const int64_t n_slow = l.m;
  if (n_slow > 0) {
    if ((rc = w.slowList.ensure((size_t)n_slow * 4))) return rc;
    PRB_HIP(hipMemcpyAsync(w.slowList.p, l.cur, (size_t)n_slow * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  // the hits an LDS tier stopped behind their first direction
  PRB_HIP(launch_flag_marked(w.tierOf.as<uint8_t>(), w.listC.as<uint32_t>(), m_first, kHandoverMark, w.overflow.as<uint8_t>(), ctx->stream));
  l.cur = w.listC.as<uint32_t>();
  l.m = m_first;
  int64_t mh = 0;
  if ((rc = advance(s, l, &mh))) return rc;
  l.m = mh;
  if (l.m > 0) {
    if (c.rs[0].slot && (rc = clear_resume(s))) return rc; // (the hand-over slots of the first pass are not to be taken for this pass's)
    if ((rc = run_front(s, c, true))) return rc; // (all of them stopped behind their first direction: a lane per hit)
    if ((rc = run_cascade(s, c, 0, true))) return rc;
  }
  if (n_slow + l.m == 0) return PRB_OK;
  if (l.m > 0) { // both passes' lists as one
    if ((rc = grow_keep(ctx, w.slowList, (size_t)n_slow * 4, (size_t)(n_slow + l.m) * 4))) return rc;
    PRB_HIP(hipMemcpyAsync(w.slowList.as<uint32_t>() + n_slow, l.cur, (size_t)l.m * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  l.cur = w.slowList.as<uint32_t>();
  l.m += n_slow;
  return run_slow(s, l, 0);
}

// the cascade for the view (s.U, s.G, s.nch, s.first)
static int extend_chunk(SubSearch &s) {
  SearchWs &w = s.w;
  int rc;
  Cascade c;
  if ((rc = w.accScratch.ensure(std::max<size_t>(gapped_acc_scratch_bytes(), 8)))) return rc;
  PRB_HIP(hipMemsetAsync(w.tierOf.p, 0, (size_t)s.nch, s.ctx->stream)); // no hit carries a resume mark yet
  if (!s.k.no_resume) {
    if ((rc = prepare_resume(s, c)) || (rc = clear_resume(s))) return rc;
  }
  c.l.m = s.nch; // all of U
  c.l.bufs[0] = w.listA.as<uint32_t>();
  c.l.bufs[1] = w.listB.as<uint32_t>();
  // In front of the cascade (gapped_front.hip; PRB_GAPPED_FRONT=0 leaves it out): the hits neither direction of which
  // finds anything - four in five - are completed by a kernel that only has to prove that.
  const bool front_on = s.k.first_tier == 0 && s.k.front && gapped_front_supported(s.sc, s.eo);
  if (front_on) {
    if ((rc = run_front(s, c))) return rc;
    c.skip_mask = s.k.skip_tiers;
  }
  if (!(front_on && s.k.handover)) return run_cascade(s, c, 0, false);
  return c.l.m > 0 ? run_handover(s, c) : PRB_OK;
}

// Of the chunk just extended, what is not above the -g threshold is appended to the kept lists: the extended hits as
// records in hitsB (what the final sort takes), the hits they came from, their first-of-query flags, tiers, chain lengths
// and trace slots - everything the traceback of the final hits reads, indexed by position in the kept lists from now on
static int keep_chunk(SubSearch &s, int64_t c0) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  const size_t trace_row = 2 * kTraceCap * sizeof(uint16_t);
  int rc;
  int64_t mc = 0;
  if ((rc = ctx->time_begin())) return rc;
  if ((rc = compact_below(ctx, w, s.G, s.nch, s.opts.final_threshold, w.cidx, w.hitsB, &mc, s.ngap))) return rc;
  if (mc > 0) {
    const size_t have = (size_t)s.ngap, need = have + (size_t)mc;
    if ((rc = grow_keep(ctx, w.keptU, have * sizeof(HitRec), need * sizeof(HitRec))) || (rc = grow_keep(ctx, w.keptFirst, have, need)) ||
        (rc = grow_keep(ctx, w.keptTier, have, need)) || (rc = grow_keep(ctx, w.keptNtrace, have * 4, need * 4)) ||
        (rc = grow_keep(ctx, w.keptTrace, have * trace_row, need * trace_row)))
      return rc;
    const uint32_t *idx = w.cidx.as<uint32_t>();
    PRB_HIP(launch_gather_hits_to_recs(s.U, idx, w.keptU.as<HitRec>() + have, mc, ctx->stream));
    PRB_HIP(launch_gather_u8(s.first, idx, w.keptFirst.as<uint8_t>() + have, mc, ctx->stream));
    PRB_HIP(launch_gather_u8(w.tierOf.as<uint8_t>(), idx, w.keptTier.as<uint8_t>() + have, mc, ctx->stream));
    PRB_HIP(launch_gather_u32(w.ntrace.as<uint32_t>(), idx, w.keptNtrace.as<uint32_t>() + have, mc, ctx->stream));
    PRB_HIP(launch_gather_rows(w.trace.p, idx, static_cast<uint8_t *>(w.keptTrace.p) + have * trace_row, mc, (int)trace_row, ctx->stream));
  }
  if ((rc = ctx->time_end("filter", 2))) return rc;
  if (s.k.debug_rows)
    fprintf(stderr, "[gapped chunk] hits %lld at %lld of %lld, kept %lld\n", (long long)s.nch, (long long)c0, (long long)s.nung, (long long)mc);
  s.ngap += mc;
  if (s.ngap > (int64_t)UINT32_MAX - 16) {
    set_error("more than 4e9 hits under the -g threshold in one sub-batch: build the database in smaller pages (db -c)");
    return PRB_ERR_NOMEM;
  }
  return PRB_OK;
}

// The state of this stage is ~350 B per hit (the extended hit, work lists, trace slots, hand-over slots): a list
// longer than PRB_GAPPED_CHUNK_HITS (a 45 kb query against a 100 M character page leaves 5e8 hits behind -f) goes through
// it in chunks of that many - the list is sorted and filtered already, the extension of a hit depends on nothing but the
// hit -, and only what is not above the -g threshold is kept of a chunk.  The final sort + filter then run over the
// union, as the reference's do over the whole list (rna_interaction_search.cpp:302-320).
int gapped_stage(SubSearch &s) {
  prb_ctx *ctx = s.ctx;
  SearchWs &w = s.w;
  int rc;
  s.chunked = s.nung > s.k.gapped_chunk_hits;
  s.nmax = s.chunked ? s.k.gapped_chunk_hits : s.nung;
  const size_t NM = (size_t)s.nmax;
  if ((rc = w.hitsC.ensure(hits_bytes(s.nmax)))) return rc;
  if ((rc = w.overflow.ensure(NM)) || (rc = w.subset.ensure(NM * 4)) || (rc = w.ntrace.ensure(NM * 4)) || (rc = w.tierOf.ensure(NM)) ||
      (rc = w.listA.ensure(NM * 4)) || (rc = w.listB.ensure(NM * 4)) || (rc = w.count.ensure(16)) ||
      (rc = w.trace.ensure(NM * 2 * kTraceCap * sizeof(uint16_t))))
    return rc;
  s.G = carve_hits(w.hitsC, s.nmax);
  s.nch = s.nmax;
  if (!s.chunked) {
    if ((rc = extend_chunk(s))) return rc;
    s.tier_all = w.tierOf.as<uint8_t>();
    s.ntrace_all = w.ntrace.as<int32_t>();
    s.trace_all = w.trace.as<uint16_t>();
    return PRB_OK;
  }
  const HitSoA Uall = s.U;
  for (int64_t c0 = 0; c0 < s.nung; c0 += s.k.gapped_chunk_hits) {
    s.nch = std::min<int64_t>(s.k.gapped_chunk_hits, s.nung - c0);
    s.U = offset_hits(Uall, c0);
    s.G = carve_hits(w.hitsC, s.nch);
    s.first = w.first.as<uint8_t>() + c0;
    if ((rc = extend_chunk(s)) || (rc = keep_chunk(s, c0))) return rc;
  }
  // from here on "the hits before the gapped stage" are the kept ones, in the order they were kept
  if (s.ngap > 0) {
    if ((rc = w.hitsA.ensure(hits_bytes(s.ngap))) || (rc = w.cidx.ensure((size_t)s.ngap * 4))) return rc;
    s.U = carve_hits(w.hitsA, s.ngap);
    PRB_HIP(launch_iota_u32(w.cidx.as<uint32_t>(), s.ngap, ctx->stream));
    PRB_HIP(launch_gather_recs_to_hits(w.keptU.as<HitRec>(), w.cidx.as<uint32_t>(), s.U, s.ngap, ctx->stream));
  }
  s.first = w.keptFirst.as<uint8_t>();
  s.tier_all = w.keptTier.as<uint8_t>();
  s.ntrace_all = w.keptNtrace.as<int32_t>();
  s.trace_all = w.keptTrace.as<uint16_t>();
  return PRB_OK;
}

int retrace_tier(SubSearch &s, int tier, const uint32_t *subset2, const int64_t *bpOff2, int64_t m) {
  if (tier == kWaveTier) return run_wave(s, 2, subset2, m, nullptr, bpOff2);
  GapArgs a = view_args(s, 2);
  a.n = m;
  a.subset = subset2;
  a.bp_off = bpOff2;
  a.acc_scratch = s.w.accScratch.as<double>();
  PRB_HIP(launch_gapped_lds(a, 2, tier, s.k.tiers, s.ctx->stream));
  return PRB_OK;
}

} // namespace prb
