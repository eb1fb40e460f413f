// ltr_plan_run.hip -- running a plan: ltr_plan_execute (the launches of a plan over the plan's stream and side streams of the
// context), ltr_plan_fetch, per-launch timing and statistics, what the context learns about the workgroup classes' first pass,
// and ltr_align_batch (create + execute + fetch + destroy).  Building a plan: ltr_plan_build.hip.

#include <cmath>
#include <cstring>

#include "ltr_ctx.h"

using namespace ltrp;                            // class table, Rules, classify_pair, sort_by_class (ltr_plan.h)

#ifdef LTR_KDEBUG
static uint32_t* g_dbg_host = nullptr;
extern "C" uint32_t* ltr_debug_buffer(void) { return g_dbg_host; }
#endif

// The statistics slots that have arrived (under ctx->mu).  Certificate pass: more than half of the pairs failed -> the threshold
// kernels go first from now on; threshold pass: fewer than a quarter aborted -> back to the certificates (a pair that aborts
// would have failed its certificate too; the converse does not hold, so the way back is the cautious one).
void wg_stats_poll(ltr_ctx* ctx) {
  if (!ctx->wg_stat_pin) return;
  for (int i = 0; i < ltr_ctx::kWgStatSlots; ++i) {
    ltr_ctx::WgStatSlot& sl = ctx->wg_stat[i];
    if (!sl.busy || hipEventQuery(sl.ev) != hipSuccess) continue;
    sl.busy = false;
    const uint32_t unfinished = ctx->wg_stat_pin[2 * i], scored = ctx->wg_stat_pin[2 * i + 1];
    if (sl.epoch != ctx->wg_epoch || scored == 0) continue;
    ctx->wg_last_unfinished = unfinished; ctx->wg_last_scored = scored;
    if (sl.mode == 0) ctx->wg_thr_first = ((uint64_t)unfinished * 2 > scored) ? 1 : 0;
    else ctx->wg_thr_first = ((uint64_t)unfinished * 4 >= scored) ? 1 : 0;
  }
  (void)hipGetLastError();                                       // (hipEventQuery's hipErrorNotReady is no error)
}

namespace {

// Exact kernels over whatever the certificate kernels queued (the list lengths live on the device); a kernel no pair
// of the plan can reach is not launched.  The exact launches are independent of each other (own list, own queue word;
// the generic kernel and kXLong park column blocks in strip regions of their own) and mostly latency: a handful of
// pairs each, as long as their longest pair.  Without per-launch timing they run on side streams of the context,
// each as soon as no certificate launch still to come can feed its list -- list c takes reads of at least
// kListMinC[c] columns and the certificate classes run longest reads first -- and the plan's stream waits for them at
// the end: a plan of 1250 loci used to end in ~4 ms of exact launches behind its last certificate launch.
// (Not for plans of a few hundred pairs -- config 2: the cross-stream waits cost more than they hide, 0.14 ms per
// pass against 0.10 -- and not when the lists are the bulk of the work, mode 4: 1.35e12 against 1.45e12 cells/s.)
const int kListMinC[kNumExact] = {0, 0, 64 * kXShortW + 1, 64 * kXMidW + 1, 64 * kXLongW + 1, kXWg4MaxC + 1};

// One ltr_plan_execute: what its launches share.  The steps below are its member functions, in the order run()
// calls them.
struct Execute {
  ltr_plan* const plan;
  ltr_ctx* const ctx;
  hipStream_t st;                           // the plan's stream for this execute
  double* out;
  KernelArgs A;
  bool sym = true;                          // symmetric indel model (ins->match == del->match, match->ins == match->del): 11-op cell body
  bool wg_thr = false;                      // the threshold kernels score the workgroup classes
  ltrp::ThresholdGroups thr;                // ... per class: its kernel; pairs of the launch it leads (0: led by a class before it)
  bool x_done[kNumExact] = {false}, x_launched[kNumExact] = {false};
  int launches = 0;
  // the schedule of this execute: fixed by the plan, its timing level and the stream, before anything is queued
  hipStream_t lanes[4];
  const bool fan;                           // the launches are dealt over the lanes
  const int nl, nb;                         // lanes; big lanes (with four lanes the last two take the small classes)
  const bool x_fan;                         // the exact launches run on side streams of their own
  const std::vector<Launch>& list;          // the launches, in order (level-2 timing: the multi-width launches class by class)

  Execute(ltr_plan* p, ltr_ctx* c, double* d_out_ll, void* stream_v);
  int snapshot_tables();
  int reset_control_words();
  int ensure_exact_events();
  hipStream_t exact_stream(int which) const;
  int capped(int grid) const { return plan->grid_cap > 0 ? std::min(grid, plan->grid_cap) : grid; }   // (the grids formed here, under the plan's "grid_cap")
  void note(int kind, int cls, int grid, int takers, int64_t items) { plan->launch_log.push_back({kind, cls, grid, takers, items}); }
  int behind_the_lanes(int c, hipStream_t s2, bool small_events);
  int launch_exact_list(int c, bool small_events);
  int launch_class(const Launch& L, int li);
  void note_wg_stats();
  int run();
};

static bool exact_lists_fan_out(const ltr_plan* plan, const ltr_ctx* ctx) {
  int64_t seeded = 0;
  for (int c = 0; c < kNumExact; ++c) seeded += plan->x_seed[c];
  return !plan->timing && plan->n_pairs >= (int64_t)32 * ctx->n_cu && seeded * 16 < plan->n_pairs;
}

// The launches go round-robin over the plan's stream and side streams of the context: the classes that fill the GPU's
// wave slots ("big") over lanes 0 .. nb-1, the classes that do not ("small": a chain of launches each as long as its
// longest pair, whatever the GPU could do meanwhile) over lanes nb .. nl-1, queued FIRST: they trickle into the tails
// of the big launches all along the plan instead of following the last of them one after the other (measured on
// MI355X, a 1250-locus plan: ten small launches of 0.3 - 3 ms each behind the last big one, 4.5 ms of 33).
// (level-2 timing: the single-class kernels have the same bodies)
Execute::Execute(ltr_plan* p, ltr_ctx* c, double* d_out_ll, void* stream_v)
    : plan(p), ctx(c), st(stream_v ? (hipStream_t)stream_v : c->stream), out(d_out_ll ? d_out_ll : p->d_ll), lanes{st, c->aux[2], c->aux[3], c->aux[1]},
      fan(plan->fan_lanes > 1 && !plan->timing && st != lanes[1] && st != lanes[2] && st != lanes[3]),
      nl(fan ? plan->fan_lanes : 1), nb(nl >= 4 ? 2 : nl), x_fan(exact_lists_fan_out(p, c)), list(plan->sched.at_level(plan->timing)) {}

// The kernel arguments every launch starts from: the plan's buffers, the model tables in force now, which first pass the
// workgroup classes get (sym, wg_thr, thr: set here and nowhere else, before the first launch).
int Execute::snapshot_tables() {
  int wg_learnt = 0;
  A.pairs = plan->d_pairs; A.index = nullptr; A.n_pairs_dev = nullptr; A.queue = nullptr;
  for (int c = 0; c < kNumExact; ++c) A.xlist[c] = plan->d_redo_list + (int64_t)c * plan->redo_cap;
  A.xcount = plan->d_redo_count;
  A.read_bytes = plan->d_reads; A.hap_bytes = plan->d_haps + kHapPad; A.hap_codes = plan->d_hap_codes + kHapPad;
  A.out_ll = out;
  {
    // (a plan being created on another thread may be rebuilding the model tables: snapshot them under the lock)
    std::lock_guard<std::mutex> lk(ctx->mu);
    A.lpc = ctx->d_lpc;
    A.colXZ = ctx->d_colXZ; A.row0XY = ctx->d_row0XY; A.thr_tab = ctx->d_thr; A.table_len = (int32_t)std::min<int64_t>(ctx->table_len + 1, 0x7fffffff);
    A.mc = ctx->mc;
    if (plan->uses_wg) { wg_stats_poll(ctx); wg_learnt = ctx->wg_thr_first; }
  }
  A.scratch = plan->d_scratch; A.scratch_stride = plan->scratch_stride;
  A.c_lo = 0; A.c_hi = 0x7fffffff; A.lp_shift = 6;
  A.mk_n = 0; A.queue_base = plan->d_queue; A.pk_tabs = nullptr; A.pk_ntabs = 0;
  A.pl_entries = nullptr; A.pl_n = 0; A.wave_clock = plan->d_wave_clock;
  for (int r = 0; r < kMultiMax; ++r) { A.mk_w[r] = kWMax; A.mk_first[r] = 0; A.mk_np[r] = 0; A.mk_class[r] = 0; }
  for (int r = 0; r < 5; ++r) { A.pk_shift[r] = kPackMaxShift; A.pk_first[r] = 0; A.pk_end[r] = 0; A.pk_grp_end[r] = 0; }
  sym = ltrp::symmetric_model(A.mc);
  // (what only the symmetric instances score: the workgroup classes, the families and the chained walk's entries, which the
  // general-model plan kernel would drain without scoring)
  const auto& ents = plan->sched.plan_entries;
  const bool chained = std::any_of(ents.begin(), ents.end(), [](const PlanEntry& e) { return e.kind == 3; });
  if ((plan->uses_wg || !plan->fams.empty() || chained) && !sym) {
    ltr::set_error(ctx, "the alignment parameters changed from a symmetric to an asymmetric indel model after this plan was created: create it again");
    return LTR_ERR_INVALID;
  }
  {
    const bool pen_ok = ltrp::band_in_table(A.mc.c);
    A.xlut = (plan->xlut && sym && pen_ok) ? 1 : 0;           // (parameters may have changed since the plan was binned: then everything goes to the generic exact kernel)
    A.thr_ok = pen_ok ? 1 : 0;                                 // (the threshold table is rebuilt with every parameter set: valid whenever it fits)
    if (!A.xlut) for (int c = 1; c < kNumExact; ++c) A.xlist[c] = A.xlist[kXGeneric];
  }
  // first pass of the workgroup classes: threshold kernels when the context has learnt that certificates fail here (or on request);
  // they need the threshold table (A.xlut)
  wg_thr = plan->uses_wg && A.xlut && (ctx->dbg.wg_first_pass == 2 || (ctx->dbg.wg_first_pass == 0 && wg_learnt != 0));
  if (wg_thr) thr = ltrp::threshold_groups(plan->bin_first, !plan->timing, ctx->dbg.wgt_keep_waves > 0);
  return LTR_OK;
}

int Execute::reset_control_words() {
  // the generic list starts as the non-ACGT pairs; the certificate kernels append to the lists
  // one D2D copy resets the work queues (zeros) and the redo count (= number of generic pairs)
  // (the plan's upload first: a compact plan's control-word image and list heads arrive with it -- the copies below read them)
  if (plan->ev_up) HIP_TRY(ctx, hipStreamWaitEvent(st, plan->ev_up, 0));
  if (plan->ctrl_fresh) plan->ctrl_fresh = false;               // (a compact plan's first execute: the control words came with the upload)
  else HIP_TRY(ctx, hipMemcpyAsync(plan->d_queue, plan->d_ctrl_init, kCtrlWords * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  for (int c = 0; c < kNumExact; ++c)
    if (plan->x_seed[c] > 0) {
      // (when the LUT exact kernels are off for this execute every list is the generic one: seeds pile up behind each other)
      int64_t at = 0;
      if (!A.xlut) for (int c2 = 0; c2 < c; ++c2) at += plan->x_seed[c2];
      HIP_TRY(ctx, hipMemcpyAsync(A.xlist[c] + at, plan->d_redo_init + (plan->bin_first[kNumFast + c] - plan->bin_first[kNumFast]),
                                  (size_t)plan->x_seed[c] * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
  if (plan->d_fam_stats) HIP_TRY(ctx, hipMemsetAsync(plan->d_fam_stats, 0, 4 * sizeof(uint32_t), st));
  if (!A.xlut) {
    // ... and the generic list's length is the sum of the seeds (one word, rewritten after the control block reset)
    uint32_t tot = 0;
    for (int c = 0; c < kNumExact; ++c) tot += (uint32_t)plan->x_seed[c];
    if (tot != (uint32_t)plan->x_seed[kXGeneric]) {
      plan->seed_total = tot;
      HIP_TRY(ctx, hipMemcpyAsync(plan->d_redo_count + kXGeneric, &plan->seed_total, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
  }
  return LTR_OK;
}

// The events of the exact launches on side streams (x_fan), once per plan.
int Execute::ensure_exact_events() {
  if (plan->ev_fast) return LTR_OK;
  // created into locals and published together: a failure half way must not leave the plan with ev_fast set and null events behind it
  hipEvent_t made[1 + (kNumExact + 1) + kNumExact * 4] = {nullptr};
  int n_made = 0;
  hipError_t e2 = hipSuccess;
  for (; n_made < (int)(sizeof(made) / sizeof(made[0])) && e2 == hipSuccess; ++n_made) e2 = hipEventCreateWithFlags(&made[n_made], hipEventDisableTiming);
  if (e2 != hipSuccess) {
    for (int i = 0; i < n_made; ++i) if (made[i]) (void)hipEventDestroy(made[i]);
    ltr::set_error(ctx, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(e2));
    return LTR_ERR_HIP;
  }
  int at = 1;
  for (int c = 0; c <= kNumExact; ++c) plan->ev_x[c] = made[at++];
  for (int c = 0; c < kNumExact; ++c) for (int k = 0; k < 4; ++k) plan->ev_close[c][k] = made[at++];
  plan->ev_fast = made[0];
  return LTR_OK;
}

// side stream of every exact launch (x_fan): short / mid / long / the W = 20 launch / four-wave / eight-wave; generic stays on st
hipStream_t Execute::exact_stream(int which) const {
  if (!x_fan || which == kXGeneric) return st;
  static const int kIdx[kNumExact + 1] = {-1, 4, 5, 6, 8, 9, 7};
  hipStream_t xs = ctx->aux[kIdx[which]];
  return xs == st ? st : xs;
}

// s2 waits for what every lane has queued so far
int Execute::behind_the_lanes(int c, hipStream_t s2, bool small_events) {
  if (s2 == st) return LTR_OK;
  for (int k = 0; k < nl; ++k) {
    // (big lanes: whatever is queued now; small lanes: the event recorded when their last feeder of this list was
    // queued -- or now, when the list stayed open to the end)
    if (k < nb || !small_events) HIP_TRY(ctx, hipEventRecord(plan->ev_close[c][k], lanes[k]));
    HIP_TRY(ctx, hipStreamWaitEvent(s2, plan->ev_close[c][k], 0));
  }
  return LTR_OK;
}

// one exact list: launched on its side stream behind the certificate launches queued so far on every lane (x_fan), or
// on the plan's stream
int Execute::launch_exact_list(int c, bool small_events) {
  x_done[c] = true;
  const bool usable = (c == kXGeneric) || A.xlut;
  const int grid = (c == kXGeneric && !A.xlut) ? std::max(plan->sched.x_grid[c], (plan->n_pairs > 0) ? 1 : 0) : plan->sched.x_grid[c];
  if (!(usable && grid > 0 && plan->n_pairs > 0)) return LTR_OK;
  KernelArgs X = A;
  X.first_pair = 0; X.n_pairs = 0; X.index = A.xlist[c]; X.n_pairs_dev = plan->d_redo_count + c;
  X.queue = plan->d_queue + kNumFast + c;
  X.scratch = plan->d_scratch; X.c_lo = 0; X.c_hi = 0x7fffffff; X.lp_shift = 6;
  const dim3 g((unsigned)grid);
  hipStream_t xs = exact_stream(c);
  int rc2;
  if ((rc2 = behind_the_lanes(c, xs, small_events)) != LTR_OK) return rc2;
  if (c == kXWg4) {
    // the list of 1026 .. 3585-base reads is worked off by two launches: reads that fit one wavefront's widest
    // strips (<= 1281 bases) by the one-wave exact kernel with W = 20 -- 0.8e12 cells/s on four-wave workgroups
    // (W = 5) in round 2a -- the rest by the workgroup kernel; each skips the other's pairs (c_lo / c_hi)
    KernelArgs B = X;
    B.queue = plan->d_queue + kNumKernels;                   // (a queue word of its own: zeroed with the others)
    B.c_hi = 64 * kXWideW;
    const int gw = std::max(1, std::min(ctx->full_x_wide_grid, plan->sched.max_grid_wide));
    hipStream_t ws = exact_stream(kNumExact);
    if (ws != xs && (rc2 = behind_the_lanes(c, ws, small_events)) != LTR_OK) return rc2;
    ltrk::launch_exact(ltrk::kXWideLaunch, sym, dim3((unsigned)gw), ws, B);
    note(kNoteExactWide, c, gw, kBlockWaves, -1);
    if (ws != st) {
      HIP_TRY(ctx, hipEventRecord(plan->ev_x[kNumExact], ws));
      HIP_TRY(ctx, hipStreamWaitEvent(st == xs ? st : xs, plan->ev_x[kNumExact], 0));     // (joined through the list's own stream / event below)
    }
    X.c_lo = 64 * kXWideW + 1;
    ltrk::launch_exact(c, sym, g, xs, X);
    note(kNoteExact, c, grid, 1, -1);
  } else if (c == kXWg8) {
    // the list of 3586 .. 10241-base reads, two launches that skip each other's pairs: reads of up to 5121 bases on strips of
    // 10 columns at four waves per SIMD (the threshold bodies fit 128 registers up to there), the longer ones on 12 / 16 / 20
    // columns at three.  ONE AFTER THE OTHER on the list's stream, the long pairs first: side by side they do not share a CU
    // (an eight-wave workgroup of 168 registers leaves room for four waves of 128, not for eight), each kernel keeps half-empty
    // CUs from the other, and the pass takes longer than the two alone (rocprofv3 per dispatch, config5hifi through the lists:
    // 5.7 ms + 21 ms alone, 40 ms side by side: profiles/r06/pmc_dispatch_config5hifi_exact.txt)
    KernelArgs B = X;
    B.queue = plan->d_queue + kNumKernels + 1;               // (a queue word of its own: zeroed with the others)
    B.c_hi = ltrk::kXWg8NarrowMaxC;
    X.c_lo = ltrk::kXWg8NarrowMaxC + 1;
    // (the narrow launch IS the first-pass threshold kernel of 10-column strips, given the list: one strip width in the function --
    // a kernel of its own with an 8- and a 10-column body spilled inside its step loops, 5.7 GB of scratch writes and 30 ms per
    // config5hifi pass against 21 ms for the same pairs: profiles/r06/pmc_dispatch_config5hifi_*.txt)
    const int gn = capped(std::max(1, std::min(ctx->full_wgt_grid[1][10], grid * 2)));
    ltrk::launch_exact(c, sym, g, xs, X);
    note(kNoteExact, c, grid, 1, -1);
    ltrk::launch_wgt(8, 10, dim3((unsigned)gn), xs, B);
    note(kNoteExactNarrow8, c, gn, 1, -1);
  } else {
    // kXLong walks the column blocks of reads beyond the eight-wave workgroups' 10241 bases through scratch strips and
    // may run beside the generic exact kernel (which does the same for non-ACGT pairs): a strip region of its own
    if (c == kXLong) X.scratch = plan->d_scratch + (size_t)plan->fan_lanes * plan->scratch_lane_stride;
    ltrk::launch_exact(c, sym, g, xs, X);
    note(kNoteExact, c, grid, kBlockWaves, -1);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (xs != st) HIP_TRY(ctx, hipEventRecord(plan->ev_x[c], xs));
  x_launched[c] = true;
  LTR_DBG("launched exact kernel %d grid %d", c, grid);
  ++launches;
  return LTR_OK;
}

int Execute::launch_class(const Launch& L, int li) {
  const int k = L.cls;
  int np = plan->bin_first[k + 1] - plan->bin_first[k];
  if (wg_thr && thr.nw[k] != 0) { if (thr.np[k] == 0) return LTR_OK; np = thr.np[k]; }      // (scored by the launch of the class that leads its group)
  A.first_pair = plan->bin_first[k]; A.n_pairs = np; A.queue = plan->d_queue + k;
  const dim3 grid((unsigned)L.grid);
  hipStream_t ls = lanes[li];
  A.scratch = plan->d_scratch + (size_t)li * plan->scratch_lane_stride;
  A.lp_shift = class_info(k).lp_shift;
  switch (L.kind) {
    case kLaunchPlan:                                          // (either model: the launch picks the instance of the parameters in force now)
      A.pl_entries = plan->d_pl_entries; A.pl_n = (int32_t)plan->sched.plan_entries.size();
      [[fallthrough]];
    case kLaunchPackMulti:
      A.pk_tabs = plan->d_pk_tabs; A.pk_ntabs = (int32_t)plan->sched.pack_tabs.size(); A.queue_base = plan->d_queue;
      if (L.kind == kLaunchPlan) ltrk::launch_plan(sym, grid, ls, A); else ltrk::launch_pack_multi(sym, grid, ls, A);
      break;
    case kLaunchMulti:
      A.mk_n = L.n_one; A.queue_base = plan->d_queue;
      for (int r = 0; r < L.n_one; ++r) {                      // widest strips first
        const int k2 = L.members[r];
        A.mk_w[r] = class_info(k2).W; A.mk_first[r] = plan->bin_first[k2]; A.mk_np[r] = plan->bin_first[k2 + 1] - plan->bin_first[k2]; A.mk_class[r] = k2;
      }
      ltrk::launch_multi(sym, grid, ls, A);
      break;
    case kLaunchOne: ltrk::launch_onewave(L.W, sym, grid, ls, A); break;
    case kLaunchFamily: {
      FamilyArgs FA;
      FA.fams = plan->d_fams; FA.n_fams = (int32_t)plan->fams.size(); FA.reserved = 0; FA.park = plan->d_fam_park; FA.stats = plan->d_fam_stats; FA.spines = plan->d_fam_spines;
      FA.wave_clock = plan->d_fam_wave_clock; plan->fam_clock_waves = L.grid * kBlockWaves;
      ltrk::launch_family(grid, ls, A, FA);
      break;
    }
    case kLaunchPack:
      ltrp::pack_ranges(plan->bin_first, L.W, A.pk_shift, A.pk_first, A.pk_end, A.pk_grp_end);
      ltrk::launch_pack(L.W, sym, grid, ls, A);
      break;
    default:
      if (wg_thr && thr.nw[k] != 0) {
        // (all of them on the plan's own stream, one after the other: two persistent eight-wave launches of different register
        // budgets side by side keep half-empty CUs from each other -- config5hifi, thresholds first: 21 + 12 ms alone, 41 ms side by side)
        const int gt = capped(std::max(1, std::min(np, ctx->full_wgt_grid[thr.nw[k] == 8 ? 1 : 0][thr.w[k]])));
        ltrk::launch_wgt(thr.nw[k], thr.w[k], dim3((unsigned)gt), lanes[0], A);
        note(kNoteThreshold, k, gt, 1, np);
      } else ltrk::launch_wg(class_info(k).waves, L.W, grid, ls, A);
  }
  if (L.kind == kLaunchFamily) note(L.kind, k, L.grid, kBlockWaves, (int64_t)plan->fams.size());
  else if (L.kind != kLaunchWg) note(L.kind, k, L.grid, kBlockWaves, L.pairs);
  else if (!(wg_thr && thr.nw[k] != 0)) note(L.kind, k, L.grid, 1, np);
  HIP_TRY(ctx, hipGetLastError());
  LTR_DBG("launched class %d grid %d pairs %d on lane %d", k, L.grid, np, li);
  ++launches;
  return LTR_OK;
}

// what this execute's workgroup classes met -> a pinned slot the next execute reads (no wait here, none there)
void Execute::note_wg_stats() {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->wg_stat_pin && hipHostMalloc((void**)&ctx->wg_stat_pin, ltr_ctx::kWgStatSlots * 2 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { ctx->wg_stat_pin = nullptr; (void)hipGetLastError(); }
  if (ctx->wg_stat_pin)
    for (int i = 0; i < ltr_ctx::kWgStatSlots; ++i) {
      ltr_ctx::WgStatSlot& sl = ctx->wg_stat[i];
      if (sl.busy) continue;
      if (!sl.ev && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) { sl.ev = nullptr; (void)hipGetLastError(); break; }
      if (hipMemcpyAsync(ctx->wg_stat_pin + 2 * i, plan->d_redo_count + kWgStatOff, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
          hipEventRecord(sl.ev, st) == hipSuccess) { sl.busy = true; sl.mode = wg_thr ? 1 : 0; sl.epoch = ctx->wg_epoch; }
      else (void)hipGetLastError();
      break;
    }
}

// snapshot tables -> reset -> fork lanes -> small classes -> big classes with their exact lists -> join -> remaining lists -> join -> record
int Execute::run() {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  plan->launch_log.clear();
  if ((rc = snapshot_tables()) != LTR_OK || (rc = reset_control_words()) != LTR_OK) return rc;
  HIP_TRY(ctx, hipEventRecord(plan->ev0, st));
  // Launch order: the first-pass launches longest reads first (ltrp::build_schedule), then the exact kernels; with per-launch
  // timing, launch number o runs between bin_ev[o] and bin_ev[o+1].
  // (The classes are independent and every launch ends in a tail in which only its longest pairs still run: the
  // launches alternate between two streams, see ltr_plan_create.)
  int o = 0;
  if (plan->timing) HIP_TRY(ctx, hipEventRecord(plan->bin_ev[o], st));
  if (fan) {
    HIP_TRY(ctx, hipEventRecord(plan->ev_fork, st));
    for (int k = 1; k < nl; ++k) HIP_TRY(ctx, hipStreamWaitEvent(lanes[k], plan->ev_fork, 0));
  }
  if (x_fan && (rc = ensure_exact_events()) != LTR_OK) return rc;
  std::vector<const Launch*> big, small;                        // both longest reads first
  for (const Launch& L : list) ((nl > nb && L.small) ? small : big).push_back(&L);
  // the small classes first, on their own lanes; per exact list an event on each of those lanes once nothing small still
  // to come can feed it
  bool small_closed[kNumExact] = {false};
  for (size_t p = 0; p < small.size(); ++p) {
    const int rc2 = launch_class(*small[p], nb + (int)(p % (size_t)(nl - nb)));
    if (rc2 != LTR_OK) return rc2;
    if (x_fan && A.xlut) {
      const int next_cmax = (p + 1 < small.size()) ? small[p + 1]->cmax : -1;
      for (int c = kNumExact - 1; c > kXShort; --c)
        if (!small_closed[c] && next_cmax < kListMinC[c]) {
          small_closed[c] = true;
          for (int k = nb; k < nl; ++k) HIP_TRY(ctx, hipEventRecord(plan->ev_close[c][k], lanes[k]));
        }
    }
  }
  size_t rr = 0;
  for (size_t p = 0; p < big.size(); ++p) {
    // (round-robin; giving every launch to the stream with less work queued so far measured 0.4 % slower)
    // (the family launch and the launch behind it -- the plan kernel -- share a stream: two persistent launches side by side would
    // halve each other's wave slots from the start)
    const int rc2 = launch_class(*big[p], (int)(rr % (size_t)nb));
    if (big[p]->kind != kLaunchFamily) ++rr;
    if (rc2 != LTR_OK) return rc2;
    if (plan->timing) HIP_TRY(ctx, hipEventRecord(plan->bin_ev[++o], st));
    // exact lists nothing still to come can feed: the next class holds only shorter reads than the list takes
    if (x_fan && A.xlut) {
      const int next_cmax = (p + 1 < big.size()) ? big[p + 1]->cmax : -1;
      for (int c = kNumExact - 1; c > kXShort; --c)
        if (!x_done[c] && next_cmax < kListMinC[c] && next_cmax >= 0) { const int rc3 = launch_exact_list(c, small_closed[c]); if (rc3 != LTR_OK) return rc3; }
    }
  }
  if (fan)
    for (int k = 1; k < nl; ++k) {
      HIP_TRY(ctx, hipEventRecord(plan->ev_join[k - 1], lanes[k]));
      HIP_TRY(ctx, hipStreamWaitEvent(st, plan->ev_join[k - 1], 0));
    }
  A.scratch = plan->d_scratch;
  // the lists still open (x_fan: the short reads' and the generic one; else all of them), in list order
  for (int c = 0; c < kNumExact; ++c) {
    if (!x_done[c]) { const int rc2 = launch_exact_list(c, false); if (rc2 != LTR_OK) return rc2; }
    if (plan->timing) HIP_TRY(ctx, hipEventRecord(plan->bin_ev[++o], st));
  }
  // ... and the plan's stream joins the side streams
  if (x_fan)
    for (int c = 0; c < kNumExact; ++c) if (exact_stream(c) != st && x_launched[c]) HIP_TRY(ctx, hipStreamWaitEvent(st, plan->ev_x[c], 0));
  HIP_TRY(ctx, hipEventRecord(plan->ev1, st));
  if (plan->uses_wg && ctx->dbg.wg_first_pass == 0) note_wg_stats();
  plan->last_wg_thr = wg_thr;
  plan->last_out = out; plan->last_stream = st; plan->last_launches = launches; plan->executed = true;
  if (std::find(plan->streams.begin(), plan->streams.end(), st) == plan->streams.end()) plan->streams.push_back(st);
  plan->timed = plan->sched.plan_launch() ? std::min(plan->timing, 1) : plan->timing;     // (the plan kernel is never split: its launches were timed as launched)
  plan->kernel_ms_counted = false;
  return LTR_OK;
}

}  // namespace

extern "C" {

int ltr_ctx_wg_first_pass(ltr_ctx* ctx, int64_t* last_unfinished, int64_t* last_scored) {
  if (!ctx) return LTR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  // (the query waits for the statistics of the executes queued so far -- ltr_plan_execute itself never does)
  for (ltr_ctx::WgStatSlot& sl : ctx->wg_stat) if (sl.busy && sl.ev) (void)hipEventSynchronize(sl.ev);
  wg_stats_poll(ctx);
  if (last_unfinished) *last_unfinished = ctx->wg_last_unfinished;
  if (last_scored) *last_scored = ctx->wg_last_scored;
  return ctx->dbg.wg_first_pass == 1 ? 0 : (ctx->dbg.wg_first_pass == 2 ? 1 : ctx->wg_thr_first);
}

int ltr_plan_execute(ltr_plan* plan, double* d_out_ll, void* stream_v) {
  if (!plan) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  // (no exception crosses the C-ABI: the launch-order lists are host vectors)
  try { return Execute(plan, ctx, d_out_ll, stream_v).run(); }
  catch (const std::bad_alloc&) { ltr::set_error(ctx, "out of host memory"); return LTR_ERR_NOMEM; }
  catch (const std::exception& e_) { ltr::set_error(ctx, std::string("internal error: ") + e_.what()); return LTR_ERR_INVALID; }
  catch (...) { ltr::set_error(ctx, "internal error"); return LTR_ERR_INVALID; }
}

int ltr_plan_fetch(ltr_plan* plan, double* out_ll, int32_t* out_seed) {
  if (!plan || !plan->executed) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LTR_DBG("fetch: waiting");
  HIP_TRY(ctx, hipEventSynchronize(plan->ev1));               // this plan's last execute (work queued behind it on the stream keeps running)
  LTR_DBG("fetch: plan done");
  if (!plan->kernel_ms_counted) {                              // device time of this execute's DP kernels -> the context's timers
    float t = 0.f;
    if (hipEventElapsedTime(&t, plan->ev0, plan->ev1) == hipSuccess) ltr::add_time(ctx, -1, 0.0, (double)t);
    { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->tm.dp_cells += ltr_plan_cells(plan); ctx->tm.dp_pairs += ltr_plan_num_pairs(plan); }
    plan->kernel_ms_counted = true;
  }
  if (out_ll && plan->ll_size > 0 && plan->h_ll && plan->last_out == plan->d_ll) {
    // a compact plan: the kernel wrote into pinned host memory, visible now that ev1 has passed
    std::memcpy(out_ll, plan->h_ll, (size_t)plan->ll_size * sizeof(double));
  } else if (out_ll && plan->ll_size > 0) {
    // Through a pinned staging block on a copy stream of its own: hipMemcpy into pageable memory is done by a copy KERNEL,
    // and behind the persistent DP launches of later plans it waited for wave slots -- measured on MI355X, the three chunks of
    // a 30 000-locus ltr_calc_hap_aln_probs call: the 2 MB of chunk 0 arrived 8 ms after its plan had finished, when chunks
    // 1 and 2 were through as well.  A pinned destination goes over the DMA engines.
    std::lock_guard<std::mutex> lk(ctx->pin_mu);
    const size_t total = (size_t)plan->ll_size * sizeof(double);
    const size_t block = std::min<size_t>(total, (size_t)8 << 20);      // (8 MB pieces: a 10 000-locus plan's 12 MB already takes two)
    if (ctx->pin_bytes < block) {
      if (ctx->pin) (void)hipHostFree(ctx->pin);
      ctx->pin = nullptr; ctx->pin_bytes = 0;
      HIP_TRY(ctx, hipHostMalloc(&ctx->pin, block, hipHostMallocDefault));
      ctx->pin_bytes = block;
    }
    if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (size_t at = 0; at < total; at += block) {
      const size_t nb = std::min(block, total - at);
      HIP_TRY(ctx, hipMemcpyAsync(ctx->pin, (const char*)plan->last_out + at, nb, hipMemcpyDeviceToHost, ctx->copy_stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
      std::memcpy((char*)out_ll + at, ctx->pin, nb);
    }
  }
  if (out_seed)
    for (int64_t r = 0; r < plan->n_reads; ++r) if (plan->seed[(size_t)r] >= 0) out_seed[r] = plan->seed[(size_t)r];
  return LTR_OK;
}

int ltr_plan_last_kernel_ms(ltr_plan* plan, float* ms, int* n_launches) {
  if (!plan || !plan->executed) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  HIP_TRY(ctx, hipEventSynchronize(plan->ev1));
  float t = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&t, plan->ev0, plan->ev1));
  if (ms) *ms = t;
  if (n_launches) *n_launches = plan->last_launches;
  return LTR_OK;
}

int ltr_plan_set_timing(ltr_plan* plan, int on) {
  if (!plan) return LTR_ERR_INVALID;
  if (!plan->ctx) return LTR_ERR_INVALID;                     // the context was destroyed before this plan
  if (on && !plan->bin_ev[0]) {
    ltr_ctx* ctx = plan->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k <= kNumKernels; ++k) HIP_TRY(ctx, hipEventCreate(&plan->bin_ev[k]));
  }
  plan->timing = on <= 0 ? 0 : (on >= 2 ? 2 : 1);
  return LTR_OK;
}

int ltr_plan_kernel_stats(ltr_plan* plan, int k, int* strip_width, int64_t* n_pairs, double* cells, float* ms) {
  if (!plan || k < 0 || k >= kNumKernels) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  const bool redo = (k >= kNumFast);
  const int xc = k - kNumFast;
  static_assert(kNumKernels == kNumFast + kNumExact, "the classes behind the certificate classes are the exact lists");
  if (strip_width) *strip_width = redo ? kXW[xc] : class_info(k).W;
  // a launch that scores several classes -- every lanes-per-pair block of a packed strip width, a multi-width launch, the plan
  // kernel -- reports its pairs, cells and time under the class it is listed under (ltr_plan_kernel_ranges names the classes),
  // its other classes report nothing; launch number o ran between bin_ev[o] and bin_ev[o+1] (see ltr_plan_execute)
  const std::vector<Launch>& list = plan->sched.at_level(plan->timed);
  const int o = redo ? (int)list.size() + xc : Schedule::find(list, k);
  if (cells) *cells = redo ? plan->stats.x_cells[xc] : (o >= 0 ? list[(size_t)o].cells : 0.0);
  if (n_pairs) {
    *n_pairs = (redo || o < 0) ? 0 : list[(size_t)o].pairs;
    if (redo && plan->executed) {                      // pairs the certificates could not clear (+ the non-ACGT ones, generic list)
      uint32_t c[kInlineCountOff + kNumExact] = {0};
      HIP_TRY(ctx, hipStreamSynchronize(plan->last_stream));
      HIP_TRY(ctx, hipMemcpy(c, plan->d_redo_count, sizeof(c), hipMemcpyDeviceToHost));
      *n_pairs = (int64_t)c[xc] + c[kInlineCountOff + xc];      // its list + what the plan kernel scored in line for it
    }
  }
  if (ms) {
    *ms = 0.f;
    if (plan->executed && plan->timed && o >= 0) {
      HIP_TRY(ctx, hipEventSynchronize(plan->bin_ev[o + 1]));
      HIP_TRY(ctx, hipEventElapsedTime(ms, plan->bin_ev[o], plan->bin_ev[o + 1]));
    }
  }
  return LTR_OK;
}

int ltr_plan_kernel_ranges(ltr_plan* plan, int k, int32_t* lanes_per_pair, int32_t* strip_width, int64_t* n_pairs) {
  if (!plan || k < 0 || k >= kNumKernels) return LTR_ERR_INVALID;
  const std::vector<Launch>& list = plan->sched.at_level(plan->timed);
  const int o = Schedule::find(list, k);
  return o < 0 ? 0 : plan->sched.ranges(list[(size_t)o], plan->bin_first, lanes_per_pair, strip_width, n_pairs);
}

int ltr_plan_family_stats(ltr_plan* plan, int64_t* out5) {
  if (!plan || !out5) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  out5[0] = (int64_t)plan->fams.size(); out5[1] = plan->fam_members; out5[2] = out5[3] = out5[4] = 0;
  if (plan->executed && plan->d_fam_stats) {
    uint32_t c[4] = {0};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(plan->last_stream));
    HIP_TRY(ctx, hipMemcpy(c, plan->d_fam_stats, sizeof(c), hipMemcpyDeviceToHost));
    out5[2] = c[0]; out5[3] = c[1]; out5[4] = c[2];
  }
  return LTR_OK;
}

int ltr_plan_family_spine_stats(const ltr_plan* plan, int64_t* out2) {
  if (!plan || !out2) return LTR_ERR_INVALID;
  out2[0] = plan->fam_with_spine; out2[1] = plan->fam_rows_saved;
  return LTR_OK;
}

int ltr_plan_kernel_class(const ltr_plan* plan) {
  const Launch* P = plan ? plan->sched.plan_launch() : nullptr;
  return P ? P->cls : -1;
}

int ltr_plan_debug_entries(const ltr_plan* plan, int32_t* kind, int32_t* strip_width, int64_t* n_pairs, double* cells, int cap) {
  if (!plan || cap < 0) return LTR_ERR_INVALID;
  const int n = (int)plan->sched.plan_entries.size();
  for (int i = 0; i < std::min(n, cap); ++i) {
    const PlanEntry& e = plan->sched.plan_entries[(size_t)i];
    int64_t np = e.n_pairs; double cl = 0.0;
    if (e.kind == 2) cl = plan->stats.x_cells[e.queue_class - ltrp::kStartQueueSlot];
    else {                                                       // (a class, or a packed width: what its own launch would report)
      const Launch& L = plan->sched.by_class[(size_t)Schedule::find(plan->sched.by_class, e.queue_class)];
      np = L.pairs; cl = L.cells;
    }
    if (kind) kind[i] = e.kind;
    if (strip_width) strip_width[i] = e.W;
    if (n_pairs) n_pairs[i] = np;
    if (cells) cells[i] = cl;
  }
  return n;
}

int ltr_debug_last_launches(const ltr_plan* plan, ltr_ctx* ctx, int cap, int64_t* out) {
  if ((!plan && !ctx) || cap < 0 || (cap > 0 && !out)) return LTR_ERR_INVALID;
  if (plan && (!plan->ctx || !plan->executed)) return LTR_ERR_INVALID;
  std::vector<ltrp::LaunchNote> log;
  try {
    if (plan) log = plan->launch_log;
    else { std::lock_guard<std::mutex> lk(ctx->err_mu); log = ctx->nw_log; }
  } catch (...) { return LTR_ERR_NOMEM; }
  for (size_t i = 0; i < log.size() && i < (size_t)cap; ++i) {
    const int64_t v[5] = {log[i].kind, log[i].cls, log[i].grid, log[i].takers, log[i].items};
    std::memcpy(out + i * 5, v, sizeof(v));
  }
  return (int)log.size();
}

int ltr_plan_debug_wave_clocks(ltr_plan* plan, uint64_t* out, int64_t cap) {
  if (!plan || !plan->ctx || !out || cap < 0) return LTR_ERR_INVALID;
  if (!plan->d_wave_clock || !plan->executed) return 0;
  ltr_ctx* ctx = plan->ctx;
  const int64_t n = (int64_t)plan->sched.plan_launch()->grid * kBlockWaves;
  if (cap < 4 * n + 4096 + 256) return LTR_ERR_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(plan->last_stream));
  HIP_TRY(ctx, hipMemcpy(out, plan->d_wave_clock, ((size_t)n * 4 + 4096 + 256) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemset(plan->d_wave_clock + 4 * n, 0, sizeof(uint64_t)));      // (the log's counter, for the next execute)
  HIP_TRY(ctx, hipMemset(plan->d_wave_clock + 4 * n + 4096, 0, 256 * sizeof(uint64_t)));   // (... and the per-entry sums)
  return (int)n;
}

int ltr_debug_family_wave_clocks(ltr_plan* plan, uint64_t* out, int64_t cap) {
  if (!plan || !plan->ctx || !out || cap < 0) return LTR_ERR_INVALID;
  if (!plan->d_fam_wave_clock || !plan->executed || plan->fam_clock_waves <= 0) return 0;
  ltr_ctx* ctx = plan->ctx;
  const int64_t n = plan->fam_clock_waves;
  if (cap < 2 * n) return LTR_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(plan->last_stream));
  HIP_TRY(ctx, hipMemcpy(out, plan->d_fam_wave_clock, (size_t)n * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return (int)n;
}

int ltr_align_batch(ltr_ctx* ctx, const ltr_locus_batch* batch, double* out_ll, int32_t* out_seed) {
  if (!ctx || !batch || !out_ll) return LTR_ERR_INVALID;
  ltr::TimedCall timed(ctx, ltr::kTimerHapAln);
  LTR_GUARD_BEGIN
  ltr_plan* plan = nullptr;
  int rc = ltr_plan_create(ctx, batch, &plan);
  if (rc != LTR_OK) return rc;
  // Masked cells must stay untouched (reference HapAligner.cpp:557-560, :841-845): results go
  // through a staging copy and only the computed entries are scattered into the caller's buffer.
  std::vector<double> tmp((size_t)std::max<int64_t>(plan->ll_size, 1));
  rc = ltr_plan_execute(plan, nullptr, nullptr);
  if (rc == LTR_OK) rc = ltr_plan_fetch(plan, tmp.data(), out_seed);
  if (rc == LTR_OK) {
    if (!batch->realign_read && !batch->realign_hap) {
      std::memcpy(out_ll, tmp.data(), (size_t)plan->ll_size * sizeof(double));
    } else {
      int64_t off = 0;
      for (int64_t l = 0; l < batch->n_loci; ++l) {
        const int64_t r0 = batch->locus_read_off[l], r1 = batch->locus_read_off[l + 1];
        const int64_t h0 = batch->locus_hap_off[l], h1 = batch->locus_hap_off[l + 1];
        const int64_t H = h1 - h0;
        for (int64_t r = r0; r < r1; ++r) {
          if (batch->realign_read && !batch->realign_read[r]) continue;
          for (int64_t h = h0; h < h1; ++h) {
            if (batch->realign_hap && !batch->realign_hap[h]) continue;
            const int64_t k = off + (r - r0) * H + (h - h0);
            out_ll[k] = tmp[(size_t)k];
          }
        }
        off += (r1 - r0) * H;
      }
    }
  }
  ltr_plan_destroy(plan);
  return rc;
  LTR_GUARD_END(ctx)
}

}  // extern "C"
