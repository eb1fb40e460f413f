// ltr_ctx.h -- the context and the plan as the units that implement them see them: ltr_ctx.hip (context, model tables, caches),
// ltr_plan_build.hip (ltr_plan_create / _destroy), ltr_plan_run.hip (execute, fetch, statistics) and the consumers of a plan's
// scores, ltr_posterior.hip, ltr_plan_genotype.hip, ltr_plan_fields.hip.
// Private to those six: everything else (ltr_host.cpp, ltr_short.hip, ltr_nw.hip, ..) goes through the ltr::ctx_* accessors
// of ltr_internal.h, which is what lets tests/host_sanitize/harness.cpp supply a context of its own.  The lease a call holds its
// device blocks and events by (ltr_lease.h) is seen by these six and by ltr_short.hip and ltr_nw.hip, which hand it the context.
#ifndef LTR_CTX_H_
#define LTR_CTX_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "ltr_internal.h"
#include "ltr_kernels.h"
#include "ltr_lease.h"
#include "ltr_plan.h"

// (DevPool, DevLease, DEV_TRY: ltr_lease.h.  RawBuf, the grow-only host array of the work arrays below: ltr_plan.h)
struct ltr_ctx {
  int device = -1;
  DevPool pool;
  std::set<ltr_plan*> plans;            // plans created on this context and not destroyed yet (under mu)
  // host work arrays of ltr_plan_create (used under mu) and the chunk staging bytes of ltr_calc_hap_aln_probs
  struct PlanScratch {
    RawBuf<PairDesc> pairs, sorted; RawBuf<int16_t> key, bin; RawBuf<int32_t> order; RawBuf<uint8_t> read_acgt, hap_acgt;
  } scratch;
  RawBuf<uint8_t> gt_units;             // host work array of ltr_plan_genotype (used under mu): the units of the first pass
  RawBuf<uint8_t> host_bytes[4];         // (two pairs: the chunks of ltr_calc_hap_aln_probs alternate, one is laid out while the other is uploaded)
  void* d_big = nullptr; size_t big_bytes = 0;      // ctx_big_scratch
  hipStream_t stream = nullptr;
  hipStream_t up_stream = nullptr;      // device-side input preparation of new plans (never behind another plan's DP kernels)
  static constexpr int kAux = 10;
  hipStream_t aux[kAux] = {};          // side streams: independent plans (the chunks of ltr_calc_hap_aln_probs) run side by side
  ltr_align_params params;
  ltr_stutter_params stutter;
  ModelConsts mc;
  // device model tables
  int64_t table_len = 0;
  double* d_lpc = nullptr;
  double* d_colXZ = nullptr;
  double* d_thr = nullptr;               // exact row-test thresholds of the LUT exact kernels (ltrp::build_threshold_table)
  double* d_row0XY = nullptr;            // first row: record j = {X(0,j), Y(0,j)} for emit(hap[j], read[0]) = mismatch, match (packed kernels)
  std::string arch;
  int n_cu = 0, clock_mhz = 0;
  int pair_packing = -1;                // two pairs per wavefront: -1 by batch size, 0 never, 1 whenever the read fits
  // resident workgroups per launch class (occupancy x CUs), asked from the runtime once per context
  bool have_grids = false;
  int full_grid[ltrp::kNumFast] = {0};
  int full_multi_grid = 0;              // the multi-width one-wave launch
  int full_pmulti_grid = 0;             // ... packed launch
  int full_plan_grid = 0;               // the plan kernel
  int full_x_wide_grid = 0;             // the W = 20 exact kernel (reads of 1026 .. 1281 bases out of the 4-wave list)
  int full_wgt_grid[2][kWgWMax + 1] = {{0}};   // threshold kernels as the first pass of a workgroup class: [0] four waves, [1] eight, by (even) strip width
  int full_redo_grid = 0;               // ... of the exact kernels
  int full_x_grid[kNumExact] = {0};
  ltr::DebugKnobs dbg;                  // ltr_ctx_set_debug
  // First pass of the workgroup classes (ltr_dp_wg.hpp): certificate kernels (11 operations a cell; a pair whose certificate
  // fails is scored a second time by an exact kernel) or threshold kernels (13 operations, exact in one pass).  Which one pays
  // depends on the READS -- HiFi reads finish, ONT reads under the default model abort (every pair of BASELINE config 5) -- so
  // the context learns it: every execute leaves {pairs the first pass could not finish, pairs it scored} of its workgroup
  // classes in a pinned slot, and the next execute reads the slots that have arrived (wg_stats_poll; never a wait).
  struct WgStatSlot { hipEvent_t ev = nullptr; bool busy = false; int mode = 0; int epoch = 0; };
  static constexpr int kWgStatSlots = 8;
  WgStatSlot wg_stat[kWgStatSlots];
  uint32_t* wg_stat_pin = nullptr;      // kWgStatSlots x 2 words, pinned
  int wg_thr_first = 0;                 // 1: the threshold kernels go first
  int wg_epoch = 0;                     // bumped by ltr_ctx_set_params: slots of the old model are ignored
  uint32_t wg_last_unfinished = 0, wg_last_scored = 0;     // the last slot read (ltr_ctx_wg_first_pass)
  std::string err;
  std::mutex mu;
  std::mutex pin_mu;                    // the pinned download block below (ltr_plan_fetch)
  void* pin = nullptr; size_t pin_bytes = 0;
  hipStream_t copy_stream = nullptr;
  // compact plans: the pinned image the host fills (one at a time: compact_ev = the copy out of it), recycled events, recycled
  // pinned blocks for the scores (hipEventCreate / hipHostMalloc per one-locus call would cost more than the call's kernel)
  RawBuf<uint8_t> compact_stage;
  hipEvent_t compact_ev = nullptr; bool compact_ev_pending = false;
  std::mutex cache_mu;
  std::vector<hipEvent_t> ev_cache[2];  // [0]: hipEventDisableTiming, [1]: timing
  struct PinBlock { void* p; void* dev; size_t cap; bool busy; };     // dev: the address the device reaches it by
  std::vector<PinBlock> pin_blocks;
  std::mutex call_mu;                   // one ltr_calc_hap_aln_probs / NW call at a time per context: they stage in host_bytes / d_big (ctx_call_lock)
  std::mutex err_mu;                    // error text and timers are written from worker threads too
  ltr_timers tm = {};
  std::vector<ltrp::LaunchNote> nw_log;   // the class launches of the last ltr_haplotype_align_to_ref as made (under err_mu; ltr_debug_last_launches)
  double short_split_ms[4] = {0, 0, 0, 0};   // ltr_ctx_set_debug "short_split": [prep + flank rows before the block, block row, flank rows after, seed log-sum]
};


constexpr int kReadPad = 1024;                  // bytes behind the device read buffer: a packed kernel's lane loads its strip (up to 641 + 24 bytes past a read's start) unclamped
constexpr size_t kCompactImageMax = (size_t)1 << 20;   // a plan whose device image (control words, tables, pairs, reads, haplotypes + codes) is at most this is uploaded as ONE block (ltr_plan_create)
constexpr size_t kCompactLlMax = (size_t)256 << 10;    // ... and its scores go straight into pinned host memory
constexpr int kHapPad = 96;                     // zero bytes either side of the device haplotype buffer

#define HIP_TRY(ctx, call)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      ltr::set_error(ctx, std::string(#call) + ": " + hipGetErrorString(e_));                \
      return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? LTR_ERR_NO_DEVICE : LTR_ERR_HIP; \
    }                                                                                        \
  } while (0)

struct ltr_plan : ltrp::BatchPlan {     // (what ltrp::describe_batch decided: sizes, class ranges, per-locus layout)
  ltr_ctx* ctx = nullptr;
  int64_t n_reads = 0;
  // device buffers
  uint8_t* d_reads = nullptr; uint8_t* d_haps = nullptr; uint16_t* d_hap_codes = nullptr;
  PairDesc* d_pairs = nullptr;
  double* d_ll = nullptr;
  uint32_t* d_queue = nullptr;          // one counter per bin
  double* d_scratch = nullptr;
  int32_t scratch_stride = 0;
  ltrp::ClassStats stats;               // nominal cells and longest read of every class
  ltrp::Schedule sched;                 // the launches of an execute, their order and grids; the plan kernel's table (ltrp::build_schedule)
  double* last_out = nullptr;
  hipStream_t last_stream = nullptr;
  std::vector<hipStream_t> streams;     // every stream an execute of this plan was queued on (synchronised before its buffers are released)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_up = nullptr;            // device-side input preparation (hap codes) done
  int fan_lanes = 1;                     // certificate launches dealt over this many streams (own scratch region each)
  size_t scratch_lane_stride = 0;        // doubles per stream region of d_scratch
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fast = nullptr, ev_x[kNumExact + 1] = {nullptr};   // exact launches side by side: after the certificate launches / joined back (+ 1: the W = 20 launch)
  hipEvent_t ev_close[kNumExact][4] = {{nullptr}};   // "every certificate launch that can feed exact list c has been queued", one per launch stream
  PackTable* d_pk_tabs = nullptr;       // sched.pack_tabs
  PlanEntry* d_pl_entries = nullptr;    // sched.plan_entries
  unsigned long long* d_wave_clock = nullptr;   // (debug) two wall-clock words per wavefront of the plan kernel
  FamilyDesc* d_fams = nullptr;         // fams (BatchPlan): the family launch's list
  FamilySpine* d_fam_spines = nullptr;  // fam_spines (BatchPlan): per family, beside d_fams
  double* d_fam_park = nullptr;         // ... per wavefront of its grid: kFamilyParkDoubles (the park rows: the stem's last row, the spine's fork rows)
  uint32_t* d_fam_stats = nullptr;      // ... 4 words, zeroed by every execute (FamilyArgs::stats)
  unsigned long long* d_fam_wave_clock = nullptr;   // (debug) ... two wall-clock words per wavefront of its grid (FamilyArgs::wave_clock)
  int fam_clock_waves = 0;              // ... wavefronts of the family launch of the last execute
  hipEvent_t bin_ev[ltrp::kNumKernels + 1] = {nullptr};   // bracket every DP launch on the launch stream
  uint32_t* d_ctrl_init = nullptr;      // image of the control words (queues = 0, redo count = n_generic)
  int32_t* d_redo_init = nullptr;       // indices of the generic pairs: copied over the head of the redo list every execute
  bool last_wg_thr = false;             // ... and the last execute scored them with the threshold kernels first
  // compact plans (ltr_plan_create): every device array below is a piece of ONE block; the scores live in pinned host memory
  void* d_block = nullptr;
  double* h_ll = nullptr; size_t h_ll_cap = 0;
  bool ctrl_fresh = false;              // the control words arrived with the upload: the first execute skips their reset
  int timed = 0;                        // the last execute recorded per-launch events (level)
  int timing = 0;                       // record a HIP event around every launch (ltr_plan_set_timing): 1 = as launched, 2 = the multi-width launches class by class
  int32_t* d_redo_list = nullptr;       // kNumExact lists (capacity n_pairs each): pairs the certificate kernels handed to the exact kernels
  uint32_t* d_redo_count = nullptr;     // their lengths (control words)
  int64_t redo_cap = 1;
  uint32_t seed_total = 0;
  int last_launches = 0;
  int grid_cap = 0;                     // ltr_ctx_set_debug "grid_cap" as it stood when the plan was built (0: none): the grids formed at execute time follow it
  std::vector<ltrp::LaunchNote> launch_log;   // the kernel launches of the last execute as made (ltr_debug_last_launches)
  bool executed = false;
  bool kernel_ms_counted = true;
};

// ---- what the units need from each other ----
#pragma GCC visibility push(hidden)
// ltr_ctx.hip
int build_tables(ltr_ctx* ctx, int64_t len, bool same_size = false);
// recycled pinned blocks of a context (see ltr_ctx: compact plans; its recycled events: ltr_lease.h)
double* ctx_take_pinned(ltr_ctx* ctx, size_t bytes, size_t* cap_out, double** dev_out);
void ctx_give_pinned(ltr_ctx* ctx, void* p);
// ltr_plan_build.hip
void release_plan_buffers(ltr_plan* plan, ltr_ctx* ctx);
// ltr_plan_run.hip
void wg_stats_poll(ltr_ctx* ctx);
#pragma GCC visibility pop

#endif
