// ltr_plan_build.hip -- ltr_plan_create / ltr_plan_destroy: what ltrp::describe_batch (ltr_plan_describe.cpp) decided about a batch
// becomes a plan on the device -- the grid query, the launch schedule (ltrp::build_schedule), the upload (one block for a compact
// plan, separate buffers otherwise), scratch strips and events.  Running a plan: ltr_plan_run.hip.

#include <cmath>
#include <cstring>

#include "ltr_ctx.h"

using namespace ltrp;                            // class table, Rules, classify_pair, sort_by_class (ltr_plan.h)

namespace {

// The LUT kernels stream each haplotype base as the byte offset of its block of the emission table
// ('A','C','T','G' -> ((byte >> 1) & 3) * 4096; the zero padding maps to 0): formed here from the uploaded bytes,
// one pass at HBM speed instead of a host loop plus a second upload twice the size.
__global__ __launch_bounds__(256) void ltr_hap_codes_kernel(const uint8_t* __restrict__ haps, uint16_t* __restrict__ codes, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t k = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; k < n; k += stride) {
    if (k + 4 <= n) {
      const uint32_t w = *(const uint32_t*)(haps + k);           // (hipMalloc'ed / pool blocks: 256-byte aligned)
      ushort4 c;
      c.x = (uint16_t)(((w >> 1) & 3u) << 12); c.y = (uint16_t)(((w >> 9) & 3u) << 12);
      c.z = (uint16_t)(((w >> 17) & 3u) << 12); c.w = (uint16_t)(((w >> 25) & 3u) << 12);
      *(ushort4*)(codes + k) = c;
    } else {
      for (size_t i = k; i < n; ++i) codes[i] = (uint16_t)((((uint32_t)haps[i] >> 1) & 3u) << 12);
    }
  }
}

}  // namespace

// Give a plan's device buffers back (to the context's pool, or to the runtime when the context is gone).
void release_plan_buffers(ltr_plan* plan, ltr_ctx* ctx) {
  for (hipStream_t st : plan->streams) (void)hipStreamSynchronize(st);       // nothing in flight may still use the buffers
  if (plan->ev_up) (void)hipEventSynchronize(plan->ev_up);                   // (... nor the input preparation of a plan that never ran)
  plan->streams.clear();
  void** bufs[] = {(void**)&plan->d_reads, (void**)&plan->d_haps, (void**)&plan->d_hap_codes, (void**)&plan->d_pairs,
                   (void**)&plan->d_ll, (void**)&plan->d_queue, (void**)&plan->d_scratch, (void**)&plan->d_redo_list,
                   (void**)&plan->d_ctrl_init, (void**)&plan->d_redo_init, (void**)&plan->d_pk_tabs, (void**)&plan->d_pl_entries, (void**)&plan->d_wave_clock,
                   (void**)&plan->d_fams, (void**)&plan->d_fam_park, (void**)&plan->d_fam_stats, (void**)&plan->d_fam_spines, (void**)&plan->d_fam_wave_clock};
  if (plan->d_block || plan->h_ll) {
    // a compact plan: one block holds every array but the scratch strips and the family launch's; the scores are a pinned block of the context
    void* const scr = plan->d_scratch; void* const fm = plan->d_fams; void* const fp = plan->d_fam_park; void* const fs = plan->d_fam_stats; void* const fsp = plan->d_fam_spines; void* const fwc = plan->d_fam_wave_clock;
    for (void** p : bufs) *p = nullptr;
    plan->d_scratch = (double*)scr; plan->d_fams = (FamilyDesc*)fm; plan->d_fam_park = (double*)fp; plan->d_fam_stats = (uint32_t*)fs; plan->d_fam_spines = (FamilySpine*)fsp; plan->d_fam_wave_clock = (unsigned long long*)fwc;
    if (ctx) ctx->pool.release(plan->d_block); else if (plan->d_block) (void)hipFree(plan->d_block);
    plan->d_block = nullptr;
    ctx_give_pinned(ctx, plan->h_ll);
    plan->h_ll = nullptr;
  }
  for (void** p : bufs) { if (ctx) ctx->pool.release(*p); else if (*p) (void)hipFree(*p); *p = nullptr; }
  plan->d_redo_count = nullptr;
}

static void destroy_plan(ltr_plan* plan, const bool ctx_locked) {
  ltr_ctx* ctx = plan->ctx;                                    // nullptr: the context was destroyed first
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    if (ctx_locked) ctx->plans.erase(plan);
    else { std::lock_guard<std::mutex> lk(ctx->mu); ctx->plans.erase(plan); }
  }
  release_plan_buffers(plan, ctx);
  ctx_give_event(ctx, plan->ev_up, false);
  if (plan->ev_fast) (void)hipEventDestroy(plan->ev_fast);
  if (plan->ev_fork) (void)hipEventDestroy(plan->ev_fork);
  for (int k = 0; k < 3; ++k) if (plan->ev_join[k]) (void)hipEventDestroy(plan->ev_join[k]);
  for (int c = 0; c <= kNumExact; ++c) if (plan->ev_x[c]) (void)hipEventDestroy(plan->ev_x[c]);
  for (int c = 0; c < kNumExact; ++c) for (int k = 0; k < 4; ++k) if (plan->ev_close[c][k]) (void)hipEventDestroy(plan->ev_close[c][k]);
  ctx_give_event(ctx, plan->ev0, true);
  ctx_give_event(ctx, plan->ev1, true);
  for (int k = 0; k <= kNumKernels; ++k) if (plan->bin_ev[k]) (void)hipEventDestroy(plan->bin_ev[k]);
  delete plan;
}

// ---- units of ltr_plan_create (the class rule, the sort, the class statistics and the launch schedule live in the ltr_plan_*.cpp units, ltr_plan.h) ----

#define GRID_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
// Resident workgroups of every launch class (occupancy x CUs), asked from the runtime once per context.
static hipError_t ctx_query_grids(ltr_ctx* ctx) {
  for (int k = 0; k < kNumFast; ++k) {
    const ClassInfo ci = class_info(k);
    int per_cu = 0;
    GRID_TRY(ci.family == kFamOne ? ltrk::occ_onewave(ci.W, &per_cu) : (ci.family == kFamPack ? ltrk::occ_pack(ci.W, &per_cu)
             : (ci.family == kFamShare ? ltrk::occ_family(&per_cu) : ltrk::occ_wg(ci.waves, ci.W, &per_cu))));
    ctx->full_grid[k] = std::max(per_cu, 1) * ctx->n_cu;
  }
  {
    int per_cu = 0;
    GRID_TRY(ltrk::occ_multi(&per_cu));
    ctx->full_multi_grid = std::max(per_cu, 1) * ctx->n_cu;
    per_cu = 0;
    GRID_TRY(ltrk::occ_pack_multi(&per_cu));
    ctx->full_pmulti_grid = std::max(per_cu, 1) * ctx->n_cu;
    per_cu = 0;
    GRID_TRY(ltrk::occ_plan(true, &per_cu));
    int per_cu_general = 0;
    GRID_TRY(ltrk::occ_plan(false, &per_cu_general));           // (same launch bounds and LDS: the smaller of the two sizes the grid for both)
    ctx->full_plan_grid = std::max(std::min(per_cu, per_cu_general), 1) * ctx->n_cu;
  }
  for (int c = 0; c <= kNumExact; ++c) {                     // (kNumExact: the W = 20 launch that shares the four-wave list)
    int per_cu = 0;
    GRID_TRY(ltrk::occ_exact(c, &per_cu));
    if (c < kNumExact) ctx->full_x_grid[c] = std::max(per_cu, 1) * ctx->n_cu;
    else ctx->full_x_wide_grid = std::max(per_cu, 1) * ctx->n_cu;
  }
  for (int nw = 0; nw < 2; ++nw)
    for (int w = (nw ? kWg8MinW : 6); w <= kWgWMax; w += 2) {
      int per_cu = 0;
      GRID_TRY(ltrk::occ_wgt(nw ? 8 : 4, w, &per_cu));
      ctx->full_wgt_grid[nw][w] = std::max(per_cu, 1) * ctx->n_cu;
    }
  ctx->full_redo_grid = ctx->full_x_grid[kXGeneric];
  ctx->have_grids = true;
  return hipSuccess;
}
#undef GRID_TRY

#define PLAN_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ltr::set_error(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); return LTR_ERR_HIP; } } while (0)

// One ltr_plan_create, under ctx->mu: the half-built plan, what the device is given besides the batch itself, and the steps that
// get it there.  THE owner of the plan until release(): whichever way ltr_plan_create is left before that -- an error status or an
// exception (bad_alloc in a host array) -- the destructor waits for the copies out of the caller's arrays (ev_copied, the upload
// stream) and takes the plan down; nothing of it is in flight when its buffers go back to the pool.
namespace {

struct PlanBuild {
  ltr_ctx* const ctx;
  const ltr_locus_batch* const b;
  ltr_plan* plan = nullptr;
  hipEvent_t ev_copied = nullptr;          // the copies out of the caller's arrays / the context's staging (separate upload)
  // host images of the small device arrays
  std::vector<uint32_t> ctrl;              // control words (queues = 0, list lengths = the seeds)
  std::vector<int32_t> init;               // the pre-seeded list heads
  bool want_clock = false;
  // sizes and the layout of a compact plan's block
  int64_t rbytes = 0, hbytes = 0;
  size_t hap_buf = 0, read_buf = 0, ll_bytes = 0;
  size_t o_queue = 0, o_ctrl = 0, o_ent = 0, o_tabs = 0, o_init = 0, o_pairs = 0, o_reads = 0, o_haps = 0, o_codes = 0, image_bytes = 0, o_list = 0, block_bytes = 0;

  PlanBuild(ltr_ctx* c, const ltr_locus_batch* batch) : ctx(c), b(batch) {}
  PlanBuild(const PlanBuild&) = delete;
  PlanBuild& operator=(const PlanBuild&) = delete;
  ~PlanBuild() {
    (void)copies_done();
    if (plan) { (void)hipStreamSynchronize(ctx->up_stream); destroy_plan(plan, true); }       // (ctx->mu is held here)
  }
  hipError_t copies_done() { if (!ev_copied) return hipSuccess; const hipError_t e_ = hipEventSynchronize(ev_copied); (void)hipEventDestroy(ev_copied); ev_copied = nullptr; return e_; }
  ltr_plan* release() { ltr_plan* p = plan; plan = nullptr; return p; }

  int describe();
  int layout();
  int upload_compact();
  int upload_separate();
  int size_scratch_and_fan();
};

// The host side: ltrp::describe_batch in the context's work arrays, then class statistics and the model tables.
int PlanBuild::describe() {
  plan = new ltr_plan();
  plan->ctx = ctx;
  plan->n_reads = b->n_reads;
  ltr_ctx::PlanScratch& s = ctx->scratch;
  std::string why;
  const ltrp::BatchScratch w{s.pairs, s.sorted, s.key, s.bin, s.order, s.read_acgt, s.hap_acgt};
  const int rc0 = ltrp::describe_batch(b, ctx->mc, ctx->params.indel_flank_len, ctx->pair_packing, ctx->n_cu, ctx->dbg, w, plan, &why);
  if (rc0 != LTR_OK) { ltr::set_error(ctx, why); return rc0; }
  ltrp::class_stats(*plan, w, &plan->stats);
  LTR_DBG("plan: %zu pairs, max_len %d", s.sorted.size(), plan->max_len);
  const int rc = build_tables(ctx, (int64_t)plan->max_len + 2);
  if (rc != LTR_OK) return rc;
  LTR_DBG("tables built");
  return LTR_OK;
}

// Sizes of the device arrays, the launch schedule, the host images of the small arrays, and where everything sits in a compact plan's block.
int PlanBuild::layout() {
  RawBuf<PairDesc>& sorted = ctx->scratch.sorted;
  const int32_t max_len = plan->max_len;
  rbytes = b->n_reads > 0 ? b->read_off[b->n_reads] : 0;
  hbytes = b->n_haps > 0 ? b->hap_off[b->n_haps] : 0;
  // 96 bytes of zero padding either side: the kernel streams haplotype rows without clamping
  // ... and the two-pairs-per-wave kernels keep streaming rows of the SHORTER haplotype of a wave
  // until the longer one ends: the tail pad also covers the longest window of the batch
  const size_t hap_tail = (size_t)kHapPad + (size_t)max_len + 384;   // (+ the workgroup kernels' 64-row chunks, two ahead)
  hap_buf = (size_t)std::max<int64_t>(hbytes, 1) + kHapPad + hap_tail;
  read_buf = (size_t)std::max<int64_t>(rbytes, 1) + kReadPad;       // (the packed kernels load a lane's strip of bytes unclamped)
  // the launches with their persistent grids (occupancy x CUs, asked from the runtime once per context), the plan kernel's table and
  // the tables of the packed widths, the images of the control words and of the pre-seeded list heads: everything the device is
  // given besides the batch itself
  if (!ctx->have_grids) PLAN_TRY(ctx_query_grids(ctx));
  {
    ltrp::OccupancyGrids occ;
    std::copy(ctx->full_grid, ctx->full_grid + kNumFast, occ.cls);
    std::copy(ctx->full_x_grid, ctx->full_x_grid + kNumExact, occ.exact);
    occ.multi = ctx->full_multi_grid; occ.pack_multi = ctx->full_pmulti_grid; occ.plan = ctx->full_plan_grid;
    ltrp::build_schedule(plan, plan->stats, occ, ctx->dbg, &plan->sched);
  }
  const std::vector<PlanEntry>& entries = plan->sched.plan_entries;
  const std::vector<PackTable>& tabs = plan->sched.pack_tabs;
  ctrl.assign(kCtrlWords, 0);
  for (int c = 0; c < kNumExact; ++c) ctrl[kRedoCountSlot + c] = (uint32_t)plan->x_seed[c];
  // image of the pre-seeded list heads: the sorted-array indices bin_first[kNumFast] .. n_pairs, in order
  const int n_seed = plan->bin_first[kNumKernels] - plan->bin_first[kNumFast];
  init.assign((size_t)std::max(n_seed, 1), 0);
  for (int g2 = 0; g2 < n_seed; ++g2) init[(size_t)g2] = plan->bin_first[kNumFast] + g2;
  plan->redo_cap = (int64_t)std::max<size_t>(sorted.size(), 1);
  want_clock = !entries.empty() && ctx->dbg.wave_clock > 0;
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  o_queue = 0; o_ctrl = up256(o_queue + kCtrlWords * sizeof(uint32_t)); o_ent = up256(o_ctrl + kCtrlWords * sizeof(uint32_t));
  o_tabs = up256(o_ent + std::max<size_t>(entries.size(), 1) * sizeof(PlanEntry));
  o_init = up256(o_tabs + std::max<size_t>(tabs.size(), 1) * sizeof(PackTable)); o_pairs = up256(o_init + init.size() * sizeof(int32_t));
  o_reads = up256(o_pairs + std::max<size_t>(sorted.size(), 1) * sizeof(PairDesc)); o_haps = up256(o_reads + read_buf);
  o_codes = up256(o_haps + hap_buf); image_bytes = up256(o_codes + hap_buf * sizeof(uint16_t));
  o_list = image_bytes; block_bytes = up256(o_list + (size_t)plan->redo_cap * kNumExact * sizeof(int32_t));
  ll_bytes = (size_t)std::max<int64_t>(plan->ll_size, 1) * sizeof(double);
  return LTR_OK;
}

// COMPACT plans (round 6): a one-locus call -- HapAligner::process_reads as the reference calls it, once per locus
// (seq_stutter_genotyper.cpp:517-523) -- is a few hundred pairs and a few hundred KB; what it costs is not the DP (0.1 ms) but
// the dozen allocations, the eight copies (four of them synchronous), the three fills, the hap-code launch, the events and
// the two downloads around it.  Such a plan is ONE device block laid out below, filled from ONE pinned image the host writes
// (the haplotype codes too: a host loop over a few KB) by ONE copy over the DMA engines; the control words arrive with it (the
// first execute skips its reset); the scores are written by the kernel straight into pinned host memory the device can
// reach, so ltr_plan_fetch is an event wait and a memcpy.  Same kernels, same launch, same bits.
int PlanBuild::upload_compact() {
  RawBuf<PairDesc>& sorted = ctx->scratch.sorted;
  const std::vector<PlanEntry>& entries = plan->sched.plan_entries;
  const std::vector<PackTable>& tabs = plan->sched.pack_tabs;
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_block, block_bytes));
  uint8_t* const base = (uint8_t*)plan->d_block;
  plan->d_queue = (uint32_t*)(base + o_queue); plan->d_ctrl_init = (uint32_t*)(base + o_ctrl); plan->d_pl_entries = (PlanEntry*)(base + o_ent);
  plan->d_pk_tabs = (PackTable*)(base + o_tabs); plan->d_redo_init = (int32_t*)(base + o_init); plan->d_pairs = (PairDesc*)(base + o_pairs);
  plan->d_reads = base + o_reads; plan->d_haps = base + o_haps; plan->d_hap_codes = (uint16_t*)(base + o_codes);
  plan->d_redo_list = (int32_t*)(base + o_list);
  plan->d_redo_count = plan->d_queue + kRedoCountSlot;
  if (entries.empty()) plan->d_pl_entries = nullptr;
  if (tabs.empty()) plan->d_pk_tabs = nullptr;
  // the image: the context's pinned staging block, free again once the previous compact plan's copy is through
  if (ctx->compact_ev_pending) { PLAN_TRY(hipEventSynchronize(ctx->compact_ev)); ctx->compact_ev_pending = false; }
  ctx->compact_stage.resize(image_bytes);
  uint8_t* const img = ctx->compact_stage.data();
  std::memset(img, 0, o_pairs);                                                      // control words, table padding
  std::memcpy(img + o_ctrl, ctrl.data(), ctrl.size() * sizeof(uint32_t));
  std::memcpy(img + o_queue, ctrl.data(), ctrl.size() * sizeof(uint32_t));       // (the control words themselves: the first execute needs no reset)
  if (!entries.empty()) std::memcpy(img + o_ent, entries.data(), entries.size() * sizeof(PlanEntry));
  if (!tabs.empty()) std::memcpy(img + o_tabs, tabs.data(), tabs.size() * sizeof(PackTable));
  std::memcpy(img + o_init, init.data(), init.size() * sizeof(int32_t));
  if (!sorted.empty()) std::memcpy(img + o_pairs, sorted.data(), sorted.size() * sizeof(PairDesc));
  std::memset(img + o_reads, 0, o_haps - o_reads);
  if (rbytes) std::memcpy(img + o_reads, b->read_bytes, (size_t)rbytes);
  std::memset(img + o_haps, 0, o_codes - o_haps);
  if (hbytes) std::memcpy(img + o_haps + kHapPad, b->hap_bytes, (size_t)hbytes);
  {
    // the haplotypes as emission-table block offsets (what ltr_hap_codes_kernel forms on the device for the large plans)
    const uint8_t* hsrc = img + o_haps;
    uint16_t* hc = (uint16_t*)(img + o_codes);
    for (size_t i = 0; i < hap_buf; ++i) hc[i] = (uint16_t)((((uint32_t)hsrc[i] >> 1) & 3u) << 12);
    std::memset(img + o_codes + hap_buf * sizeof(uint16_t), 0, image_bytes - (o_codes + hap_buf * sizeof(uint16_t)));
  }
  PLAN_TRY(hipMemcpyAsync(plan->d_block, img, image_bytes, hipMemcpyHostToDevice, ctx->up_stream));
  if (!ctx->compact_ev) PLAN_TRY(hipEventCreateWithFlags(&ctx->compact_ev, hipEventDisableTiming));
  PLAN_TRY(hipEventRecord(ctx->compact_ev, ctx->up_stream));
  ctx->compact_ev_pending = true;
  plan->ev_up = ctx_take_event(ctx, false);
  if (!plan->ev_up) { ltr::set_error(ctx, "hipEventCreate failed"); return LTR_ERR_HIP; }
  PLAN_TRY(hipEventRecord(plan->ev_up, ctx->up_stream));
  // the scores: pinned host memory the kernel writes into (zero = what a masked cell keeps)
  plan->h_ll = ctx_take_pinned(ctx, ll_bytes, &plan->h_ll_cap, &plan->d_ll);
  if (!plan->h_ll) { plan->d_ll = nullptr; ltr::set_error(ctx, "out of pinned host memory"); return LTR_ERR_NOMEM; }
  std::memset(plan->h_ll, 0, ll_bytes);
  plan->ctrl_fresh = true;
  return LTR_OK;
}

int PlanBuild::upload_separate() {
  RawBuf<PairDesc>& sorted = ctx->scratch.sorted;
  const std::vector<PlanEntry>& entries = plan->sched.plan_entries;
  const std::vector<PackTable>& tabs = plan->sched.pack_tabs;
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_reads, read_buf));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_haps, hap_buf));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_hap_codes, hap_buf * sizeof(uint16_t)));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_pairs, std::max<size_t>(sorted.size(), 1) * sizeof(PairDesc)));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_ll, ll_bytes));
  // Everything on the context's upload stream, the COPIES FIRST: they go over the DMA engines, while a fill (hipMemset) or the
  // hap-code kernel needs wave slots -- and behind the persistent launch of the previous chunk of ltr_calc_hap_aln_probs there are
  // none until that launch drains.  The host waits for the copies only (ev_copied, at the end of this call: the caller's arrays and
  // the context's staging are free again on return); the plan's executes wait for all of it (ev_up).  (Measured on MI355X, 30 000
  // catalogue loci in three chunks: with hipMemset + hipMemcpy on the null stream the uploads of chunks 1 and 2 took 2.0 - 2.1 ms
  // against 0.24 for chunk 0 -- the copy sat behind the fill, the fill behind the running plan kernel; profiles/r05/e2e_prep_ahead.log.)
  if (rbytes) PLAN_TRY(hipMemcpyAsync(plan->d_reads, b->read_bytes, (size_t)rbytes, hipMemcpyHostToDevice, ctx->up_stream));
  if (hbytes) PLAN_TRY(hipMemcpyAsync(plan->d_haps + kHapPad, b->hap_bytes, (size_t)hbytes, hipMemcpyHostToDevice, ctx->up_stream));
  if (!sorted.empty()) PLAN_TRY(hipMemcpyAsync(plan->d_pairs, sorted.data(), sorted.size() * sizeof(PairDesc), hipMemcpyHostToDevice, ctx->up_stream));
  PLAN_TRY(hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming));
  {
    const hipError_t e_ = hipEventRecord(ev_copied, ctx->up_stream);
    if (e_ != hipSuccess) { (void)hipEventDestroy(ev_copied); ev_copied = nullptr; ltr::set_error(ctx, std::string("hipEventRecord: ") + hipGetErrorString(e_)); return LTR_ERR_HIP; }
  }
  LTR_DBG("upload: copies queued");
  {
    // the zero padding either side of the haplotype bytes, then the hap codes (see ltr_hap_codes_kernel), then the output rows
    PLAN_TRY(hipMemsetAsync(plan->d_haps, 0, kHapPad, ctx->up_stream));
    PLAN_TRY(hipMemsetAsync(plan->d_haps + kHapPad + hbytes, 0, hap_buf - kHapPad - (size_t)hbytes, ctx->up_stream));
    const int blocks = (int)std::min<size_t>((hap_buf / 4 + 255) / 256 + 1, (size_t)ctx->n_cu * 8);
    hipLaunchKernelGGL(ltr_hap_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->up_stream, plan->d_haps, plan->d_hap_codes, hap_buf);
    PLAN_TRY(hipGetLastError());
    PLAN_TRY(hipMemsetAsync(plan->d_ll, 0, ll_bytes, ctx->up_stream));
    plan->ev_up = ctx_take_event(ctx, false);
    if (!plan->ev_up) { ltr::set_error(ctx, "hipEventCreate failed"); return LTR_ERR_HIP; }
    PLAN_TRY(hipEventRecord(plan->ev_up, ctx->up_stream));
  }
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_queue, kCtrlWords * sizeof(uint32_t)));      // work queues + exact list lengths (ltr_plan.h)
  plan->d_redo_count = plan->d_queue + kRedoCountSlot;
  LTR_DBG("uploaded");
  if (!tabs.empty()) {
    PLAN_TRY(ctx->pool.alloc((void**)&plan->d_pk_tabs, tabs.size() * sizeof(PackTable)));
    PLAN_TRY(hipMemcpy(plan->d_pk_tabs, tabs.data(), tabs.size() * sizeof(PackTable), hipMemcpyHostToDevice));
  }
  if (want_clock) {
    const size_t nb = ((size_t)ctx->full_plan_grid * kBlockWaves * 4 + 4096 + 256) * sizeof(unsigned long long);
    PLAN_TRY(ctx->pool.alloc((void**)&plan->d_wave_clock, nb));
    PLAN_TRY(hipMemset(plan->d_wave_clock, 0, nb));
  }
  if (!entries.empty()) {
    PLAN_TRY(ctx->pool.alloc((void**)&plan->d_pl_entries, entries.size() * sizeof(PlanEntry)));
    PLAN_TRY(hipMemcpy(plan->d_pl_entries, entries.data(), entries.size() * sizeof(PlanEntry), hipMemcpyHostToDevice));
  }
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_redo_list, (size_t)plan->redo_cap * kNumExact * sizeof(int32_t)));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_ctrl_init, ctrl.size() * sizeof(uint32_t)));
  PLAN_TRY(hipMemcpy(plan->d_ctrl_init, ctrl.data(), ctrl.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  PLAN_TRY(ctx->pool.alloc((void**)&plan->d_redo_init, init.size() * sizeof(int32_t)));
  PLAN_TRY(hipMemcpy(plan->d_redo_init, init.data(), init.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return LTR_OK;
}

// Boundary strips of the resident waves, the streams the launches are dealt over, the plan's events.
int PlanBuild::size_scratch_and_fan() {
  const int32_t max_len = plan->max_len;
  plan->scratch_stride = ((max_len + 2 + 15) / 16) * 16;
  {
    // boundary strips: 6 arrays x stride doubles per resident wave; for very long reads shrink
    // the persistent grids instead of allocating more than ~8 GB
    const size_t per_wave = (size_t)6 * plan->scratch_stride * sizeof(double);
    // The certificate launches of a plan are dealt over TWO streams (regions of their own in the scratch strips): every
    // launch ends in a last, partly filled round of pairs per wave slot, and the next class fills it.  Measured on
    // MI355X, config 3, same box: 10 000 loci 245.5 ms per pass on one stream, 241.6 on two, 243.0 on three, 244.7 on
    // four; 1250 loci (one GPU's share of the catalogue sharded over eight) 38.6 / 32.2 / 32.4 / 33.8 ms -- 2.16e12 ->
    // 2.58e12 cells/s.  (ltr_ctx_set_debug "fan_lanes" / "fan_pairs": the A/B switches of those runs.)
    const int64_t fan_below = ctx->dbg.fan_pairs > 0 ? ctx->dbg.fan_pairs : INT64_MAX;
    const int fan_n = ctx->dbg.fan_lanes > 0 ? std::min(4, ctx->dbg.fan_lanes) : 4;       // two lanes for the big classes + two for the small ones
    // (... or, with fewer pairs, when pairs go to workgroup kernels: a launch of a few hundred 5-kb pairs is a handful of
    // rounds of one pair per workgroup, each milliseconds long -- config5hifi: the 180 pairs of the W = 11 class, 4.2 ms,
    // used to start behind the 23 ms of the W = 10 class)
    plan->fan_lanes = (ctx->pair_packing < 0 && (plan->n_pairs >= (int64_t)16 * ctx->n_cu || plan->uses_wg) && plan->n_pairs < fan_below) ? fan_n : 1;
    const int cap = (int)std::max<size_t>(16, ((size_t)8 << 30) / (per_wave * kBlockWaves * ((size_t)plan->fan_lanes + 1)));
    plan->sched.cap_grids(cap);
    plan->grid_cap = std::max(ctx->dbg.grid_cap, 0);
    if (plan->grid_cap > 0) plan->sched.cap_every_grid(plan->grid_cap);      // (tests; before anything below is sized by a grid)
    plan->scratch_lane_stride = (size_t)plan->sched.max_grid * kBlockWaves * 6 * (size_t)plan->scratch_stride;
    PLAN_TRY(ctx->pool.alloc((void**)&plan->d_scratch, plan->scratch_lane_stride * sizeof(double) * ((size_t)plan->fan_lanes + 1)));   // (+ 1: the kXLong exact launch, see ltr_plan_execute)
    // the family launch: its list, a parking block per wavefront of ITS grid (as capped above), its counters
    if (!plan->fams.empty()) {
      int fam_grid = 1;
      for (const Launch& L : plan->sched.launches) if (L.kind == kLaunchFamily) fam_grid = std::max(fam_grid, L.grid);
      for (const Launch& L : plan->sched.by_class) if (L.kind == kLaunchFamily) fam_grid = std::max(fam_grid, L.grid);
      PLAN_TRY(ctx->pool.alloc((void**)&plan->d_fams, plan->fams.size() * sizeof(FamilyDesc)));
      PLAN_TRY(hipMemcpy(plan->d_fams, plan->fams.data(), plan->fams.size() * sizeof(FamilyDesc), hipMemcpyHostToDevice));
      PLAN_TRY(ctx->pool.alloc((void**)&plan->d_fam_spines, plan->fam_spines.size() * sizeof(FamilySpine)));
      PLAN_TRY(hipMemcpy(plan->d_fam_spines, plan->fam_spines.data(), plan->fam_spines.size() * sizeof(FamilySpine), hipMemcpyHostToDevice));
      // (kFamilyParkSlots park rows per wavefront, each sized for the widest strip: 8 x 42 x 64 doubles = 168 KB (172 032 bytes), 528 MB
      // for the 3072 wavefronts of a full grid on 256 CUs; a family with a spine uses 8 x (2W+2) x 64 doubles of it, dense from the block's start)
      PLAN_TRY(ctx->pool.alloc((void**)&plan->d_fam_park, (size_t)fam_grid * kBlockWaves * kFamilyParkDoubles * sizeof(double)));
      PLAN_TRY(ctx->pool.alloc((void**)&plan->d_fam_stats, 4 * sizeof(uint32_t)));
      PLAN_TRY(hipMemset(plan->d_fam_stats, 0, 4 * sizeof(uint32_t)));
      if (ctx->dbg.wave_clock > 0) {                           // (measurement aid: ltr_debug_family_wave_clocks)
        const size_t nb = (size_t)fam_grid * kBlockWaves * 2 * sizeof(unsigned long long);
        PLAN_TRY(ctx->pool.alloc((void**)&plan->d_fam_wave_clock, nb));
        PLAN_TRY(hipMemset(plan->d_fam_wave_clock, 0, nb));
      }
    }
    if (plan->fan_lanes > 1) {
      PLAN_TRY(hipEventCreateWithFlags(&plan->ev_fork, hipEventDisableTiming));
      for (int k = 0; k < 3; ++k) PLAN_TRY(hipEventCreateWithFlags(&plan->ev_join[k], hipEventDisableTiming));
    }
  }
  plan->ev0 = ctx_take_event(ctx, true);
  plan->ev1 = ctx_take_event(ctx, true);
  if (!plan->ev0 || !plan->ev1) { ltr::set_error(ctx, "hipEventCreate failed"); return LTR_ERR_HIP; }
  // (the per-launch events are created by ltr_plan_set_timing, only for plans that ask for them)
  return LTR_OK;
}

}  // namespace

extern "C" {

int ltr_plan_create(ltr_ctx* ctx, const ltr_locus_batch* b, ltr_plan** out) {
  if (!ctx || !b || !out) return LTR_ERR_INVALID;
  *out = nullptr;
  LTR_DBG("plan: create");
  std::lock_guard<std::mutex> lk(ctx->mu);
  // (no exception crosses the C-ABI: a host array that cannot grow ends the call with LTR_ERR_NOMEM and the half-built plan is taken
  // down by its owner, PlanBuild)
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PlanBuild pb(ctx, b);
  int rc;
  if ((rc = pb.describe()) != LTR_OK || (rc = pb.layout()) != LTR_OK) return rc;
  const bool compact = ctx->dbg.compact_plan >= 0 && !pb.want_clock && pb.image_bytes <= kCompactImageMax && pb.ll_bytes <= kCompactLlMax;
  if ((rc = compact ? pb.upload_compact() : pb.upload_separate()) != LTR_OK || (rc = pb.size_scratch_and_fan()) != LTR_OK) return rc;
  {                                                            // the caller's arrays / the context's staging are free again
    const hipError_t e_ = pb.copies_done();
    if (e_ != hipSuccess) { ltr::set_error(ctx, std::string("copies_done(): ") + hipGetErrorString(e_)); return LTR_ERR_HIP; }
  }
  LTR_DBG("upload: copies done");
  ctx->plans.insert(pb.plan);                                  // (ctx->mu is held)
  *out = pb.release();                                         // (handed out)
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

void ltr_plan_destroy(ltr_plan* plan) {
  if (plan) destroy_plan(plan, false);
}

int64_t ltr_plan_num_pairs(const ltr_plan* p) { return p ? p->n_pairs : 0; }
int64_t ltr_plan_ll_size(const ltr_plan* p) { return p ? p->ll_size : 0; }
double ltr_plan_cells(const ltr_plan* p) { return p ? p->cells : 0.0; }
double ltr_plan_input_bytes(const ltr_plan* p) { return p ? p->input_bytes : 0.0; }

}  // extern "C"
