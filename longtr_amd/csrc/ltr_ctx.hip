// ltr_ctx.hip -- the context of the C-ABI (include/ltr_gpu.h): create / destroy, alignment and stutter parameters, the model
// tables the kernels read, debug knobs, timers, the event and pinned-block caches, and the ltr::ctx_* accessors the other
// translation units reach a context through (ltr_internal.h).  Plans: ltr_plan_build.hip, ltr_plan_run.hip.
//
// No CPU fallback exists in this file: every compute entry point fails with
// LTR_ERR_NO_DEVICE when there is no HIP device.

#include <cmath>
#include <cstdio>
#include <cstring>

#include "ltr_ctx.h"

using namespace ltrp;                            // class table, Rules, classify_pair, sort_by_class (ltr_plan.h)

#define LTR_VERSION_STR "longtr_amd 0.6 (gfx950; ABI 6)"

namespace ltrp {
void* pinned_alloc(size_t bytes) {
  void* v = nullptr;
  if (hipHostMalloc(&v, bytes, hipHostMallocPortable) == hipSuccess) return v;
  (void)hipGetLastError();
  return nullptr;
}
void pinned_free(void* p) { (void)hipHostFree(p); }
}

namespace ltr {
std::atomic<int> g_trace{0};
double dbg_ms() {
  static const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
void set_error(ltr_ctx* ctx, const std::string& msg) { if (ctx) { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->err = msg; } }
void add_time(ltr_ctx* ctx, int which, double seconds, double kernel_ms) {
  if (!ctx) return;
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  if (which == kTimerHapBuild) { ctx->tm.hap_build_s += seconds; if (seconds > 0) ctx->tm.hap_build_calls++; }
  else if (which == kTimerHapAln) { ctx->tm.hap_aln_s += seconds; if (seconds > 0) ctx->tm.hap_aln_calls++; }
  else if (which == kTimerPosterior) { ctx->tm.posterior_s += seconds; if (seconds > 0) ctx->tm.posterior_calls++; }
  if (which == kTimerNwKernel) ctx->tm.nw_kernel_ms += kernel_ms;
  else if (which == kTimerShortKernel) ctx->tm.short_kernel_ms += kernel_ms;
  else ctx->tm.dp_kernel_ms += kernel_ms;
}
void ctx_note_short_split(ltr_ctx* ctx, const double ms4[4]) { std::lock_guard<std::mutex> lk(ctx->err_mu); for (int k = 0; k < 4; ++k) ctx->short_split_ms[k] += ms4[k]; }
ltr_align_params ctx_params(const ltr_ctx* ctx) { return ctx->params; }
DebugKnobs ctx_debug(const ltr_ctx* ctx) { return ctx->dbg; }
void ctx_note_nw_launch(ltr_ctx* ctx, int kind, int cls, int grid, int takers, int64_t items) {
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  if (kind < 0) ctx->nw_log.clear(); else ctx->nw_log.push_back({kind, cls, grid, takers, items});
}
ltr_stutter_params ctx_stutter_params(const ltr_ctx* ctx) { return ctx->stutter; }
int ctx_device(const ltr_ctx* ctx) { return ctx->device; }
void* ctx_stream(const ltr_ctx* ctx) { return (void*)ctx->stream; }
void* ctx_big_scratch(ltr_ctx* ctx, size_t bytes) {
  if (bytes > ctx->big_bytes) {
    if (ctx->d_big) { (void)hipDeviceSynchronize(); (void)hipFree(ctx->d_big); ctx->d_big = nullptr; ctx->big_bytes = 0; }
    if (hipMalloc(&ctx->d_big, bytes) != hipSuccess) { (void)hipGetLastError(); ctx->d_big = nullptr; return nullptr; }
    ctx->big_bytes = bytes;
  }
  return ctx->d_big;
}
std::unique_lock<std::mutex> ctx_call_lock(ltr_ctx* ctx) { return std::unique_lock<std::mutex>(ctx->call_mu); }
uint8_t* ctx_host_bytes(ltr_ctx* ctx, int which, size_t bytes) {
  (void)hipSetDevice(ctx->device);              // (the caller may be a helper thread of ltr_calc_hap_aln_probs: pinned memory is allocated against the context's device)
  ctx->host_bytes[which & 3].resize(bytes); return ctx->host_bytes[which & 3].data(); }
void* ctx_side_stream(const ltr_ctx* ctx, int k) { k %= (ltr_ctx::kAux + 1); return (void*)(k == 0 ? ctx->stream : ctx->aux[k - 1]); }
}


static void fill_model_consts(const ltr_align_params& p, ModelConsts* mc) {
  *mc = ltrp::model_consts_from(p);
  mc->match = (float)(-0.000100005);     // float MATCH = -0.000100005;  HapAligner.cpp:261
  mc->mismatch = (float)(-9.0);          // float MISMATCH = -9.0;       HapAligner.cpp:260
  volatile float mf = mc->match + mc->f; // float + float, evaluated in float (HapAligner.cpp:277)
  mc->match_plus_f = mf;
}

// Boundary tables of the first row / first column (HapAligner.cpp:267-280): pure functions
// of the model, so they are built once per parameter set instead of once per pair.
int build_tables(ltr_ctx* ctx, int64_t len, bool same_size) {
  // (the kernels stream the column table with a pointer that keeps advancing while the last lanes
  // drain: keep 80 records of slack beyond the longest haplotype)
  if (!same_size) {
    if (len + 80 <= ctx->table_len) return LTR_OK;
    len = std::max<int64_t>(len + len / 4 + 80, 4096);
  }
  const ModelConsts& mc = ctx->mc;
  const double IMP = ltr::kImpossible;
  std::vector<double> lpc(len + 2), cx[2], cz[2];
  lpc[0] = 0.0; lpc[1] = 0.0;
  for (int64_t j = 1; j <= len; ++j) lpc[j + 1] = lpc[j] + (double)mc.c;       // left_prob += LOG_DEL_TO_DEL
  for (int e = 0; e < 2; ++e) {
    cx[e].assign(len + 2, IMP); cz[e].assign(len + 2, IMP);
    const double emit = e ? (double)mc.match : (double)mc.mismatch;
    double lpa = 0.0;                       // left_prob of the column loop
    double I_prev = IMP;                    // insertion_matrix[0]
    for (int64_t i = 1; i <= len + 1; ++i) {
      const double Mv = (I_prev + (double)mc.b) + emit;        // match_matrix[i*m], :276
      const double Iv = (double)mc.match_plus_f + lpa;         // insertion_matrix[i*m], :277
      const double Dv = IMP;                                    // :278
      cx[e][i] = std::max(Mv + (double)mc.e, std::max(Dv + (double)mc.d, Iv + (double)mc.b));
      cz[e][i] = std::max(Mv + (double)mc.g, Dv + (double)mc.c);
      I_prev = Iv;
      lpa += (double)mc.a;                                      // :279
    }
  }
  auto up = [&](double** dst, const std::vector<double>& src) -> int {
    if (*dst) (void)hipFree(*dst);
    *dst = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)dst, src.size() * sizeof(double)));
    HIP_TRY(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice));
    return LTR_OK;
  };
  // plans may be executing on caller-supplied streams: nothing may still read the old tables
  HIP_TRY(ctx, hipDeviceSynchronize());
  int rc;
  if ((rc = up(&ctx->d_lpc, lpc))) return rc;
  {
    std::vector<double> xz((size_t)(len + 2) * 4);
    for (int64_t i = 0; i < len + 2; ++i)
      for (int e = 0; e < 2; ++e) { xz[(size_t)(i * 4 + e * 2)] = cx[e][i]; xz[(size_t)(i * 4 + e * 2 + 1)] = cz[e][i]; }
    if ((rc = up(&ctx->d_colXZ, xz))) return rc;
  }
  {
    // first row (HapAligner.cpp:267-272) as the packed kernels consume it: X(0,j), Y(0,j) -- the two max-terms row 1
    // reads -- for both outcomes of the row's emission test; the operations and their order are the kernels' own
    // set-up code (ltr_dp_kernel.hpp, column_block: row0), so the bits are
    std::vector<double> xy((size_t)(len + 2) * 4, IMP);
    const double cg = (double)mc.g, cd = (double)mc.d, ce = (double)mc.e, cb = (double)mc.b, cf = (double)mc.f, ca = (double)mc.a;
    for (int64_t j = 1; j <= len + 1; ++j)
      for (int e = 0; e < 2; ++e) {
        const double lp1 = lpc[(size_t)std::max<int64_t>(j - 1, 0)], lp = lpc[(size_t)j];
        const double D0jm1 = (j == 1) ? IMP : (cg + lp1);                 // deletion_matrix[j-1]
        const double D0j = cg + lp;                                       // deletion_matrix[j] = g + left_prob
        const double M0 = (D0jm1 + cd) + (e ? (double)mc.match : (double)mc.mismatch);
        xy[(size_t)(j * 4 + e * 2)] = std::max(M0 + ce, std::max(D0j + cd, IMP + cb));
        xy[(size_t)(j * 4 + e * 2 + 1)] = std::max(M0 + cf, IMP + ca);
      }
    if ((rc = up(&ctx->d_row0XY, xy))) return rc;
  }
  {
    std::vector<double> thr((size_t)kPenTabDoubles);
    ltrp::build_threshold_table(mc.c, thr.data());
    if ((rc = up(&ctx->d_thr, thr))) return rc;
  }
  ctx->table_len = len;
  return LTR_OK;
}

static int validate_params(const ltr_align_params* p) {
  if (!p) return LTR_ERR_INVALID;
  if (p->indel_flank_len < 0 || p->indel_flank_len > ltr::kRefFlankLen) return LTR_ERR_INVALID;
  const float v[7] = {p->log_ins_to_ins, p->log_ins_to_match, p->log_del_to_del, p->log_del_to_match,
                      p->log_match_to_match, p->log_match_to_ins, p->log_match_to_del};
  for (float x : v) if (!(x < 0.0f) || !std::isfinite(x)) return LTR_ERR_INVALID;   // hipstr_main.cpp:429-430
  return LTR_OK;
}

extern "C" {

const char* ltr_version(void) { return LTR_VERSION_STR; }
int ltr_abi_version(void) { return LTR_ABI_VERSION; }
int ltr_num_kernels(void) { return kNumKernels; }
int ltr_kernel_lanes_per_pair(int k) {
  if (k < 0 || k >= kNumKernels) return 64;
  if (k >= kNumFast) return (k - kNumFast == kXWg4) ? 256 : ((k - kNumFast == kXWg8) ? 512 : 64);
  const ClassInfo ci = class_info(k);
  return ci.family == kFamPack ? (1 << ci.lp_shift) : 64 * ci.waves;
}
int ltr_kernel_family(int k) {
  if (k < 0 || k >= kNumKernels) return -1;
  if (k >= kNumFast) return 3;
  return class_info(k).family == kFamShare ? (int)kFamWg : class_info(k).family;     // (the family class: a launch of its own beside the plan kernel)
}

void ltr_default_params(ltr_align_params* p) {
  // AlignmentModel(10, -1.0, -0.458675, -1.0, -0.458675, -0.00005800168, -10.448214728, -10.448214728)
  // (reference HapAligner.h:118): double literals narrowed to the float members.
  p->log_ins_to_ins = (float)(-1.0);
  p->log_ins_to_match = (float)(-0.458675);
  p->log_del_to_del = (float)(-1.0);
  p->log_del_to_match = (float)(-0.458675);
  p->log_match_to_match = (float)(-0.00005800168);
  p->log_match_to_ins = (float)(-10.448214728);
  p->log_match_to_del = (float)(-10.448214728);
  p->indel_flank_len = 5;
  p->use_short_path = 0;
}

void ltr_default_stutter_params(ltr_stutter_params* p) {
  // the CLI always installs this fixed model (reference hipstr_main.cpp:140,362-363)
  p->in_geom = 0.95; p->in_up = 0.05; p->in_down = 0.05; p->out_geom = 0.95; p->out_up = 0.01; p->out_down = 0.01;
}

int ltr_ctx_set_pair_packing(ltr_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 8) return LTR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->pair_packing = mode;
  return LTR_OK;
}

int ltr_ctx_set_debug(ltr_ctx* ctx, const char* key, double value) {
  if (!ctx || !key) return LTR_ERR_INVALID;
  std::unique_lock<std::mutex> lk(ctx->mu);
  const std::string k(key);
  if (k == "fan_lanes") ctx->dbg.fan_lanes = (int)value;
  else if (k == "fan_pairs") ctx->dbg.fan_pairs = (int64_t)value;
  else if (k == "chunks") ctx->dbg.chunks = (int64_t)value;
  else if (k == "prep_ahead") ctx->dbg.prep_ahead = (int)value;
  else if (k == "chunk_streams") ctx->dbg.chunk_streams = (int)value;
  else if (k == "chunk_growth") { ctx->dbg.chunk_growth = value; ctx->dbg.chunk_growth_set = true; }
  else if (k == "trace") { ctx->dbg.trace = (int)value; ltr::g_trace.store((int)value); }
  else if (k == "fold_rounds") ctx->dbg.fold_rounds = (int)value;
  else if (k == "pack_rule") ctx->dbg.pack_rule = (int)value;
  else if (k == "no_multi") ctx->dbg.no_multi = (int)value;
  else if (k == "wg_first_pass") ctx->dbg.wg_first_pass = (int)value;
  else if (k == "compact_plan") ctx->dbg.compact_plan = (int)value;
  else if (k == "short_split") ctx->dbg.short_split = (int)value;
  else if (k == "wgt_keep_waves") ctx->dbg.wgt_keep_waves = (int)value;
  else if (k == "plan_kernel") ctx->dbg.plan_kernel = (int)value;
  else if (k == "plan_share") ctx->dbg.plan_share = (int)value;
  else if (k == "families") ctx->dbg.families = (int)value;
  else if (k == "family_min_rows") ctx->dbg.family_min_rows = (int)value;
  else if (k == "family_spine") ctx->dbg.family_spine = (int)value;
  else if (k == "chain") ctx->dbg.chain = (int)value;
  else if (k == "chain_min_w") ctx->dbg.chain_min_w = (int)value;
  else if (k == "chain_max_w") ctx->dbg.chain_max_w = (int)value;
  else if (k == "wave_clock") ctx->dbg.wave_clock = (int)value;
  else if (k == "grid_cap") ctx->dbg.grid_cap = value > 0.0 ? (int)std::min(value, 1048576.0) : 0;
  else if (k == "poa_group_cap_bytes") ctx->dbg.poa_group_cap_bytes = (int64_t)value;
  else if (k == "poa_call_budget_bytes") ctx->dbg.poa_call_budget_bytes = (int64_t)value;
  else if (k == "pageable_staging" || k == "reset") {            // A/B: 1 = the library's own staging arrays in pageable memory again ("reset": pinned, the default)
    const bool pin = (k == "reset") || value == 0.0;
    if (pin != ctx->host_bytes[0].pinned) {
      // (the staging arrays belong to the call that is running: wait for it -- lock order call_mu before mu, as ltr_calc_hap_aln_probs takes them)
      lk.unlock();
      std::lock_guard<std::mutex> call_lk(ctx->call_mu);
      lk.lock();
      for (RawBuf<uint8_t>& b : ctx->host_bytes) { b.release(); b.n = 0; b.pinned = pin; }
      ctx->scratch.sorted.release(); ctx->scratch.sorted.n = 0; ctx->scratch.sorted.pinned = pin;
    }
    if (k == "reset") ctx->dbg = ltr::DebugKnobs();
  }
  else if (k == "short_lane_kernel") ctx->dbg.short_lane_kernel = (int)value;
  else if (k == "ll_chunk_loci") ctx->dbg.ll_chunk_loci = (int64_t)value;
  else { ltr::set_error(ctx, "ltr_ctx_set_debug: unknown key " + k); return LTR_ERR_INVALID; }
  return LTR_OK;
}

int ltr_ctx_set_stutter_params(ltr_ctx* ctx, const ltr_stutter_params* p) {
  if (!ctx || !p) return LTR_ERR_INVALID;
  // StutterModel constructor asserts (stutter_model.h:37-42)
  if (!(p->in_geom > 0 && p->in_geom < 1 && p->out_geom > 0 && p->out_geom < 1 && p->in_up > 0 && p->in_down > 0 &&
        p->out_up > 0 && p->out_down > 0 && p->in_up + p->in_down + p->out_up + p->out_down < 1)) {
    ltr::set_error(ctx, "invalid stutter model"); return LTR_ERR_INVALID;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->stutter = *p;
  return LTR_OK;
}

int ltr_ctx_create(int device_ordinal, ltr_ctx** out) {
  if (!out) return LTR_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return LTR_ERR_NO_DEVICE;
  if (device_ordinal < 0 || device_ordinal >= ndev) return LTR_ERR_NO_DEVICE;
  ltr_ctx* ctx = new ltr_ctx();
  ctx->device = device_ordinal;
  if (hipSetDevice(device_ordinal) != hipSuccess) { delete ctx; return LTR_ERR_NO_DEVICE; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) { delete ctx; return LTR_ERR_HIP; }
  ctx->arch = prop.gcnArchName;
  ctx->n_cu = prop.multiProcessorCount;
  ctx->clock_mhz = prop.clockRate / 1000;
  for (RawBuf<uint8_t>& hb : ctx->host_bytes) hb.pinned = true;   // staging of ltr_calc_hap_aln_probs' chunks: uploaded by ltr_plan_create
  ctx->scratch.sorted.pinned = true;                              // the sorted pair descriptors: uploaded by ltr_plan_create
  ctx->compact_stage.pinned = true;                               // the one-block image of a compact plan
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return LTR_ERR_HIP; }
  if (hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking) != hipSuccess) { ltr_ctx_destroy(ctx); return LTR_ERR_HIP; }
  for (int k = 0; k < ltr_ctx::kAux; ++k)
    if (hipStreamCreateWithFlags(&ctx->aux[k], hipStreamNonBlocking) != hipSuccess) { ltr_ctx_destroy(ctx); return LTR_ERR_HIP; }
  ltr_default_params(&ctx->params);
  ltr_default_stutter_params(&ctx->stutter);
  fill_model_consts(ctx->params, &ctx->mc);
  *out = ctx;
  return LTR_OK;
}

}  // extern "C"

// what a DevLease takes from its context (ltr_lease.h); recycled events / pinned blocks (see ltr_ctx: compact plans)
DevPool& ctx_pool(ltr_ctx* ctx) { return ctx->pool; }
hipEvent_t ctx_take_event(ltr_ctx* ctx, bool timing) {
  {
    std::lock_guard<std::mutex> lk(ctx->cache_mu);
    std::vector<hipEvent_t>& c = ctx->ev_cache[timing ? 1 : 0];
    if (!c.empty()) { hipEvent_t e = c.back(); c.pop_back(); return e; }
  }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return e;
}
void ctx_give_event(ltr_ctx* ctx, hipEvent_t e, bool timing) {
  if (!e) return;
  if (!ctx) { (void)hipEventDestroy(e); return; }
  std::lock_guard<std::mutex> lk(ctx->cache_mu);
  std::vector<hipEvent_t>& c = ctx->ev_cache[timing ? 1 : 0];
  if (c.size() < 64) c.push_back(e); else (void)hipEventDestroy(e);
}
double* ctx_take_pinned(ltr_ctx* ctx, size_t bytes, size_t* cap_out, double** dev_out) {
  std::lock_guard<std::mutex> lk(ctx->cache_mu);
  for (ltr_ctx::PinBlock& b : ctx->pin_blocks) if (!b.busy && b.cap >= bytes) { b.busy = true; *cap_out = b.cap; *dev_out = (double*)b.dev; return (double*)b.p; }
  size_t cap = 4096;
  while (cap < bytes) cap <<= 1;
  void* p = nullptr;
  void* d = nullptr;
  if (hipHostMalloc(&p, cap, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || !d) { (void)hipGetLastError(); (void)hipHostFree(p); return nullptr; }
  ctx->pin_blocks.push_back({p, d, cap, true});
  *cap_out = cap; *dev_out = (double*)d;
  return (double*)p;
}
void ctx_give_pinned(ltr_ctx* ctx, void* p) {
  if (!p) return;
  if (!ctx) return;                                              // (the context freed its blocks when it went)
  std::lock_guard<std::mutex> lk(ctx->cache_mu);
  for (ltr_ctx::PinBlock& b : ctx->pin_blocks) if (b.p == p) { b.busy = false; return; }
}

extern "C" {

void ltr_ctx_destroy(ltr_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // plans that outlive their context keep working as handles (destroy is still legal) but lose
  // their device memory here
  for (ltr_plan* plan : ctx->plans) { release_plan_buffers(plan, ctx); plan->ctx = nullptr; plan->last_stream = nullptr; }
  ctx->plans.clear();
  if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
  if (ctx->up_stream) { (void)hipStreamSynchronize(ctx->up_stream); (void)hipStreamDestroy(ctx->up_stream); }
  for (int k = 0; k < ltr_ctx::kAux; ++k) if (ctx->aux[k]) { (void)hipStreamSynchronize(ctx->aux[k]); (void)hipStreamDestroy(ctx->aux[k]); }
  ctx->pool.clear();
  if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  for (ltr_ctx::WgStatSlot& sl : ctx->wg_stat) if (sl.ev) (void)hipEventDestroy(sl.ev);
  for (std::vector<hipEvent_t>& c : ctx->ev_cache) for (hipEvent_t e : c) (void)hipEventDestroy(e);
  for (ltr_ctx::PinBlock& b : ctx->pin_blocks) (void)hipHostFree(b.p);
  if (ctx->compact_ev) (void)hipEventDestroy(ctx->compact_ev);
  if (ctx->wg_stat_pin) (void)hipHostFree(ctx->wg_stat_pin);
  if (ctx->d_big) (void)hipFree(ctx->d_big);
  if (ctx->d_lpc) (void)hipFree(ctx->d_lpc);
  if (ctx->d_colXZ) (void)hipFree(ctx->d_colXZ);
  if (ctx->d_row0XY) (void)hipFree(ctx->d_row0XY);
  if (ctx->d_thr) (void)hipFree(ctx->d_thr);
  delete ctx;
}

int ltr_ctx_set_params(ltr_ctx* ctx, const ltr_align_params* p) {
  if (!ctx) return LTR_ERR_INVALID;
  if (validate_params(p) != LTR_OK) { ltr::set_error(ctx, "invalid alignment parameters (transitions must be < 0, 0 <= indel_flank_len <= 35)"); return LTR_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->params = *p;
  fill_model_consts(ctx->params, &ctx->mc);
  ctx->wg_thr_first = 0; ++ctx->wg_epoch;                        // (what was learnt about the workgroup classes' first pass belonged to the old model)
  const int64_t want = ctx->table_len;
  ctx->table_len = 0;                       // force rebuild with the new transitions
  (void)hipSetDevice(ctx->device);
  return want > 0 ? build_tables(ctx, want, true) : LTR_OK;      // same length: plans made earlier stay covered
}

const char* ltr_last_error(const ltr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ltr_ctx_device_info(const ltr_ctx* ctx, char* arch, int arch_len, int* n_cu, int* clock_mhz) {
  if (!ctx) return LTR_ERR_INVALID;
  if (arch && arch_len > 0) { std::snprintf(arch, (size_t)arch_len, "%s", ctx->arch.c_str()); }
  if (n_cu) *n_cu = ctx->n_cu;
  if (clock_mhz) *clock_mhz = ctx->clock_mhz;
  return LTR_OK;
}

int ltr_ctx_timers(ltr_ctx* ctx, ltr_timers* out, int reset) {
  if (!ctx || !out) return LTR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  *out = ctx->tm;
  if (reset) ctx->tm = ltr_timers{};
  return LTR_OK;
}

int ltr_ctx_short_kernel_split(ltr_ctx* ctx, double out_ms[4], int reset) {
  if (!ctx || !out_ms) return LTR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  for (int k = 0; k < 4; ++k) { out_ms[k] = ctx->short_split_ms[k]; if (reset) ctx->short_split_ms[k] = 0.0; }
  return LTR_OK;
}

int ltr_ctx_timers_n(ltr_ctx* ctx, void* out, size_t out_bytes, int reset) {
  if (!ctx || !out) return LTR_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  std::memcpy(out, &ctx->tm, std::min(out_bytes, sizeof(ltr_timers)));
  if (reset) ctx->tm = ltr_timers{};
  return LTR_OK;
}

}  // extern "C"
