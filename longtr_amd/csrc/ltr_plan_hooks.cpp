// ltr_plan_hooks.cpp -- test hooks of the planning units (include/ltr_gpu.h, "planning units"; ltr_plan.h): the rule, the sort,
// the description and the schedule of a batch without a GPU.

#include <cstring>

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace {
// The work arrays of one hook call (a context keeps its own from plan to plan).
struct HookScratch {
  RawBuf<PairDesc> pairs, sorted; RawBuf<int16_t> key, bin; RawBuf<int32_t> order; RawBuf<uint8_t> read_acgt, hap_acgt;
  ltrp::BatchScratch view() { return {pairs, sorted, key, bin, order, read_acgt, hap_acgt}; }
};
}  // namespace

extern "C" {

int ltr_debug_num_classes(void) { return ltrp::kNumKernels; }

int ltr_debug_class_info(int k, int* family, int* strip_width, int* waves_per_pair, int* lanes_per_pair) {
  if (k < 0 || k >= ltrp::kNumKernels) return LTR_ERR_INVALID;
  if (k >= ltrp::kNumFast) {
    const int xc = k - ltrp::kNumFast;
    if (family) *family = ltrp::kFamExact;
    if (strip_width) *strip_width = ltrp::kXW[xc];
    if (waves_per_pair) *waves_per_pair = (xc == kXWg4) ? 4 : ((xc == kXWg8) ? 8 : 1);
    if (lanes_per_pair) *lanes_per_pair = (xc == kXWg4) ? 256 : ((xc == kXWg8) ? 512 : 64);
    return LTR_OK;
  }
  const ltrp::ClassInfo ci = ltrp::class_info(k);
  if (family) *family = ci.family == ltrp::kFamShare ? (int)ltrp::kFamWg : ci.family;
  if (strip_width) *strip_width = ci.W;
  if (waves_per_pair) *waves_per_pair = ci.waves;
  if (lanes_per_pair) *lanes_per_pair = ci.family == ltrp::kFamPack ? (1 << ci.lp_shift) : 64 * ci.waves;
  return LTR_OK;
}

int ltr_debug_classify(const ltr_align_params* p, int mode, int n_cu, int64_t pairs_in_batch, int64_t long_pairs_in_batch,
                       int32_t window_len, int32_t read_len, int32_t hap_full_len, int generic,
                       int* launch_class, int* order_key, int* exact_list) {
  if (!p || n_cu <= 0) return LTR_ERR_INVALID;
  const ModelConsts mc = ltrp::model_consts_from(*p);
  const ltrp::Rules R = ltrp::make_rules(mc, p->indel_flank_len, mode, n_cu, pairs_in_batch, long_pairs_in_batch);
  const ltrp::PairClass pc = ltrp::classify_pair(R, window_len, read_len, hap_full_len, generic != 0);
  if (launch_class) *launch_class = pc.cls;
  if (order_key) *order_key = pc.key;
  if (exact_list) *exact_list = pc.xc;
  return LTR_OK;
}

int ltr_debug_pair_costs(const ltr_align_params* p, int mode, int n_cu, int64_t pairs_in_batch, int64_t long_pairs_in_batch, int64_t n,
                         const int32_t* window_len, const int32_t* read_len, const int32_t* hap_full_len, double* cost) {
  if (!p || n_cu <= 0 || n < 0 || (n > 0 && (!window_len || !read_len || !hap_full_len || !cost))) return LTR_ERR_INVALID;
  const ModelConsts mc = ltrp::model_consts_from(*p);
  const ltrp::Rules R = ltrp::make_rules(mc, p->indel_flank_len, mode, n_cu, pairs_in_batch, long_pairs_in_batch);
  for (int64_t i = 0; i < n; ++i) cost[i] = ltrp::classify_pair(R, window_len[i], read_len[i], hap_full_len[i], false).cost;
  return LTR_OK;
}

int ltr_debug_threshold_table(float log_del_to_del, double* out, int64_t cap) {
  if (!out || cap < kPenTabDoubles || !(log_del_to_del < 0.f)) return LTR_ERR_INVALID;
  ltrp::build_threshold_table(log_del_to_del, out);
  return kPenTabDoubles;
}

int ltr_debug_sort_by_class(const int16_t* launch_class, const int16_t* order_key, int64_t n_pairs, int fold, int n_cu,
                            int32_t* order, int32_t* class_first /* [ltr_debug_num_classes() + 1] */) {
  if ((!launch_class || !order_key || !order) && n_pairs > 0) return LTR_ERR_INVALID;
  if (n_pairs < 0 || n_pairs > 0x7fffffff || !class_first || n_cu <= 0) return LTR_ERR_INVALID;
  for (int64_t i = 0; i < n_pairs; ++i) if (launch_class[i] < 0 || launch_class[i] >= ltrp::kNumKernels || order_key[i] < 0 || order_key[i] > 511) return LTR_ERR_INVALID;
  int bf[ltrp::kNumKernels + 1], counts[ltrp::kNumKernels];
  // fold: 0 = no folding; 1 = automatic mode's folding, a launch per class; 2 = ... with the multi-width launches (plans of
  // 512 .. 4096 pairs per CU before round 5, asymmetric models since); 3 = ... with the plan kernel (no folding in its families)
  try { ltrp::sort_by_class(launch_class, order_key, n_pairs, fold != 0 ? ltrp::kFoldRounds : 0, n_cu, order, bf, counts, fold >= 2 ? fold - 1 : 0); }
  catch (...) { return LTR_ERR_NOMEM; }
  for (int k = 0; k <= ltrp::kNumKernels; ++k) class_first[k] = bf[k];
  return LTR_OK;
}

int ltr_debug_describe_batch(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, int64_t* out_i64, double* out_f64,
                             int32_t* class_first, int64_t pair_cap, int32_t* pair_n, int32_t* pair_m, int64_t* pair_out_idx, int16_t* pair_key,
                             char* err, int err_cap) {
  if (!p || !b || n_cu <= 0 || mode < -1 || mode > 8) return LTR_ERR_INVALID;
  const ModelConsts mc = ltrp::model_consts_from(*p);
  try {
    HookScratch hs;
    const ltrp::BatchScratch w = hs.view();
    ltrp::BatchPlan d;
    std::string why;
    const int rc = ltrp::describe_batch(b, mc, p->indel_flank_len, mode, n_cu, ltr::DebugKnobs(), w, &d, &why);
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", why.c_str());
    if (rc != LTR_OK) return rc;
    if (out_i64) { out_i64[0] = d.n_pairs; out_i64[1] = d.ll_size; out_i64[2] = d.max_len; }
    if (out_f64) { out_f64[0] = d.cells; out_f64[1] = d.input_bytes; }
    if (class_first) for (int k = 0; k <= ltrp::kNumKernels; ++k) class_first[k] = d.bin_first[k];
    for (int64_t i = 0; i < std::min<int64_t>(pair_cap, d.n_pairs); ++i) {
      if (pair_n) pair_n[i] = w.sorted[(size_t)i].n;
      if (pair_m) pair_m[i] = w.sorted[(size_t)i].m;
      if (pair_out_idx) pair_out_idx[i] = w.sorted[(size_t)i].out_idx;
      if (pair_key) pair_key[i] = w.key[(size_t)w.order[(size_t)i]];
    }
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}

int ltr_debug_threshold_groups(const int32_t* class_first, int merge, int keep_waves, int32_t* nw, int32_t* w, int32_t* np) {
  if (!class_first || !nw || !w || !np) return LTR_ERR_INVALID;
  const ltrp::ThresholdGroups G = ltrp::threshold_groups(class_first, merge != 0, keep_waves != 0);
  for (int k = 0; k < ltrp::kNumKernels; ++k) { nw[k] = k < ltrp::kNumFast ? G.nw[k] : 0; w[k] = k < ltrp::kNumFast ? G.w[k] : 0; np[k] = k < ltrp::kNumFast ? G.np[k] : 0; }
  return LTR_OK;
}

int ltr_debug_plan_schedule(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* grids, const int32_t* knobs,
                            int64_t* out, int32_t* x_grid, int launch_cap, int32_t* launch, double* launch_cells, int member_cap, int32_t* members,
                            int entry_cap, int32_t* entry) {
  if (!p || !b || !grids || !knobs || !out || !x_grid || n_cu <= 0 || mode < -1 || mode > 8 || launch_cap < 0 || member_cap < 0 || entry_cap < 0) return LTR_ERR_INVALID;
  if ((launch_cap > 0 && (!launch || !launch_cells)) || (member_cap > 0 && !members) || (entry_cap > 0 && !entry)) return LTR_ERR_INVALID;
  const ModelConsts mc = ltrp::model_consts_from(*p);
  try {
    HookScratch hs;
    const ltrp::BatchScratch w = hs.view();
    ltr::DebugKnobs dbg;
    dbg.plan_kernel = knobs[0]; dbg.no_multi = knobs[1]; dbg.chain = knobs[2]; dbg.chain_min_w = knobs[3]; dbg.chain_max_w = knobs[4]; dbg.plan_share = knobs[5];
    ltrp::BatchPlan d;
    std::string why;
    const int rc = ltrp::describe_batch(b, mc, p->indel_flank_len, mode, n_cu, dbg, w, &d, &why);
    if (rc != LTR_OK) return rc;
    ltrp::ClassStats st;
    ltrp::class_stats(d, w, &st);
    ltrp::OccupancyGrids occ;
    for (int k = 0; k < ltrp::kNumFast; ++k) occ.cls[k] = grids[k];
    for (int c = 0; c < kNumExact; ++c) occ.exact[c] = grids[ltrp::kNumFast + c];
    occ.multi = grids[ltrp::kNumKernels]; occ.pack_multi = grids[ltrp::kNumKernels + 1]; occ.plan = grids[ltrp::kNumKernels + 2];
    ltrp::Schedule S;
    ltrp::build_schedule(&d, st, occ, dbg, &S);
    if (knobs[6] > 0) S.cap_grids(knobs[6]);
    else if (knobs[6] < 0) S.cap_every_grid(knobs[6] == INT32_MIN ? INT32_MAX : -knobs[6]);      // (seven knobs, as ever: the sign picks the cap)
    out[0] = (int64_t)S.launches.size(); out[1] = (int64_t)S.by_class.size(); out[2] = (int64_t)S.plan_entries.size(); out[3] = (int64_t)S.pack_tabs.size();
    out[4] = d.use_plan ? 1 : 0; out[5] = S.max_grid; out[6] = S.max_grid_wide; out[7] = d.max_len;
    for (int c = 0; c < kNumExact; ++c) { out[8 + c] = d.xcand[c]; x_grid[c] = S.x_grid[c]; }
    for (int k = 0; k <= ltrp::kNumKernels; ++k) out[8 + kNumExact + k] = d.bin_first[k];
    int at = 0, n_mem = 0;
    for (const std::vector<ltrp::Launch>* list : {&S.launches, &S.by_class})
      for (const ltrp::Launch& L : *list) {
        const int nm = L.n_one + L.n_pack;
        if (at < launch_cap) {
          const int32_t v[8] = {L.kind, L.cls, L.W, L.grid, L.small ? 1 : 0, L.cmax, (int32_t)L.pairs, nm};
          std::memcpy(launch + (size_t)at * 8, v, sizeof(v));
          launch_cells[at] = L.cells;
        }
        for (int i = 0; i < nm; ++i, ++n_mem) if (n_mem < member_cap) members[n_mem] = L.members[i];
        ++at;
      }
    for (int i = 0; i < std::min((int)S.plan_entries.size(), entry_cap); ++i) {
      const PlanEntry& e = S.plan_entries[(size_t)i];
      const int32_t v[6] = {e.kind, e.W, e.first, e.n_pairs, e.queue_class, e.first_wave};
      std::memcpy(entry + (size_t)i * 6, v, sizeof(v));
    }
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}

int ltr_debug_plan_families(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* knobs, int64_t* out,
                            int fam_cap, int32_t* fam, double* U, int member_cap, int32_t* member_n, int64_t* member_out) {
  if (!p || !b || !knobs || !out || n_cu <= 0 || mode < -1 || mode > 8 || fam_cap < 0 || member_cap < 0) return LTR_ERR_INVALID;
  if ((fam_cap > 0 && (!fam || !U)) || (member_cap > 0 && (!member_n || !member_out))) return LTR_ERR_INVALID;
  ModelConsts mc = ltrp::model_consts_from(*p);
  mc.match = (float)(-0.000100005); mc.mismatch = (float)(-9.0);     // (HapAligner.cpp:260-261; the bound U holds MATCH)
  try {
    HookScratch hs;
    const ltrp::BatchScratch w = hs.view();
    ltr::DebugKnobs dbg;
    dbg.families = knobs[0]; dbg.family_min_rows = knobs[1];
    ltrp::BatchPlan d;
    std::string why;
    const int rc = ltrp::describe_batch(b, mc, p->indel_flank_len, mode, n_cu, dbg, w, &d, &why);
    if (rc != LTR_OK) return rc;
    const int f0 = d.bin_first[ltrp::kFamClass], f1 = d.bin_first[ltrp::kFamClass + 1];
    out[0] = (int64_t)d.fams.size(); out[1] = d.fam_members; out[2] = f0; out[3] = d.n_pairs;
    for (int i = 0; i < std::min((int)d.fams.size(), fam_cap); ++i) {
      const FamilyDesc& f = d.fams[(size_t)i];
      const int32_t v[6] = {f.first, f.count, f.p, f.W, f.dd_min, f.dd_max};
      std::memcpy(fam + (size_t)i * 6, v, sizeof(v));
      U[i] = d.fam_U[(size_t)i];
    }
    for (int i = f0; i < f1 && i - f0 < member_cap; ++i) { member_n[i - f0] = w.sorted[(size_t)i].n; member_out[i - f0] = w.sorted[(size_t)i].out_idx; }
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}

int ltr_debug_plan_family_forks(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* knobs, int64_t* out,
                                int fam_cap, int32_t* fam, int32_t* slot_row, int member_cap, int32_t* member_fork, int32_t* member_slot, int64_t* member_out) {
  if (!p || !b || !knobs || !out || n_cu <= 0 || mode < -1 || mode > 8 || fam_cap < 0 || member_cap < 0) return LTR_ERR_INVALID;
  if ((fam_cap > 0 && (!fam || !slot_row)) || (member_cap > 0 && (!member_fork || !member_slot || !member_out))) return LTR_ERR_INVALID;
  ModelConsts mc = ltrp::model_consts_from(*p);
  mc.match = (float)(-0.000100005); mc.mismatch = (float)(-9.0);     // (as ltr_debug_plan_families)
  try {
    HookScratch hs;
    const ltrp::BatchScratch w = hs.view();
    ltr::DebugKnobs dbg;
    dbg.families = knobs[0]; dbg.family_min_rows = knobs[1]; dbg.family_spine = knobs[2];
    ltrp::BatchPlan d;
    d.keep_forks = true;
    std::string why;
    const int rc = ltrp::describe_batch(b, mc, p->indel_flank_len, mode, n_cu, dbg, w, &d, &why);
    if (rc != LTR_OK) return rc;
    out[0] = (int64_t)d.fams.size(); out[1] = d.fam_members; out[2] = d.fam_with_spine; out[3] = d.fam_rows_saved;
    const int f0 = d.bin_first[ltrp::kFamClass];
    for (int i = 0; i < (int)d.fams.size(); ++i) {
      const FamilyDesc& f = d.fams[(size_t)i];
      const FamilySpine& sp = d.fam_spines[(size_t)i];
      const ltrp::FamilyForks& fk = d.fam_forks[(size_t)i];
      if (i < fam_cap) {
        const int32_t v[10] = {sp.spine, sp.n_slots, (int32_t)fk.steps, kFamilyParkSlots, f.first, f.count, f.p, f.W, f.dd_min, f.dd_max};
        std::memcpy(fam + (size_t)i * 10, v, sizeof(v));
        for (int s = 0; s < kFamilyParkSlots; ++s) slot_row[(size_t)i * kFamilyParkSlots + s] = s < sp.n_slots ? sp.slot_row[s] : 0;
      }
      for (int k = 0; k < f.count; ++k) {
        const int at = f.first + k - f0;
        if (at < 0 || at >= member_cap) continue;
        member_fork[at] = sp.spine < 0 ? f.p : fk.fork[k];
        member_slot[at] = sp.spine < 0 ? 0 : sp.slot_of[k];
        member_out[at] = w.sorted[(size_t)(f.first + k)].out_idx;
      }
    }
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}

}  // extern "C"
