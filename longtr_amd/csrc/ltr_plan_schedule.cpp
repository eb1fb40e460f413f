// ltr_plan_schedule.cpp -- class statistics and the launch schedule of a described batch (ltr_plan.h), and the pure pieces
// of ltr_plan_execute: threshold_groups, pack_ranges.

#include <cstring>

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace ltrp {

// Blocks of the sorted pairs on the host cores (a block spans a few classes; a class's pairs are one contiguous range), partial
// sums merged in block order.
void class_stats(const BatchPlan& d, const BatchScratch& w, ClassStats* st) {
  const RawBuf<PairDesc>& sorted = w.sorted; const RawBuf<int32_t>& order = w.order; const RawBuf<int16_t>& key = w.key;
  const size_t np = sorted.size();
  const int64_t n_blk = (int64_t)((np + kPlanBlock - 1) / kPlanBlock);
  struct Part { int k0 = 0, k1 = -1; std::vector<double> cl; std::vector<int32_t> cm; };
  std::vector<Part> parts((size_t)n_blk);
  auto class_of = [&](size_t i) { int k = 0; while (d.bin_first[k + 1] <= (int)i) ++k; return k; };
  ltr::parallel_for(n_blk, np < 20000 ? n_blk + 1 : 1, [&](int64_t c) {                         // (a one-locus plan: not worth waking the worker pool)
    const size_t i0 = (size_t)c * kPlanBlock, i1 = std::min(np, i0 + kPlanBlock);
    Part& P = parts[(size_t)c];
    int k = class_of(i0);
    P.k0 = k; P.k1 = k;
    double cl = 0.0; int32_t cm = 0;
    for (size_t i = i0; i < i1; ++i) {
      while (d.bin_first[k + 1] <= (int)i) { P.cl.push_back(cl); P.cm.push_back(cm); cl = 0.0; cm = 0; ++k; P.k1 = k; }
      if (key[(size_t)order[i]] > 0) cl += (double)sorted[i].n * (double)sorted[i].m;
      cm = std::max(cm, sorted[i].m - 1);
    }
    P.cl.push_back(cl); P.cm.push_back(cm);
  }, 1);
  *st = ClassStats();
  for (const Part& P : parts)
    for (int k = P.k0; k <= P.k1 && np > 0; ++k) {
      const double cl = P.cl[(size_t)(k - P.k0)];
      if (k < kNumFast) { st->bin_cells[k] += cl; st->cls_cmax[k] = std::max(st->cls_cmax[k], P.cm[(size_t)(k - P.k0)]); }
      else if (k < kNumKernels) st->x_cells[k - kNumFast] += cl;
    }
}

int Schedule::find(const std::vector<Launch>& list, const int k) {
  for (size_t i = 0; i < list.size(); ++i) if (list[i].cls == k) return (int)i;
  return -1;
}

int Schedule::ranges(const Launch& L, const int* bin_first, int32_t* lanes_per_pair, int32_t* strip_width, int64_t* n_pairs) const {
  if (L.kind == kLaunchOne || L.kind == kLaunchWg) return 0;
  int nr = 0;                                      // (at most kNumBins + kNumPack ranges: the caller's arrays hold ltr_num_kernels() entries)
  auto range = [&](int k, int lanes) {
    if (lanes_per_pair) lanes_per_pair[nr] = lanes;
    if (strip_width) strip_width[nr] = class_info(k).W;
    if (n_pairs) n_pairs[nr] = bin_first[k + 1] - bin_first[k];
    ++nr;
  };
  for (int i = 0; i < L.n_one; ++i) range(L.members[i], 64);
  for (int i = L.n_one; i < L.n_one + L.n_pack; ++i)
    for (int sft = kPackMaxShift; sft >= kPackMinShift; --sft) {
      const int k = pack_class(sft, class_info(L.members[i]).W);
      if (bin_first[k + 1] > bin_first[k]) range(k, 1 << sft);
    }
  return nr;
}

void Schedule::cap_grids(const int cap) {
  for (std::vector<Launch>* list : {&launches, &by_class})
    for (Launch& L : *list) if (L.kind == kLaunchOne || L.kind == kLaunchMulti || L.kind == kLaunchPlan || L.kind == kLaunchFamily) L.grid = std::min(L.grid, cap);
  for (int c = 0; c <= kXLong; ++c) x_grid[c] = std::min(x_grid[c], cap);
  max_grid = std::min(max_grid, cap);
}

void Schedule::cap_every_grid(const int cap) {
  for (std::vector<Launch>* list : {&launches, &by_class}) for (Launch& L : *list) L.grid = std::min(L.grid, cap);
  for (int c = 0; c < kNumExact; ++c) x_grid[c] = std::min(x_grid[c], cap);      // (0 stays 0: not launched)
  max_grid = std::min(max_grid, cap);
  max_grid_wide = std::min(max_grid_wide, cap);
}

namespace {

// grid and "small" flag of a persistent launch with work for wgs workgroups where `full` are resident
void size_launch(Launch* L, const int wgs, const int full) { L->grid = std::min(full, std::max(wgs, 1)); L->small = wgs < full; }
int blocks_of(const int waves) { return (waves + kBlockWaves - 1) / kBlockWaves; }
void absorb(Launch* G, const Launch& L) { G->pairs += L.pairs; G->cells += L.cells; G->cmax = std::max(G->cmax, L.cmax); }

// The plan kernel's entries: every one-wave class, every packed width (table t of pack_tabs), the entry with the longest
// pairs first (modelled steps x strip cost of its longest read); the launch's wavefronts start spread over the entries in
// proportion to their modelled work (cells x (1 + per-step overhead / W)) and walk the table from the top afterwards.
// own: the single-class launches (their cmax, cells).  Returns the wavefronts the table has work for.
struct Ent { PlanEntry e; double longest, work; };
int plan_kernel_entries(BatchPlan* d, const ClassStats& st, const ltr::DebugKnobs& dbg, const std::vector<Launch>& own, const Launch& P,
                        const int32_t pack_cmax, const std::vector<PackTable>& tabs, std::vector<Ent>* ents) {
  const int* bf = d->bin_first;
  int waves_all = 0;
  auto own_of = [&](int k) -> const Launch& { for (const Launch& L : own) if (L.cls == k) return L; return P; };
  // (the entry of the class the launch is listed under is costed with the longest read of the LAUNCH, the first packed width
  // with the longest read of any packed width: how the merged maxima have entered this model since the plan kernel was measured)
  for (int i = 0; i < P.n_one; ++i) {
    const int k = P.members[i], w = class_info(k).W, np = bf[k + 1] - bf[k];
    const int32_t cm = (k == P.cls) ? P.cmax : st.cls_cmax[k];
    PlanEntry e; std::memset(&e, 0, sizeof(e));
    e.kind = 0; e.W = w; e.first = bf[k]; e.n_pairs = np; e.queue_class = k; e.tab = 0; e.limit = np;
    // the chained walk (ltr_dp_chain.hpp: no fill and drain of the skew between the pairs of a class; on request) for the strip
    // widths whose reads fill the wave's scratch strip, where the next pair's first row is parked
    {
      const int64_t need = 2 * (int64_t)w * 64 + ((w + 3) / 4) * 32 + 2;
      const int64_t have = 6 * (int64_t)(((d->max_len + 2 + 15) / 16) * 16);
      const int lo = dbg.chain_min_w > 0 ? dbg.chain_min_w : kMultiMinW, hi = dbg.chain_max_w > 0 ? dbg.chain_max_w : kWMax;
      if (dbg.chain > 0 && d->sym_at_create && w >= std::max(lo, (int)kMultiMinW) && w <= hi && need <= have) e.kind = 3;   // (off by default: measured slower, ltr_dp_chain.hpp)
    }
    const int ncb = (cm + 64 * w - 1) / (64 * w);
    ents->push_back({e, (double)std::max(ncb, 1) * (cm + 64.0) * (w + 1.5), st.bin_cells[k] * (1.0 + 1.5 / w)});
    waves_all += np;
  }
  for (size_t t = 0; t < tabs.size(); ++t) {
    const PackTable& T = tabs[t];
    const Launch& L = own_of(T.queue_class);
    PlanEntry e; std::memset(&e, 0, sizeof(e));
    e.kind = 1; e.W = T.W; e.queue_class = T.queue_class; e.tab = (int32_t)t; e.limit = T.grp_end[4];
    const int32_t cm = (t == 0) ? pack_cmax : L.cmax;
    const int lp = 1 << class_info(T.queue_class).lp_shift;      // (listed under its widest lanes-per-pair class with pairs)
    ents->push_back({e, (cm + (double)lp) * (T.W + 1.5), L.cells * (1.0 + 1.5 / T.W)});
    waves_all += e.limit;
  }
  // The pairs that START OUT in an exact list -- bytes outside ACGT, length differences no certificate can hold
  // (Rules::risky_dd_pos / _neg) -- are scored by the plan kernel itself, FIRST: they are the longest jobs of the plan (an exact body of
  // 1 - 3 ms per pair on one wavefront).  (Measured on MI355X, 1250 loci of config 3: as launches of their own beside the plan
  // kernel they found no free wave slot before its workgroups left and the pass ended 3 ms after the plan kernel, 34.0 ms; as
  // its last work they were its tail, 33.8 ms; first, 30.4 ms.)  The exact launches of such a plan only take what the
  // workgroup classes queue on the device.
  for (int c = 0; c < kNumExact; ++c) {
    const int np = bf[kNumFast + c + 1] - bf[kNumFast + c];
    d->x_seed[c] = 0;
    if (np <= 0) continue;
    PlanEntry e; std::memset(&e, 0, sizeof(e));
    e.kind = 2; e.W = (c == kXGeneric) ? 0 : 1; e.first = bf[kNumFast + c]; e.n_pairs = np; e.queue_class = kStartQueueSlot + c; e.limit = np;   // (a counter of its own: list c's exact launch may run as well, fed by the workgroup classes)
    ents->push_back({e, 1e30 - c, st.x_cells[c] * 1.4});
    waves_all += np;
  }
  std::stable_sort(ents->begin(), ents->end(), [](const Ent& x, const Ent& y) { return x.longest > y.longest; });
  return waves_all;
}

}  // namespace

void build_schedule(BatchPlan* d, const ClassStats& st, const OccupancyGrids& occ, const ltr::DebugKnobs& dbg, Schedule* S) {
  const int* bf = d->bin_first; const int* counts = d->counts;
  *S = Schedule();
  S->launches.reserve(kNumFast); S->by_class.reserve(kNumFast);
  // ---- a launch per class, in descending class order.  The packed classes of one strip width -- 32, 16, 8, 4, 2 lanes per
  // pair -- are ONE launch (ltr_dp_pack.hpp), listed under the first of them that has pairs and as long as the longest read of
  // any of them; a packed wave takes 64 / LP pairs
  for (int k = kNumFast - 1; k >= 0; --k) {
    if (bf[k + 1] <= bf[k]) continue;
    const ClassInfo ci = class_info(k);
    Launch L;
    L.cls = k; L.W = ci.W; L.members[0] = (int16_t)k;
    if (ci.family == kFamPack) {
      bool listed = false;
      for (int sft = kPackMaxShift; sft > ci.lp_shift; --sft) listed = listed || bf[pack_class(sft, ci.W) + 1] > bf[pack_class(sft, ci.W)];
      if (listed) continue;
      int waves = 0;
      for (int sft = kPackMinShift; sft <= kPackMaxShift; ++sft) {
        const int k2 = pack_class(sft, ci.W), per = 64 >> sft;
        waves += (counts[k2] + per - 1) / per;
        L.pairs += bf[k2 + 1] - bf[k2]; L.cells += st.bin_cells[k2]; L.cmax = std::max(L.cmax, st.cls_cmax[k2]);
      }
      L.kind = kLaunchPack; L.n_pack = 1;
      size_launch(&L, blocks_of(waves), occ.cls[k]);
    } else {
      L.pairs = bf[k + 1] - bf[k]; L.cells = st.bin_cells[k]; L.cmax = st.cls_cmax[k];
      if (ci.family == kFamShare) { L.kind = kLaunchFamily; L.W = 0; size_launch(&L, blocks_of((int)d->fams.size()), occ.cls[k]); }   // one family per wavefront at a time
      else if (ci.family == kFamWg) { L.kind = kLaunchWg; size_launch(&L, counts[k], occ.cls[k]); }      // one pair per workgroup, no scratch strips
      else { L.kind = kLaunchOne; L.n_one = 1; size_launch(&L, blocks_of(counts[k]), occ.cls[k]); }
    }
    S->by_class.push_back(L);
  }
  // ---- the launches that take several of those: in automatic mode, large plans, the one-wave classes of strip widths
  // kMultiMinW .. kWMax are ONE launch (ltr_dp_multi_kernel) and so are the packed widths kPackMultiMinW .. kPackWMax
  // (ltr_dp_pack_multi_kernel), each where at least two have pairs; under the plan kernel EVERY one-wave class and every packed
  // width is one launch.  Each is listed under the widest of its members
  const bool use_plan = d->use_plan, shared = use_plan || d->use_multi;
  Launch M, PM;
  M.kind = kLaunchMulti; PM.kind = kLaunchPackMulti;
  int waves_one = 0;
  for (int k = kNumBins - 1; shared && k >= (use_plan ? 0 : kMultiMinW - 1); --k) if (bf[k + 1] > bf[k]) { M.members[M.n_one++] = (int16_t)k; waves_one += counts[k]; }
  for (int w = kPackWMax; shared && w >= (use_plan ? 1 : kPackMultiMinW); --w)
    for (const Launch& L : S->by_class) if (L.kind == kLaunchPack && L.W == w) PM.members[PM.n_pack++] = (int16_t)L.cls;
  if (M.n_one < (use_plan ? 1 : 2)) M.n_one = 0;
  if (PM.n_pack < (use_plan ? 1 : 2)) PM.n_pack = 0;
  auto group_of = [&](const Launch& L) -> Launch* {
    if (L.kind == kLaunchOne && M.n_one > 0 && (use_plan || L.W >= kMultiMinW)) return &M;
    if (L.kind == kLaunchPack && PM.n_pack > 0 && (use_plan || L.W >= kPackMultiMinW)) return &PM;
    return nullptr;
  };
  for (const Launch& L : S->by_class) if (Launch* G = group_of(L)) absorb(G, L);
  M.cls = M.members[0]; PM.cls = PM.members[0];
  // one range table per packed width (its ranges as the single-width launch would get them), widest first
  int groups_all = 0;
  for (int i = 0; i < PM.n_pack; ++i) {
    PackTable T;
    std::memset(&T, 0, sizeof(T));
    T.W = class_info(PM.members[i]).W; T.queue_class = PM.members[i];
    pack_ranges(bf, T.W, T.shift, T.first, T.end, T.grp_end);
    groups_all += T.grp_end[4];
    S->pack_tabs.push_back(T);
  }
  size_launch(&M, blocks_of(waves_one), occ.multi);
  size_launch(&PM, blocks_of(groups_all), occ.pack_multi);
  // (the scratch strips have always been sized for the multi-width one-wave launch of the plan kernel's classes too)
  if (M.n_one > 0) S->max_grid = std::max(S->max_grid, M.grid);
  Launch P;
  if (use_plan && M.n_one + PM.n_pack == 0) {
    // nothing for the plan kernel to score (workgroup classes and list starters only): the exact launches take the starters
    d->use_plan = false;
    for (int c = 0; c < kNumExact; ++c) d->xcand[c] += d->xstart[c];
  } else if (use_plan) {
    P = M;
    P.kind = kLaunchPlan; P.n_pack = PM.n_pack;
    for (int i = 0; i < PM.n_pack; ++i) P.members[P.n_one + i] = PM.members[i];
    if (P.n_one == 0) P.cls = PM.cls;
    absorb(&P, PM);
    std::vector<Ent> ents;
    const int waves_all = plan_kernel_entries(d, st, dbg, S->by_class, P, PM.cmax, S->pack_tabs, &ents);
    size_launch(&P, blocks_of(waves_all), occ.plan);
    double total = 0.0, run = 0.0;
    for (const Ent& x : ents) total += x.work;
    const double n_waves = (double)P.grid * kBlockWaves;
    for (Ent& x : ents) {
      x.e.first_wave = total > 0.0 ? (int32_t)std::min(n_waves, std::floor(n_waves * run / total)) : 0;
      run += x.work;
      S->plan_entries.push_back(x.e);
    }
    if (!S->plan_entries.empty()) S->plan_entries[0].first_wave = 0;
    // (Measured on MI355X, plan kernel with the shares against every wavefront starting at the top of the table
    // (ltr_ctx_set_debug "plan_share" = 1): shards of config 3 of 625 / 1250 / 2500 / 5000 loci 15.5 - 15.6 against 15.8 - 16.0 ms,
    // 30.2 against 30.4, 59.4 both, 125.8 against 125.1 - 125.5; shards of the catalogue of 6250 / 12 500 loci 4.57 against 4.99,
    // 8.09 against 8.54 -- 3072 wavefronts racing down a table of 30 - 40 short entries pop every counter 3072 times.  While
    // failed certificates still ended the launch (first version) the shares looked worse: 32.28 against 31.68 ms at 1250 loci.)
    if (dbg.plan_share == 1) for (size_t i = 1; i < S->plan_entries.size(); ++i) S->plan_entries[i].first_wave = 0x7fffffff;
  }
  // ---- launch order: longest reads first (the classes that can feed the exact lists of long reads are through early, and those
  // lists' launches -- a handful of pairs, each as long as its longest pair -- run beside the remaining certificate launches
  // instead of behind the last one); a launch over several classes is as long as the longest read of any of them
  for (const Launch& L : S->by_class) {
    const Launch* G = d->use_plan ? ((L.kind == kLaunchWg || L.kind == kLaunchFamily) ? nullptr : &P) : group_of(L);
    if (!G) S->launches.push_back(L);
    else if (G->cls == L.cls) S->launches.push_back(*G);
  }
  auto longer = [](const Launch& x, const Launch& y) { return x.cmax > y.cmax; };
  std::stable_sort(S->launches.begin(), S->launches.end(), longer);
  std::stable_sort(S->by_class.begin(), S->by_class.end(), longer);
  // the family launch first: it deals its families out statically, so what its last wavefronts still hold is filled by the plan
  // kernel's first pairs behind it, not by nothing
  for (std::vector<Launch>* list : {&S->launches, &S->by_class}) {
    const auto it = std::find_if(list->begin(), list->end(), [](const Launch& L) { return L.kind == kLaunchFamily; });
    if (it != list->end()) std::rotate(list->begin(), it, it + 1);
  }
  for (const std::vector<Launch>* list : {&S->launches, &S->by_class})
    for (const Launch& L : *list) if (L.kind == kLaunchOne || L.kind == kLaunchPlan || L.kind == kLaunchFamily) S->max_grid = std::max(S->max_grid, L.grid);   // (the family launch: its exact bodies index the strips by workgroup)
  // exact kernels: launched only when some pair of the plan can land in their list
  for (int c = 0; c < kNumExact; ++c) {
    if (d->xcand[c] <= 0) continue;
    const bool wgx = (c == kXWg4 || c == kXWg8);
    const int64_t wgs = wgx ? d->xcand[c] : (d->xcand[c] + kBlockWaves - 1) / kBlockWaves;
    S->x_grid[c] = (int)std::min<int64_t>(occ.exact[c], std::max<int64_t>(wgs, 1));
    if (!wgx) S->max_grid = std::max(S->max_grid, S->x_grid[c]);      // (the one-wave kernels park column blocks in scratch strips)
  }
  S->max_grid_wide = (int)std::max<int64_t>(1, std::min<int64_t>((d->xcand[kXWg4] + kBlockWaves - 1) / kBlockWaves, 1 << 20));
}

// Threshold first pass: which kernel scores a workgroup class, and which classes share a launch.  The threshold kernels carry
// two quads of thresholds on top of the certificate body's registers: the wide four-wave strips (W = 15 .. 20, reads of 3586 ..
// 5121 bases) would run at two waves per SIMD -- such a class goes to EIGHT waves with strips half as wide (8 / 10 columns: 128
// registers, two workgroups = four waves per SIMD); the geometry follows the kernel.  Classes that are neighbours in the sorted
// pair list and end up on eight waves with strips of up to LTR_WGT_LB4_MAXW columns (the wide four-wave classes and the eight-wave
// classes W = 8 .. 10: a batch of 5-kb pairs that the certificate rules split into whole rounds of four-wave workgroups plus a
// rest) are ONE launch of the widest of those kernels: one ramp, one tail, no two persistent launches fighting for the same
// wave slots.  (Not under per-launch timing: every class keeps its own launch and its own time then.)
ThresholdGroups threshold_groups(const int* bin_first, const bool merge, const bool keep_waves) {
  ThresholdGroups G;
  int lead = -1;
  for (int k = kWg4First; k < kWg1First; ++k) {
    const int np = bin_first[k + 1] - bin_first[k];
    if (np <= 0) continue;
    const ClassInfo ci = class_info(k);
    int nw = ci.waves, w = ci.W;
    if (nw == 4 && w >= ltrp::kWg4WideMinW && !keep_waves) { nw = 8; w = std::max((int)kWg8MinW, (w + 1) / 2); }
    w = threshold_strip_width(w);
    G.nw[k] = nw; G.w[k] = w; G.np[k] = np;
    const bool narrow8 = (nw == 8 && w <= 10);                     // (lead: the narrow eight-wave class the current run of such classes began with)
    if (narrow8 && lead >= 0 && merge && !keep_waves) {
      G.np[lead] += np; G.np[k] = 0;                               // (pairs of consecutive non-empty classes are consecutive in the sorted list)
      G.w[lead] = std::max(G.w[lead], w);
    } else lead = narrow8 ? k : -1;
  }
  return G;
}

void pack_ranges(const int* bin_first, const int W, int32_t* shift, int32_t* first, int32_t* end, int32_t* grp_end) {
  int nr = 0, groups = 0;
  for (int sft = kPackMaxShift; sft >= kPackMinShift; --sft) {
    const int k2 = ltrp::pack_class(sft, W);
    const int c2 = bin_first[k2 + 1] - bin_first[k2];
    if (c2 <= 0) continue;
    const int per = 64 >> sft;
    groups += (c2 + per - 1) / per;
    shift[nr] = sft; first[nr] = bin_first[k2]; end[nr] = bin_first[k2 + 1]; grp_end[nr] = groups;
    ++nr;
  }
  for (; nr < 5; ++nr) { shift[nr] = kPackMaxShift; first[nr] = 0; end[nr] = 0; grp_end[nr] = groups; }
}

}  // namespace ltrp
