// ltr_plan.h -- host-side planning of a batch (no HIP in here), the one header of these units:
//   ltr_plan_rules.cpp     what the batch as a whole decides (make_rules), the cost model (pack_cost), the rule that gives every
//                          (read, haplotype) pair its launch class and launch-order key (classify_pair), build_threshold_table
//   ltr_plan_sort.cpp      sort_by_class: the pairs class by class, longest first; the fold walk of the under-filled classes
//   ltr_plan_families.cpp  form_families: haplotype families
//   ltr_plan_describe.cpp  describe_batch, the host half of ltr_plan_create that strings those together: validation, byte scan,
//                          one descriptor per pair
//   ltr_plan_schedule.cpp  class_stats, and build_schedule, which turns the description into the list of launches
//                          (ltr_plan_build.hip adds the grid query and the uploads, ltr_plan_run.hip walks the list);
//                          threshold_groups, pack_ranges
//   ltr_plan_hooks.cpp     the ltr_debug_* entry points tests/test_plan_units.py exercises all of this through, on the CPU
// A rule that more than one of them states -- or the execute path, or the C-ABI -- is an inline function here.
#ifndef LTR_PLAN_H_
#define LTR_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../include/ltr_gpu.h"
#include "ltr_dp_types.h"

namespace ltr { struct DebugKnobs; }
namespace ltrp {
// page-locked host memory for RawBuf (hipHostMalloc / hipHostFree behind them: ltr_ctx.hip); nullptr = none to be had
void* pinned_alloc(size_t bytes) __attribute__((visibility("hidden")));
void pinned_free(void* p) __attribute__((visibility("hidden")));
}

// Grow-only host array of trivially copyable elements that keeps its storage between uses and never
// initialises it: the per-plan work arrays (tens of MB: descriptors, costs, sort order) would otherwise be
// mapped, zero-filled page by page and unmapped again for every plan.
template <class T>
struct RawBuf {
  T* p = nullptr; size_t n = 0, cap = 0;
  // pinned: page-locked host memory (hipHostMalloc) -- for arrays the library uploads itself: a copy from pinned memory goes
  // over the DMA engines; from pageable memory it is staged by a copy KERNEL that waits for wave slots behind the persistent
  // DP launches of the previous chunk (measured on MI355X, ltr_calc_hap_aln_probs on the catalogue: the uploads of chunks
  // 1 and 2 took 1.1 - 1.6 ms against 0.3 - 0.4 ms for chunk 0, which finds the GPU idle).  Falls back to malloc.
  bool pinned = false, p_is_pinned = false;
  RawBuf() = default;
  RawBuf(const RawBuf&) = delete;
  RawBuf& operator=(const RawBuf&) = delete;
  ~RawBuf() __attribute__((visibility("hidden"))) { release(); }
  void release() { if (p) { if (p_is_pinned) ltrp::pinned_free(p); else std::free(p); } p = nullptr; cap = 0; n = 0; }
  // NOTE: the contents are UNDEFINED after a growth (resize is not std::vector's: every user rewrites the whole buffer).
  void resize(size_t m) {
    if (m > cap) {
      const size_t c = std::max(m + m / 4, (size_t)1024);
      // (the contents are never kept across a growth: the old block goes first, so that a context never holds both -- hundreds of
      // MB of pinned memory each on a 30 000-locus call; hipHostMallocPortable: usable from whichever device is current)
      release();
      T* q = nullptr;
      bool q_pinned = false;
      if (pinned) { q = (T*)ltrp::pinned_alloc(c * sizeof(T)); q_pinned = (q != nullptr); }
      if (!q) q = (T*)std::malloc(c * sizeof(T));
      if (!q) throw std::bad_alloc();
      p = q; cap = c; p_is_pinned = q_pinned;
    }
    n = m;
  }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T* data() { return p; }
  T* begin() { return p; }
  T* end() { return p + n; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

namespace ltrp {

// Launch classes ("bins") of the certificate kernels, in this order:
//   [0, kNumBins)             one pair per wavefront, strip width W = k+1 (any read length: column blocks through scratch strips)
//   [kPackFirst, +kNumPack)   64 / LP pairs per wavefront, LP = 2 << (j / kPackWMax) lanes per pair, W = j % kPackWMax + 1
//   [kWg4First, +kNumWg4)     one pair per 4-wave workgroup, W = kWg4MinW+j (reads of 1282 .. 5121 bases), LDS hand-off
//   [kWg8First, +kNumWg8)     one pair per 8-wave workgroup, W = kWg8MinW+j (reads of 5122 .. 10241 bases)
//   [kWg1First, +kNumWg1)     one pair per 1-wave workgroup, W = j+1: the latency variant for small batches
//   kFamClass                 members of haplotype families (ltr_dp_family.hpp): a launch of its own, the rows a read's haplotypes share scored once
// then the exact (redo) kernels, classes kNumFast + kXGeneric .. kXWg8.
constexpr int kNumBins = kWMax;
constexpr int kNumPack = kNumPackLp * kPackWMax;
constexpr int kPackFirst = kNumBins;
constexpr int kNumWg1 = kWg1MaxW;
constexpr int kWg4First = kPackFirst + kNumPack;
constexpr int kWg8First = kWg4First + kNumWg4;
constexpr int kWg1First = kWg8First + kNumWg8;
constexpr int kFamClass = kWg1First + kNumWg1;
constexpr int kNumFast = kFamClass + 1;         // certificate kernel classes
constexpr int kNumKernels = kNumFast + kNumExact;
// control words of a plan: [0, kNumKernels + 1] work queues (the last two: the W = 20 exact launch, the eight-wave list's narrow launch), [kRedoCountSlot, +kNumExact) exact list lengths
constexpr int kCtrlWords = 256;
constexpr int kStartQueueSlot = 176;           // [kStartQueueSlot, +kNumExact): work counters of the plan kernel's entries of kind 2 (the pairs that start out in an exact list)
constexpr int kRedoCountSlot = 192;
static_assert(kNumKernels + 2 <= kStartQueueSlot && kStartQueueSlot + kNumExact <= kRedoCountSlot, "control block layout");
static_assert(kNumKernels + 1 <= kRedoCountSlot && kRedoCountSlot + kInlineCountOff + kNumExact <= kCtrlWords && kInlineCountOff >= kNumExact, "control block layout");
static_assert(kWgStatOff >= kInlineCountOff + kNumExact && kRedoCountSlot + kWgStatOff + 2 <= kCtrlWords, "control block layout");

// pairs per block of the host loops over a plan's pairs (counting sort, gather, class statistics): a 10 000-locus chunk of a
// catalogue is 235 k pairs -- four blocks of 64 k kept four of the host's cores busy
constexpr size_t kPlanBlock = 16384;
constexpr int kWg4WideMinW = 15;               // (ltr_plan_rules.cpp, make_rules)
constexpr int kFoldRounds = 6;                 // automatic mode: classes below 6 x 4 x (pairs per wave) x CUs pairs are folded (tests/manual/gpu_fold_sweep.py)
enum { kFamOne = 0, kFamPack = 1, kFamWg = 2, kFamExact = 3, kFamShare = 4 };   // (kFamShare: kFamClass; the C-ABI lists it with the workgroup family -- a launch beside the plan kernel)
struct ClassInfo { int family; int W; int waves; int lp_shift; };   // waves per pair (workgroup kernels); lanes per pair = 1 << lp_shift (pack)
inline ClassInfo class_info(int k) {
  if (k < kPackFirst) return {kFamOne, k + 1, 1, 6};
  if (k < kWg4First) { const int j = k - kPackFirst; return {kFamPack, j % kPackWMax + 1, 1, kPackMinShift + j / kPackWMax}; }
  if (k < kWg8First) return {kFamWg, k - kWg4First + kWg4MinW, 4, 6};
  if (k < kWg1First) return {kFamWg, k - kWg8First + kWg8MinW, 8, 6};
  if (k == kFamClass) return {kFamShare, 0, 1, 6};              // (strip width per family: the read's)
  return {kFamWg, k - kWg1First + 1, 1, 6};
}
inline int pack_class(int lp_shift, int W) { return kPackFirst + (lp_shift - kPackMinShift) * kPackWMax + (W - 1); }

// W = ceil(C / (64 * ncb)), ncb = ceil(C / (64 * kWMax)): the narrowest strip that covers the read in the
// fewest column blocks of one wavefront (ltr_dp_kernel.hpp).
inline int strip_width_for(int m, int* ncb_out) {
  const int C = m - 1 > 1 ? m - 1 : 1;
  const int ncb = (C + 64 * kWMax - 1) / (64 * kWMax);
  if (ncb_out) *ncb_out = ncb;
  return (C + 64 * ncb - 1) / (64 * ncb);
}

constexpr int kLengthBuckets = 96;
inline int length_bucket(int C) {               // quarter octaves of the read's columns: 4 * floor(log2 C) + the next two bits
  if (C < 4) return C < 1 ? 0 : C;
  int e = 31 - __builtin_clz((unsigned)C);
  const int b = 4 * e + ((C >> (e - 2)) & 3);
  return b < kLengthBuckets ? b : kLengthBuckets - 1;
}

// ---- rules with more than one user ----------------------------------------------------------------------------------------
// The seven transitions of a parameter set (the emission constants stay 0: no class rule reads them; ltr_ctx.hip adds them).
inline ModelConsts model_consts_from(const ltr_align_params& p) {
  ModelConsts mc;
  mc.a = p.log_ins_to_ins; mc.b = p.log_ins_to_match; mc.c = p.log_del_to_del; mc.d = p.log_del_to_match;
  mc.e = p.log_match_to_match; mc.f = p.log_match_to_ins; mc.g = p.log_match_to_del;
  mc.match = mc.mismatch = mc.match_plus_f = 0.f;
  return mc;
}
// symmetric indel model (ins->match == del->match, match->ins == match->del): the 11-operation cell, every kernel but the generic ones
inline bool symmetric_model(const ModelConsts& mc) { return (mc.b == mc.d) && (mc.f == mc.g); }
// Band-penalty bound: the first |k| from which the band penalty (float)|k| * c alone is below -600, in float as the kernels form
// it (ltr_dp_kernel.hpp, ltr_dp_wg.hpp); kNoK600 where c is too small for any.  The penalty table, the threshold table and the
// length-sorted exact lists (Rules::xlut, Rules::thr_lists, KernelArgs::xlut, KernelArgs::thr_ok) need it within kPenKMax.
constexpr int kNoK600 = 0x3fffffff;
inline int band_k600(float c) { const float cabs = std::fabs(c); return (cabs * 1.0e9f > 600.0f) ? (int)(600.0f / cabs) + 2 : kNoK600; }
inline bool band_in_table(float c) { return band_k600(c) <= kPenKMax; }
// per-step overhead of a strip, in cells: steps x (cells of a step + this) is the modelled cost of a pair (classify_pair, form_families)
constexpr double kStepOverhead = 1.5;
// launch-order key of a modelled cost: steps of 1/16 octave (4.4 %), 1 .. 511 (a pair that is scored always has a key >= 1 -- key 0
// marks the constant-score pairs -- however small its cost)
inline int16_t launch_key(double cost) { return (int16_t)std::min(511, std::max(1, (cost > 1.0 ? (int)(std::log2(cost) * 16.0) : 0) - 16)); }
// strip width of every exact list's kernel (0: the workgroup exact kernels pick the width per pair)
constexpr int kXW[kNumExact] = {kExactW, kXShortW, kXMidW, kXLongW, 0, 0};

// What a batch as a whole decides (ltr_ctx_set_pair_packing mode, size of the batch, the indel model).
struct Rules {
  int mode = -1;               // ltr_ctx_set_pair_packing
  bool sym_model = true;       // ins->match == del->match and match->ins == match->del
  bool xlut = true;            // LUT / penalty-table exact kernels usable
  bool thr_lists = true;       // pairs are listed by read length for the threshold bodies: xlut, or -- any model -- under the plan kernel, whose exact bodies are calls of its own
  bool wg_long = false;        // workgroup kernels for reads longer than one wavefront's widest strips
  bool wg_wide4 = false;       // ... four-wave workgroups with strips of kWg4WideMinW columns and more: at any number of long pairs
  int64_t wide4_quota = INT64_MAX;   // ... for this many pairs of the batch; the rest of them on eight waves (ltr_plan_create moves them)
  bool wg_short = false;       // ... and their one-wave variant for every short read (mode 2)
  int wg_min_c = 64 * kWMax;
  int pack_min_shift = 7;      // fewest lanes per pair a packed class may use (7: no packed classes at all)
  int pack_force_shift = 0;    // != 0: this many lanes per pair whenever the read fits (modes 1, 5 .. 8)
  // fewest lanes per pair by read length (quarter-octave buckets of the read's columns, length_bucket()) -- only on request
  // (ltr_ctx_set_debug "pack_rule" = 3) since a packed launch is a whole strip width: pairs of a length that is rare in the
  // batch kept more lanes each, so that the launch of their (lanes, width) class still put about two wavefronts on every SIMD
  int8_t bucket_min_shift[kLengthBuckets];
  int flank = 5;               // indel_flank_len
  // |n - m| from which a pair goes straight to its exact list: a pair whose lengths differ by L carries a gap of at least L, and
  // once that gap alone costs ~520 the one-cell-per-lane certificate cannot hold the -600 line (measured on MI355X, a 1250-locus
  // shard of config 3: every one of the 119 pairs whose certificate failed had 531 <= |n - m| <= 600) -- scoring it with the
  // certificate body first is wasted work, and inside the plan kernel its exact body started late is the launch's tail
  int risky_dd_pos = 0x7fffffff, risky_dd_neg = 0x7fffffff;   // n - m / m - n from which a pair goes straight to the exact body (make_rules)
  // The plan kernel (ltr_dp_plan.hpp) scores the one-wave and packed classes of this batch in one persistent launch: automatic
  // mode, symmetric model.  Such a launch holds every wave slot until it ends, so launches beside it starve: once the batch can
  // fill the GPU, reads of up to two column blocks (2560 columns) stay with the one-wave classes (wg_min_c).
  bool plan_kernel = false;
};
// pairs_by_bucket: pairs of the batch by length_bucket(read columns), or nullptr (no per-length rule)
Rules make_rules(const ModelConsts& mc, int indel_flank_len, int mode, int n_cu, int64_t pairs_upper, int64_t n_long_pairs,
                 const int64_t* pairs_by_bucket = nullptr, int pack_rule = 0, int plan_knob = 0);

// Modelled cost of one pair in a packed class, in wave-cycles per pair: steps x (cells + per-step overhead)
// x the share of the wave the pair holds.  (Constants from the sweep of tests/manual/gpu_pack_sweep.py.)
double pack_cost(int n, int C, int lp_shift, int* W_out);

struct PairClass {
  int16_t cls = -1;            // launch class, or kNumFast + exact list for pairs that start out in an exact list
  double cost = 1.0;           // modelled launch time of the pair (wave-cycles; what the key is the logarithm of)
  int16_t key = 0;             // launch-order key: the cost in steps of 1/16 octave (4.4 %), 1 .. 511; shortcut pairs 0 (last)
  int8_t xc = kXGeneric;       // exact list the pair lands in if its certificate fails
  bool shortcut = false;       // HapAligner.cpp:241-244, :249-252: constant score, no DP
  bool x_candidate = false;    // counts towards the size of exact list xc
  bool uses_wg = false;
};
// n: window length (0 when hap_full_len <= 60), m: read length, generic: bytes outside ACGT
PairClass classify_pair(const Rules& R, int64_t n, int64_t m, int64_t hap_full_len, bool generic);

// Counting sort of the pairs by class (input order kept), every class then longest first by key.  In automatic mode
// a class whose pairs cannot fill the GPU's wave slots a few times over is folded into the next wider class of its
// family.  Out: order[i] = index of the pair that goes to sorted position i; bin_first[k] .. bin_first[k+1] = class k.
// fold_rounds: a class is folded while it holds fewer pairs than this many rounds of resident wavefronts (0: never)
// multi_launch: 1 = the one-wave widths kMultiMinW.. and the packed widths kPackMultiMinW.. share a launch each (nothing is
// folded there: every pair keeps its own strip width, and the last width below folds at most up to the first of them);
// 2 = the plan kernel takes every one-wave and packed class: nothing of the two families is folded
void sort_by_class(const int16_t* bin, const int16_t* key, int64_t n_pairs, int fold_rounds, int n_cu, int32_t* order,
                   int* bin_first /* [kNumKernels + 1] */, int* counts /* [kNumKernels] */, int multi_launch = 0);

// ---- the host half of ltr_plan_create ------------------------------------------------------------------------------------
// The context's work arrays a description is built in (a view: the context keeps the storage from plan to plan).
struct BatchScratch {
  RawBuf<PairDesc>& pairs; RawBuf<PairDesc>& sorted; RawBuf<int16_t>& key; RawBuf<int16_t>& bin; RawBuf<int32_t>& order;
  RawBuf<uint8_t>& read_acgt; RawBuf<uint8_t>& hap_acgt;
};
// What the host alone keeps of a spine: the family's modelled steps as it is run (the launch-order key) and every member's own fork
// row max(p, min(lcp(spine, member), n - 1)) (the spine member's: its n; a plain family's: unused).
struct FamilyForks { int64_t steps; int16_t fork[kFamilyMaxMembers]; };
// What describe_batch decides about a batch; a plan (struct ltr_plan, ltr_ctx.h) starts out as one of these.
struct __attribute__((visibility("hidden"))) BatchPlan {
  int64_t n_pairs = 0, ll_size = 0;
  double cells = 0.0, input_bytes = 0.0;
  int32_t max_len = 0;
  int bin_first[kNumKernels + 1] = {0};    // classes kNumFast + c: pairs that start out in exact list c (non-ACGT pairs; mode 4: all)
  int counts[kNumKernels] = {0};           // pairs per class after folding
  int x_seed[kNumExact] = {0};          // pairs pre-seeded into every exact list (sorted array ranges bin_first[kNumFast + c] ..)
  int64_t xcand[kNumExact] = {0};          // pairs that could end up in each exact kernel's list
  int64_t xstart[kNumExact] = {0};         // (plan kernel: the pairs that start out in a list, counted apart -- the plan kernel scores them itself)
  std::vector<int32_t> seed;            // host: read length - 1 (or -1 when the read is masked out)
  std::vector<int32_t> locus_P, locus_H;   // per locus: pools, haplotypes
  std::vector<int64_t> locus_ll_off;       // per locus: offset of its [P x H] block
  bool sym_at_create = true;            // indel model was symmetric when the pairs were binned
  bool xlut = false;                    // LUT / penalty-table exact kernels usable (symmetric model, k600 <= kPenKMax)
  bool uses_wg = false;                 // some pairs sit in workgroup-kernel classes (symmetric models only)
  bool use_plan = false;                // the plan kernel (ltr_dp_plan.hpp) scores the one-wave and packed classes
  bool use_multi = false;               // ... or the multi-width launches do
  // haplotype families (form_families), in the order of their members in the sorted pair list: by modelled cost, largest first
  std::vector<FamilyDesc> fams;
  std::vector<double> fam_U;            // per family: the acceptance bound the host filtered its members with (the device forms its own)
  int64_t fam_members = 0;
  std::vector<FamilySpine> fam_spines;  // per family: its spine and park rows (spine -1: plain)
  std::vector<FamilyForks> fam_forks;   // ... its steps and fork rows, kept only on request (ltr_debug_plan_family_forks)
  bool keep_forks = false;
  int64_t fam_with_spine = 0, fam_rows_saved = 0;   // families run along a spine; modelled steps they save against plain families
};
constexpr int kFamPerCu = 12;           // by rule a batch forms families from this many per CU up: one for every wavefront of the family launch's full grid (form_families)
constexpr int kSpinePerCu = 24;         // by rule a plan runs its families along spines from this many families per CU up (form_families)
constexpr int kFamMinRows = 64;         // fewest shared rows a family is formed for (ltr_ctx_set_debug "family_min_rows")
// Haplotype families (ltr_dp_family.hpp).  A family is the pairs of one pooled read against two or more haplotypes of its locus whose
// windows share their first rows; its fork row p = min(longest common prefix of the members' WINDOWS, smallest n - 1), so that every
// tail has a row.  A pair is a member only as a one-wave pair of ONE column block (641 .. 1280 read columns) that the class rule
// left in the one-wave class of its own strip width -- no constant score, pure ACGT, not on a risky_dd list -- under the plan kernel
// and a symmetric model, and only if its score has a chance against the bound U of the fork: the gap its length difference forces,
// open + (|n - m| - 1) x extend in exact doubles, must be > U = ((g + lpc[p-1]) + d) + MATCH, or the device's acceptance rule is
// certain to send it to the exact body.  A family is formed when p >= min_rows and its modelled steps, (p-1 + L-1) + sum(n_h - p +
// L-1), are fewer than the members' own, sum(n_h - 1 + L-1) (L lanes; both x the same strip cost), and when the batch holds at least
// kFamPerCu families per CU (below that the plan kernel, which spreads the pairs over idle wave slots, is faster: measured); knob 1: whenever p allows.
// Members move to kFamClass with ONE launch-order key per family (its modelled cost): the class sort keeps the input order inside
// a key, so a family's members stay side by side, and lists the families largest first.
// The NARROW band is the same family on the same geometry -- strips of W = ceil(C / 64) = 6 .. 10 on ceil(C / W) <= 64 lanes of one
// wavefront -- for reads of 321 .. 640 columns (what is said above describes the WIDE band, 641 .. 1280).  By rule its members are the pairs the
// class rule put into the packed class of 32 lanes (a batch too small to pack forms none), and since a packed pair holds half a
// wavefront of strips of Wp = ceil(C / 32) columns the cost rule compares modelled work, not steps: fam_steps x (W + 1.5) against
// sum((n_h - 1) + (Lp - 1)) x (Wp + 1.5) x 32/64, Lp = ceil(C / Wp).  The count rule: narrow families are formed only when they alone number
// kFamPerCu per CU (a smaller plan keeps the launches it had); then both bands together are held against the same count, as before.  Knob 1 forms no
// narrow family; knob 2 is "on request" in both bands: no cost rule, no count rule, and narrow candidates also from the one-wave
// class of their strip width (where a batch that does not pack leaves them).
// The SPINE (choose_spine; FamilySpine, ltr_dp_types.h) is chosen after forming and changes none of it -- p, U, count, W, dd_min, dd_max and
// which families exist stay what they were; it only removes steps, so a family that pays keeps paying.  For a formed family the member s
// that minimises (n_s - p) + sum over the others of (n_k - f_k), f_k = max(p, min(lcp(s, k), n_k - 1)), is the spine (the first such
// member in haplotype order), at most kFamilyParkSlots - 1 of the distinct f_k beyond p are kept as park rows -- the subset that saves
// most rows --, and a member whose own row is not kept starts from the nearest kept row below it.  A family in which no member forks
// beyond p stays plain (spine -1).  The launch-order key is the modelled steps of the family AS RUN, (n_s - 1 + L-1) + sum(n_k - row_k + L-1),
// so that the static deal balances the real work.  By rule only plans of at least kSpinePerCu families per CU (6144 on 256 CUs) use spines: a
// smaller plan keeps plain families, the keys and the launch it had (why).  ltr_ctx_set_debug "family_spine": -1 never, 0 by
// rule, 1 in any plan.
struct FamilyRec {
  int64_t first_pair; FamilyDesc f; double U;        // (first_pair: in batch order, before the sort)
  int64_t row_at; uint64_t members; int16_t key;     // the read's first pair in batch order, its member pairs from there as bits, their launch-order key
  int16_t plain_key;                                 // ... and the key of the family run as a plain one
  int32_t steps, plain_steps;                        // modelled steps as it is run / as a plain family (the cost rule's)
  int32_t locus, spine_at;                           // its spine: FamilySide::sp[locus][spine_at] (spine_at -1: plain)
};
// The spines of the families of a batch (choose_spine), locus by locus beside the family list: written once where they are chosen, read
// once where the sorted list is resolved.  fork: kFamilyMaxMembers fork rows per spine (FamilyForks::fork), kept on request only.
struct FamilySide {
  bool keep_forks = false;
  std::vector<std::vector<FamilySpine>> sp;
  std::vector<std::vector<int16_t>> fork;
};
// spine_knob: ltr_ctx_set_debug "family_spine" (-1 never: every family plain; 0 by rule: a spine wherever a member forks beyond p, in
// plans of at least kSpinePerCu families per CU; 1: in any plan)
void form_families(const ltr_locus_batch* b, const ModelConsts& mc, int F, int n_cu, int knob, int min_rows, int spine_knob, const std::vector<int64_t>& pair_base,
                   const BatchScratch& w, std::vector<FamilyRec>* out, FamilySide* side) __attribute__((visibility("hidden")));
// Validates the batch, gives every pair its descriptor, class and key, sorts them (w.sorted, w.order, w.key stay valid for the
// caller) and fills *d.  mode: ltr_ctx_set_pair_packing.  LTR_OK, or LTR_ERR_INVALID with the reason in *err.
int describe_batch(const ltr_locus_batch* b, const ModelConsts& mc, int indel_flank_len, int mode, int n_cu, const ltr::DebugKnobs& dbg,
                   const BatchScratch& w, BatchPlan* d, std::string* err) __attribute__((visibility("hidden")));

// Nominal cells and longest read (columns, m - 1) of every certificate class, nominal cells of the pairs that start out in every
// exact list: one pass over the sorted pairs (w.sorted, w.order, w.key as describe_batch left them).
struct ClassStats { double bin_cells[kNumFast] = {0}; int32_t cls_cmax[kNumFast] = {0}; double x_cells[kNumExact] = {0}; };
void class_stats(const BatchPlan& d, const BatchScratch& w, ClassStats* st) __attribute__((visibility("hidden")));

// ---- the launch schedule of a plan ------------------------------------------------------------------------------------------
// One first-pass launch.  Launches that take several classes -- a packed launch takes every lanes-per-pair class of its strip
// width; the multi-width launches and the plan kernel take whole families -- use the queue word, the statistics slot and the
// pair range of ONE of their classes, cls: the widest that has pairs.
enum LaunchKind { kLaunchOne = 0, kLaunchPack, kLaunchMulti, kLaunchPackMulti, kLaunchPlan, kLaunchWg, kLaunchFamily };
struct Launch {
  int kind = kLaunchOne;
  int cls = 0;                 // the class it is launched, timed and reported under
  int W = 0;                   // strip width (kLaunchOne, kLaunchPack, kLaunchWg)
  int grid = 1;                // persistent grid
  bool small = false;          // cannot fill the GPU's wave slots once
  int32_t cmax = 0;            // longest read (columns) of any member: the launch order, and when the exact lists close
  int64_t pairs = 0;
  double cells = 0.0;          // nominal
  // member classes, widest first: n_one one-wave classes, then n_pack packed widths as the widest lanes-per-pair class of each
  // that has pairs (what a single-width packed launch is listed under)
  int n_one = 0, n_pack = 0;
  int16_t members[kNumBins + kPackWMax] = {0};
};
// Resident workgroups (occupancy x CUs) of every launch the schedule sizes: the context asks the runtime once.
struct OccupancyGrids { int cls[kNumFast] = {0}; int multi = 0, pack_multi = 0, plan = 0; int exact[kNumExact] = {0}; };
struct __attribute__((visibility("hidden"))) Schedule {
  std::vector<Launch> launches;          // in launch order: longest cmax first, ties in descending class order
  std::vector<Launch> by_class;          // ... with the multi-width launches class by class again (ltr_plan_set_timing level 2)
  std::vector<PlanEntry> plan_entries;   // the plan kernel's table in walk order, with the wavefronts' starting shares
  std::vector<PackTable> pack_tabs;      // range tables of the packed widths of a kLaunchPackMulti / kLaunchPlan launch, widest first
  int x_grid[kNumExact] = {0};           // launch grid of every exact kernel; 0 = no pair of this plan can land in its list
  int max_grid = 1;                      // largest grid of a launch that parks column blocks in scratch strips
  int max_grid_wide = 1;                 // grid of the W = 20 exact launch (candidates of the 4-wave list)
  const Launch* plan_launch() const { for (const Launch& L : launches) if (L.kind == kLaunchPlan) return &L; return nullptr; }
  // the launches at a timing level (the plan kernel is never split: its classes score their failed certificates in line, and
  // no exact launch is sized for what a single-class kernel would queue)
  const std::vector<Launch>& at_level(int level) const { return (level >= 2 && !plan_launch()) ? by_class : launches; }
  // position in such a list of the launch that is listed under class k, or -1 (no pairs; a member of another class's launch)
  static int find(const std::vector<Launch>& list, int k);
  // (lanes per pair, strip width, pairs) of every class a launch over several classes takes, in launch order; 0 for the others
  int ranges(const Launch& L, const int* bin_first, int32_t* lanes_per_pair, int32_t* strip_width, int64_t* n_pairs) const;
  // scratch strips are finite: no launch that uses them (one-wave bodies) gets more than cap workgroups
  void cap_grids(int cap);
  // ltr_ctx_set_debug "grid_cap" (tests): NO launch gets more than cap workgroups -- the packed and workgroup launches, the
  // four- and eight-wave exact lists and the W = 20 exact launch too; every kernel is persistent, so only the items a wavefront
  // takes one after the other change
  void cap_every_grid(int cap);
};
// One kernel launch as it was made (ltr_debug_last_launches): kind = LaunchKind of a first-pass launch, or one of the kinds below;
// cls = launch class (exact list; class of ltr_haplotype_align_to_ref); takers = wavefronts (one-wave bodies) or workgroups
// (workgroup kernels: 1) per workgroup that take items independently of each other; items = pairs / families / tasks the launch
// was given, -1 where only the device knows (the exact lists)
enum { kNoteThreshold = 7, kNoteExact = 8, kNoteExactWide = 9, kNoteExactNarrow8 = 10, kNoteNwWave = 11, kNoteNwWg = 12 };
struct LaunchNote { int32_t kind, cls, grid, takers; int64_t items; };
// The schedule of a described batch.  Pure: class ranges and statistics, occupancy grids and A/B knobs (chain*, plan_share) in.
// Settles in *d what depends on it: without anything for the plan kernel to score use_plan falls back and the exact launches
// take the list starters (xcand); with it the plan kernel scores them itself (x_seed = 0).
void build_schedule(BatchPlan* d, const ClassStats& st, const OccupancyGrids& occ, const ltr::DebugKnobs& dbg, Schedule* out) __attribute__((visibility("hidden")));

// ---- pure pieces of ltr_plan_execute --------------------------------------------------------------------------------------
// Threshold first pass of the workgroup classes: which kernel scores a class (nw waves, strips of w columns; nw 0 = not a
// workgroup class with pairs) and how many pairs the launch it leads takes (np 0: led by a class before it).
// strip width of the threshold kernel that takes strips of W columns: W rounded up to even (the launchers of ltr_k_wgt.hip round
// whatever they are given the same way, ltrk::wgt_width: a width from here is a fixed point of theirs)
inline int threshold_strip_width(int W) { return W + (W & 1); }
struct ThresholdGroups { int nw[kNumFast] = {0}, w[kNumFast] = {0}, np[kNumFast] = {0}; };
// merge: neighbouring narrow eight-wave classes share a launch (not under per-launch timing); keep_waves: ltr_ctx_set_debug "wgt_keep_waves"
ThresholdGroups threshold_groups(const int* bin_first, bool merge, bool keep_waves) __attribute__((visibility("hidden")));
// The ranges of the packed launch of strip width W, widest segments first (their groups last longest): five entries each.
void pack_ranges(const int* bin_first, int W, int32_t* shift, int32_t* first, int32_t* end, int32_t* grp_end) __attribute__((visibility("hidden")));

// The exact kernels' row test (ltr_dp_kernel.hpp, column_block): the reference aborts a pair when a row's maximum of
// fl(best + pen(k)), pen(k) = (double)((float)|k| * c), is below -600 (HapAligner.cpp:297-306).  x -> fl(x + p) is monotone, so
// "some cell reaches -600" is "some cell has best >= thr(k)" with thr(k) the SMALLEST double that does.  Entry k + kPenHalf of
// out[kPenTabDoubles]; +inf where no (negative) cell value can pass: |k| >= k600, |k| > kPenKMax, thr(k) >= 0.
void build_threshold_table(float c, double* out);

}  // namespace ltrp

// Test hooks of the two units above (tests/test_plan_units.py; the other ltr_debug_* hooks are declared in include/ltr_gpu.h).
// ltr_debug_describe_batch: ltrp::describe_batch on arrays of its own; out_i64[0..2] = pairs, LL size, longest sequence,
// out_f64[0..1] = cells, input bytes, class_first[ltr_debug_num_classes() + 1], per sorted pair its descriptor fields
// (n, m, out_idx) and key; the reason of an LTR_ERR_INVALID goes to err[err_cap].
// ltr_debug_threshold_groups: ltrp::threshold_groups; nw / w / np hold ltr_debug_num_classes() entries each.
// ltr_debug_plan_schedule: describe_batch, class_stats and build_schedule.  grids[ltr_debug_num_classes() + 3]: the occupancy grid of
// every certificate class, of the exact kernels, then of the multi-width one-wave launch, the multi-width packed launch and the plan
// kernel.  knobs[7] = plan_kernel, no_multi, chain, chain_min_w, chain_max_w, plan_share, grid cap (0: none; n > 0: the strips' cap,
// Schedule::cap_grids; -n: ltr_ctx_set_debug "grid_cap" = n, Schedule::cap_every_grid).  Per launch 8 words
// in launch[launch_cap][8] = kind, class, strip width, grid, small, cmax, pairs, members and its cells in launch_cells[]; the
// members of all launches one after the other in members[member_cap]; per entry 6 words in entry[entry_cap][6] = kind, strip
// width, first pair, pairs, queue class, first_wave.  out[8 + kNumExact] = launches, level-2 launches (listed behind the first),
// entries, pack tables, use_plan, max_grid, max_grid_wide, max_len, then xcand[kNumExact], then class_first[ltr_debug_num_classes() + 1];
// x_grid[kNumExact].
extern "C" {
int ltr_debug_plan_schedule(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* grids, const int32_t* knobs,
                            int64_t* out, int32_t* x_grid, int launch_cap, int32_t* launch, double* launch_cells, int member_cap, int32_t* members,
                            int entry_cap, int32_t* entry);
int ltr_debug_describe_batch(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, int64_t* out_i64, double* out_f64,
                             int32_t* class_first, int64_t pair_cap, int32_t* pair_n, int32_t* pair_m, int64_t* pair_out_idx, int16_t* pair_key,
                             char* err, int err_cap);
int ltr_debug_threshold_groups(const int32_t* class_first, int merge, int keep_waves, int32_t* nw, int32_t* w, int32_t* np);
// ltr_debug_plan_families: describe_batch with knobs[2] = families (-1 never, 0 by rule, 1 whenever one can be formed in the wide band, 2 ... in both bands), family_min_rows
// (0: the rule's).  out[4] = families, members, first sorted pair of the family class, pairs of the batch; per family 6 words in
// fam[fam_cap][6] = first member (sorted pair), members, p, strip width, dd_min, dd_max, and its bound in U[]; per sorted pair of the
// family class (from out[2] on) its window length in member_n[member_cap] and its LL index in member_out[].
int ltr_debug_plan_families(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* knobs, int64_t* out,
                            int fam_cap, int32_t* fam, double* U, int member_cap, int32_t* member_n, int64_t* member_out);
// ltr_debug_plan_family_forks: the same call with knobs[3] = families, family_min_rows, family_spine, for the spines (choose_spine).  out[4] =
// families, members, families with a spine, modelled steps saved; per family (in the order of its members in the sorted pair list) 10
// words in fam[fam_cap][10] = spine member (-1: plain), slots, modelled steps, park-slot capacity, then first member, members, p, strip
// width, dd_min, dd_max as ltr_debug_plan_families lists them, and slot_row[fam_cap][capacity]; per sorted pair of the family class its
// fork row in member_fork[member_cap] (the spine member's: its n; plain: p), its slot in member_slot[] and its LL index in member_out[].
int ltr_debug_plan_family_forks(const ltr_align_params* p, int mode, int n_cu, const ltr_locus_batch* b, const int32_t* knobs, int64_t* out,
                                int fam_cap, int32_t* fam, int32_t* slot_row, int member_cap, int32_t* member_fork, int32_t* member_slot, int64_t* member_out);
// ltr_debug_last_launches (ltr_plan_run.hip; needs a device): the kernel launches of the last ltr_plan_execute of `plan`, or (plan
// NULL) of the last ltr_haplotype_align_to_ref of `ctx`, in the order made and as made -- recorded at the launch, the grids formed at
// execute time included.  Per launch 5 words in out[cap][5] = kind (ltrp::LaunchKind, kNote*), class, grid, takers per workgroup,
// items (-1: on the device); returns the number of launches (which may exceed cap) or LTR_ERR_INVALID.
struct ltr_plan; struct ltr_ctx;
int ltr_debug_last_launches(const ltr_plan* plan, ltr_ctx* ctx, int cap, int64_t* out);
// ltr_debug_family_wave_clocks (ltr_plan_run.hip; needs a device): a measurement aid beside ltr_plan_debug_wave_clocks (include/ltr_gpu.h).
// With ltr_ctx_set_debug(ctx, "wave_clock", 1) set when the plan was created, the family launch (ltr_dp_family.hpp) records the wall
// clock (100 MHz, the plan kernel's clock) at which every one of ITS wavefronts started and left, in a buffer of its own: out = {first,
// last} per wavefront of the last execute -- how far apart the wavefronts of the static deal finish and, set against the plan kernel's
// first clocks, whether the launch behind it starts before the family launch's last wavefront ends.  cap (64-bit words) must hold 2 x
// wavefronts.  Returns the number of wavefronts written (0: not recorded, or a plan without a family launch), negative on error.
int ltr_debug_family_wave_clocks(ltr_plan* plan, uint64_t* out, int64_t cap);
}

#endif
