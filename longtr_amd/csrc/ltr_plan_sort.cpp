// ltr_plan_sort.cpp -- the class sort (ltr_plan.h): the pairs class by class, every class longest first; in automatic mode
// the under-filled classes of a family folded into their wider neighbours first.

#include <cstring>

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace ltrp {

// One family of classes as the fold walk sees it: a POSITION is a strip width, its classes -- one per row, class first[r] + (w - w_lo)
// -- move together, each into the class of the next width, and its fill is what it launches: groups of per[r] pairs (wavefronts of
// a one-wave or packed width, workgroups).
struct FoldFamily {
  int w_lo, w_stop, w_max;     // widths folded FROM: [w_lo, w_stop); the family's widest
  bool small_ok;               // widths <= 4 fold whatever the ratio
  int64_t min_fill;            // a width with less than this folds
  int n_rows, first[kNumPackLp], per[kNumPackLp];
};

// A width that cannot fill the GPU's wave slots folds into the next one while the widest strip of the running group stays within a
// third of its narrowest, lo_w (or <= 4: small_ok) -- and only towards a width that has pairs of its own: a lone small class keeps
// its strip width.  remap[k]: where class k's pairs go (one step; the caller resolves chains).  True if anything moved.
static bool fold_walk(const FoldFamily& f, int* counts, int* remap) {
  auto fill = [&](int w) {
    int64_t v = 0;
    for (int r = 0; r < f.n_rows; ++r) v += (counts[f.first[r] + (w - f.w_lo)] + f.per[r] - 1) / f.per[r];
    return v;
  };
  bool any = false;
  int lo_w = 0;                                                               // narrowest strip folded into the running group
  for (int w = f.w_lo; w < f.w_stop; ++w) {
    const int64_t v = fill(w);
    if (v == 0) { lo_w = 0; continue; }
    if (lo_w == 0) lo_w = w;
    auto within = [&](int w2) { return (f.small_ok && w2 <= 4) || 3 * w2 <= 4 * lo_w; };
    bool target = false;                                                      // (none unless w + 1 itself is within the group)
    for (int w2 = w + 1; w2 <= f.w_max && within(w2); ++w2) if (fill(w2) > 0) { target = true; break; }
    if (v >= f.min_fill || !target) { lo_w = 0; continue; }
    for (int r = 0; r < f.n_rows; ++r) {
      const int k = f.first[r] + (w - f.w_lo);
      if (counts[k] == 0) continue;
      counts[k + 1] += counts[k]; counts[k] = 0; remap[k] = k + 1; any = true;
    }
  }
  return any;
}

void sort_by_class(const int16_t* bin, const int16_t* key, int64_t n_pairs, int fold_rounds, int n_cu, int32_t* order,
                   int* bin_first, int* counts, int multi_launch) {
  // (counted and placed in blocks of kPlanBlock pairs on all host cores: block b's pairs of class k go behind those of
  // the blocks before it, which keeps the input order inside a class)
  const size_t np = (size_t)n_pairs;
  const int64_t n_blk = (int64_t)((np + kPlanBlock - 1) / kPlanBlock);
  std::vector<int32_t> blk_cnt((size_t)n_blk * kNumKernels, 0);
  ltr::parallel_for(n_blk, 1, [&](int64_t c) {
    int32_t* cn = blk_cnt.data() + (size_t)c * kNumKernels;
    for (size_t i = (size_t)c * kPlanBlock; i < std::min(np, ((size_t)c + 1) * kPlanBlock); ++i) cn[bin[i]]++;
  }, 1);
  for (int k = 0; k < kNumKernels; ++k) counts[k] = 0;
  for (int64_t c = 0; c < n_blk; ++c) for (int k = 0; k < kNumKernels; ++k) counts[k] += blk_cnt[(size_t)c * kNumKernels + k];
  int remap[kNumKernels];
  for (int k = 0; k < kNumKernels; ++k) remap[k] = k;
  // Small plans (the chunks of ltr_calc_hap_aln_probs, single loci): a class whose pairs cannot fill the GPU's
  // wave slots even once is folded into the next wider class of its family -- any strip width >= a pair's own
  // scores it with the same bits, only with idle slack columns -- as long as the widest strip of the group stays
  // within a third of its narrowest (or <= 4).  Measured on MI355X: a 600-locus chunk spent 9.7 ms in twenty
  // two-per-wave launches of 200-600 workgroups each, every one as long as its longest pair.  Automatic mode only:
  // the explicit packing modes keep one class per strip width.
  if (fold_rounds > 0) {
    const int64_t waves = (int64_t)fold_rounds * 4 * n_cu;                    // (4 SIMDs per CU; ~3-4 resident wavefronts each: fold_rounds = 3 is one full round)
    const int64_t wgs = (int64_t)fold_rounds * n_cu;                          // (two or three workgroups per CU: two to three rounds)
    // (the classes of strip widths kMultiMinW and up are one persistent launch when multi_launch is set, ltr_dp_multi_kernel:
    // a class of a few pairs costs nothing there, every pair keeps its own strip width; so are the packed widths kPackMultiMinW
    // and up, ltr_dp_pack_multi_kernel: nothing to fold there; multi_launch 2: nothing in either family)
    const int one_stop = multi_launch == 2 ? 0 : (multi_launch ? kMultiMinW : kNumBins);
    const int pack_stop = multi_launch == 2 ? 0 : (multi_launch ? kPackMultiMinW : kPackWMax);
    FoldFamily fams[4] = {
      {1, one_stop, kNumBins, true, waves, 1, {0}, {1}},                      // one-wave family
      // packed family: a launch is ONE strip width -- the pairs of every lanes-per-pair block of it (ltr_dp_pack.hpp) --
      // so what is folded is a whole width: every (LP, W) class of it into (LP, W + 1), while the wavefronts of the
      // width (groups of 64 / LP pairs) cannot fill the wave slots
      {1, pack_stop, kPackWMax, true, waves, kNumPackLp, {0}, {1}},
      // ... and the workgroup families: a class of a few hundred pairs next to another one leaves both launches with a
      // partly filled last round of workgroups (measured on MI355X: 1116 + 420 five-kb pairs as W = 17 and W = 18
      // four-wave classes 2.05e12 cells/s, the neighbouring single-class lengths 2.5 - 2.7e12)
      {kWg4MinW, kWg4MinW + kNumWg4 - 1, kWg4MinW + kNumWg4 - 1, false, wgs, 1, {kWg4First}, {1}},
      {kWg8MinW, kWg8MinW + kNumWg8 - 1, kWg8MinW + kNumWg8 - 1, false, wgs, 1, {kWg8First}, {1}}};
    for (int sft = kPackMinShift; sft <= kPackMaxShift; ++sft) { fams[1].first[sft - kPackMinShift] = pack_class(sft, 1); fams[1].per[sft - kPackMinShift] = 64 >> sft; }
    bool any = false;
    for (const FoldFamily& f : fams) any = fold_walk(f, counts, remap) || any;
    if (any)
      for (int k = kNumKernels - 2; k >= 0; --k) if (remap[k] != k) remap[k] = remap[remap[k]];     // (chains resolve wide to narrow)
  }
  bin_first[0] = 0;
  for (int k = 0; k < kNumKernels; ++k) bin_first[k + 1] = bin_first[k] + counts[k];
  {
    // where block c starts inside every (folded) class
    std::vector<int32_t> blk_at((size_t)n_blk * kNumKernels, 0);
    int fill[kNumKernels];
    for (int k = 0; k < kNumKernels; ++k) fill[k] = bin_first[k];
    for (int64_t c = 0; c < n_blk; ++c) {
      int32_t* at = blk_at.data() + (size_t)c * kNumKernels;
      for (int k = 0; k < kNumKernels; ++k) at[k] = -1;
      for (int k = 0; k < kNumKernels; ++k) {
        const int32_t n_k = blk_cnt[(size_t)c * kNumKernels + k];
        if (n_k == 0) continue;
        const int t = remap[k];
        if (at[t] < 0) at[t] = fill[t];
        fill[t] += n_k;
      }
    }
    ltr::parallel_for(n_blk, 1, [&](int64_t c) {
      int32_t at[kNumKernels];
      std::memcpy(at, blk_at.data() + (size_t)c * kNumKernels, sizeof(at));
      for (size_t i = (size_t)c * kPlanBlock; i < std::min(np, ((size_t)c + 1) * kPlanBlock); ++i) order[(size_t)at[remap[bin[i]]]++] = (int32_t)i;
    }, 1);
  }
  {
    // Every class longest first (by the 1/16-octave key).  A class is cut into segments of <= 32 k pairs: the
    // segments of all classes are counting-sorted side by side on the host cores, then merged pairwise, level by
    // level (a catalogue of short repeats puts half a million pairs into one class: 13.5 ms on one core before this).
    auto longer = [&](int32_t x, int32_t y) { return key[(size_t)x] > key[(size_t)y]; };
    struct Seg { int32_t a, b; };
    constexpr int32_t kSeg = 32768;
    std::vector<Seg> segs;
    std::vector<std::vector<int32_t>> cuts((size_t)kNumKernels);        // per class: segment boundaries
    for (int k = 0; k < kNumKernels; ++k) {
      const int32_t a = bin_first[k], b2 = bin_first[k + 1];
      if (b2 <= a) continue;
      const int32_t ns = (b2 - a + kSeg - 1) / kSeg;
      for (int32_t i = 0; i <= ns; ++i) cuts[(size_t)k].push_back(a + (int32_t)((int64_t)(b2 - a) * i / ns));
      for (int32_t i = 0; i < ns; ++i) segs.push_back({cuts[(size_t)k][(size_t)i], cuts[(size_t)k][(size_t)i + 1]});
    }
    ltr::parallel_for((int64_t)segs.size(), 1, [&](int64_t i) {
      // counting sort of the segment by key, longest first, input order kept inside a key
      int32_t* seg = order + segs[(size_t)i].a;
      const int32_t n_seg = segs[(size_t)i].b - segs[(size_t)i].a;
      if (n_seg < 64) { std::stable_sort(seg, seg + n_seg, longer); return; }
      int32_t at[513] = {0};
      for (int32_t k = 0; k < n_seg; ++k) at[512 - (int)key[(size_t)seg[k]]]++;           // slot 1 + (511 - key)
      for (int q = 1; q <= 512; ++q) at[q] += at[q - 1];
      std::vector<int32_t> tmp(seg, seg + n_seg);
      for (int32_t k = 0; k < n_seg; ++k) seg[at[511 - (int)key[(size_t)tmp[(size_t)k]]]++] = tmp[(size_t)k];
    }, 1);
    for (;;) {                                                          // merge levels: neighbours of every class, all classes at once
      struct Mrg { int32_t a, m, b; };
      std::vector<Mrg> work;
      for (int k = 0; k < kNumKernels; ++k) {
        std::vector<int32_t>& c = cuts[(size_t)k];
        if (c.size() <= 2) continue;
        std::vector<int32_t> next;
        size_t i = 0;
        for (; i + 2 < c.size(); i += 2) { work.push_back({c[i], c[i + 1], c[i + 2]}); next.push_back(c[i]); }
        for (; i < c.size(); ++i) next.push_back(c[i]);
        if (next.back() != c.back()) next.push_back(c.back());
        c.swap(next);
      }
      if (work.empty()) break;
      ltr::parallel_for((int64_t)work.size(), 1, [&](int64_t i) {
        std::inplace_merge(order + work[(size_t)i].a, order + work[(size_t)i].m, order + work[(size_t)i].b, longer);
      }, 1);
    }
  }
}

}  // namespace ltrp
