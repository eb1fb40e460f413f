// ltr_plan.cpp -- host-side planning units of a batch: launch-class rule, cost model, class sort (see ltr_plan.h).
// Pure host code: what it decides is WHICH kernel scores a pair and in what order -- never the score
// (every kernel returns the reference's bits, HapAligner.cpp:236-343).

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace ltrp {

Rules make_rules(const ModelConsts& mc, int indel_flank_len, int mode, int n_cu, int64_t pairs_upper, int64_t n_long_pairs,
                 const int64_t* pairs_by_bucket, int pack_rule, int plan_knob) {
  Rules R;
  R.mode = mode;
  R.flank = indel_flank_len;
  R.sym_model = (mc.b == mc.d) && (mc.f == mc.g);
  {
    const float cabs = std::fabs(mc.c);
    const int64_t k600 = (cabs * 1.0e9f > 600.0f) ? ((int64_t)(600.0f / cabs) + 2) : (int64_t)1 << 40;
    R.xlut = R.sym_model && k600 <= kPenKMax;
  }
  // Workgroup-per-pair kernels (ltr_dp_wg.hpp; symmetric indel models, ACGT pairs): for reads longer than one
  // wavefront's 1280 columns (64 lanes x the widest strip, W = 20) -- and only while the long pairs alone cannot fill
  // the GPU one wavefront each (fewer than ten per CU; measured on MI355X, 5-kb pairs, workgroup kernels against one
  // wavefront per pair with W = 20 strips: 1536 pairs 2.31e12 against 1.72e12 cells/s, 3008 pairs 2.30 against 2.40,
  // 9216 pairs 2.32 against 2.46).  Their one-wave variant (haplotype rows and first-column table through LDS) is only
  // taken on request (mode 2): a one-locus batch is bound by the instructions issued per step, not by memory latency
  // -- 0.151 ms per config-2 pass against 0.099 ms for the leaner one-wave kernel.
  // Round 3: four waves with WIDE strips (W = 15 .. 20: reads of 3586 .. 5121 bases, three workgroups a CU at three waves a
  // SIMD) against the eight-wave workgroups with their narrow strips (W = 8 .. 10, two a CU) and against column blocks on
  // one wavefront, measured on MI355X: 1536 pairs of 3.7 / 4.3 / 4.9 kb 2.51 / 2.53 / 2.70e12 cells/s against 1.95 / 2.12 /
  // 2.26e12 on eight waves; 9216 pairs of 4.9 kb 2.72e12 against 2.45e12 on one wavefront each.  A four-wave pair lasts
  // 1.26 x its eight-wave time on half the lanes, so what decides is how the pairs fill ROUNDS of 3 against 2 workgroups
  // per CU: 1868 such pairs (config5hifi) are 2.4 rounds of four-wave workgroups, 27.0 ms, or 3.6 of eight-wave ones,
  // 25.9 ms.  Taken when the rounds say so with a tenth to spare, up to 80 long pairs per CU.
  R.wg_long = R.sym_model && mode != 3 && (mode == 2 || n_long_pairs < (int64_t)10 * n_cu);
  {
    int64_t n_wide = n_long_pairs;                                        // pairs of 3585 .. 5120 columns (no histogram: every long pair)
    if (pairs_by_bucket) n_wide = pairs_by_bucket[length_bucket(4 * 64 * (kWg4WideMinW - 1) + 1)] + pairs_by_bucket[length_bucket(4096)];
    const int64_t slots4 = (int64_t)3 * n_cu, slots8 = (int64_t)2 * n_cu;
    const double rounds4 = std::ceil((double)n_wide / (double)slots4) * 1.26, rounds8 = std::ceil((double)n_wide / (double)slots8);
    // (up to 80 long pairs per CU: at 32 000 pairs the two are level -- 2.82e12 both at 4.9 kb, 2.66 against 2.83e12 at 3.7 kb --
    // and the chunked plans of ltr_calc_hap_aln_probs, 48 k and 144 k five-kb pairs each, ran 19 % slower on workgroups)
    R.wg_wide4 = R.sym_model && mode != 3 && (mode == 2 || (n_wide > 0 && n_long_pairs < (int64_t)80 * n_cu && rounds4 < 0.9 * rounds8));
    R.wide4_quota = INT64_MAX;
    // ... or BOTH: whole rounds of four-wave workgroups, the rest on eight waves (config5hifi: 1536 of its 1868 pairs as two
    // rounds of four-wave workgroups, the other 332 with the 180 longer pairs as one round of eight-wave ones).  Only while
    // the eight-wave kernels are in use at all (few long pairs), and only if the rounds say so.
    if (R.sym_model && mode < 0 && R.wg_long && n_wide > slots4) {
      const int64_t full = n_wide / slots4, rest = n_wide - full * slots4;
      const double split = (double)full * 1.26 + std::ceil((double)rest / (double)slots8);
      if (rest > 0 && split < 0.9 * rounds8 && split < rounds4) { R.wg_wide4 = true; R.wide4_quota = full * slots4; }
    }
  }
  {
    // A gap of L bases costs open + (L - 1) x extend + close, and which transitions those are depends on its direction
    // (HapAligner.cpp:285-295): the haplotype window LONGER than the read (n > m) is the insertion state -- match->ins f, ins->ins a,
    // ins->match b --, the read longer is the deletion state -- g, c, d.  A pair whose length difference alone costs more than ~520
    // of the 600 the reference allows cannot hold a one-cell-per-lane certificate: it starts with the exact body.  (Round 6: one
    // threshold per direction -- under a model with a != c the cheaper direction's threshold let the other direction's pairs through,
    // 214 of them in a 1250-locus shard, each a millisecond-long exact body met late in the launch.)
    auto first_risky = [](double open_close, double ext) -> int {
      return ext > 1e-3 ? (int)std::min(1.0e9, std::max(1.0, std::ceil((520.0 - open_close) / ext + 1.0))) : 0x7fffffff;
    };
    if (mode < 0) {
      R.risky_dd_pos = first_risky(std::fabs((double)mc.f) + std::fabs((double)mc.b), std::fabs((double)mc.a));
      R.risky_dd_neg = first_risky(std::fabs((double)mc.g) + std::fabs((double)mc.d), std::fabs((double)mc.c));
    }
  }
  R.wg_short = R.sym_model && mode == 2;
  // plan_knob (ltr_ctx_set_debug "plan_kernel"): 1 = never; 0 and -1 = the rule (every automatic-mode plan, any size, any model)
  // (Measured on MI355X against round 4's launches -- a launch per class / the multi-width launches, exact lists -- on cost shards
  // of config 3: 625 loci 15.1 against 17.8 ms per pass, 1250 loci 30.2 against 32.9, 5000 loci 118.1 against 122.3, all 10 000
  // loci 235.6 against 240.1; the catalogue: 12 500 loci 8.1 against 11.5, 50 000 loci 30.8 against 33.7, all 100 000 loci 60.7
  // against 62.7: profiles/r05/plan_kernel/.)
  // Round 6: the general model too (any seven negative transitions, HapAligner.h:111-119) -- ltr_dp_plan_kernel<false>, the 13-operation
  // cell, failed certificates by the generic exact body in line -- so that --alignment-params with ins != del keeps the one launch.
  R.plan_kernel = mode < 0 && plan_knob <= 0;
  {
    // the threshold test itself (every cell against thr(k), ltrp::build_threshold_table) depends on the band penalty only, not on the
    // model's symmetry: inside the plan kernel the general model's failed certificates and risky pairs take the threshold bodies too
    // (redo_thr_call<W, false>) instead of the byte-compare running-maximum body -- those few pairs were the tail of its small plans
    const float cabs = std::fabs(mc.c);
    const int64_t k600 = (cabs * 1.0e9f > 600.0f) ? ((int64_t)(600.0f / cabs) + 2) : (int64_t)1 << 40;
    R.thr_lists = R.xlut || (R.plan_kernel && k600 <= kPenKMax);
  }
  // (Workgroup launches beside the plan kernel wait for wave slots its persistent workgroups give back only at its end, and the
  // exact launches their failed certificates feed come after that: a 625-locus shard of config 3 -- a few dozen reads of ~1290
  // bases -- ended in them.  As two column blocks on one wavefront such reads are the plan kernel's first pairs, ~2 ms each.)
  // (a batch of fewer pairs than the GPU has wave slots keeps the workgroup kernels from 1281 columns on: nothing starves, and a
  // single locus of 2-kb reads is through sooner on four waves per pair)
  R.wg_min_c = (mode == 2) ? 64 * kWg1MaxW : ((R.plan_kernel && pairs_upper >= (int64_t)12 * n_cu) ? 2 * 64 * kWMax : 64 * kWMax);
  // Several pairs per wavefront is a throughput device: a wave of 64 / LP pairs is as long as its longest pair and a
  // batch that cannot fill the GPU's wave slots anyway (one locus at a time through ltr_process_reads: a few hundred
  // pairs) finishes sooner with one pair per wave.  Automatic mode: as many pairs per wave as still leave 16 waves
  // per CU -- two from 32 pairs per CU up (the rule of the two-per-wave kernels of round 2), 32 from 512 per CU up.
  R.pack_min_shift = 7;
  if (mode < 0) {
    const int64_t per_wave = pairs_upper / ((int64_t)16 * std::max(n_cu, 1));
    if (per_wave >= 2) {
      int np_shift = 1;
      while (np_shift < 6 - kPackMinShift && ((int64_t)2 << np_shift) <= per_wave) ++np_shift;
      R.pack_min_shift = 6 - np_shift;
      if (pack_rule == 2) R.pack_min_shift = kPackMinShift;
    }
  } else if (mode == 1 || (mode >= 5 && mode <= 8)) {
    R.pack_force_shift = (mode == 1) ? 5 : (9 - mode);           // 32 lanes per pair; 16, 8, 4, 2
    R.pack_min_shift = kPackMinShift;
  }
  for (int b = 0; b < kLengthBuckets; ++b) R.bucket_min_shift[b] = (int8_t)kPackMinShift;
  // (Round 4: the per-length floor is off by default, kept behind ltr_ctx_set_debug("pack_rule", 3).  It was there so that the
  // launch of a rare length still put two wavefronts on every SIMD -- when every (lanes per pair, strip width) class was a
  // launch of its own.  A packed launch is a whole strip width now, every lanes-per-pair range in one queue: measured on
  // MI355X, shards of config 3 with and without the floor: 625 loci 17.55 -> 17.13 ms per pass, 1250 loci 32.80 -> 32.34,
  // 2500 and 10 000 loci the same.)
  if (mode < 0 && pairs_by_bucket && pack_rule == 3) {
    const int64_t want_waves = (int64_t)2 * 4 * std::max(n_cu, 1);               // two wavefronts on every SIMD
    for (int b = 0; b < kLengthBuckets; ++b) {
      // (a launch class collects about a third of an octave of lengths: the bucket and its neighbours)
      const int64_t nb = pairs_by_bucket[b] + (b > 0 ? pairs_by_bucket[b - 1] : 0) + (b + 1 < kLengthBuckets ? pairs_by_bucket[b + 1] : 0);
      int np_shift = 0;
      while (np_shift < 6 - kPackMinShift && (nb >> (np_shift + 1)) >= want_waves) ++np_shift;
      R.bucket_min_shift[b] = (int8_t)(6 - np_shift);
    }
  }
  return R;
}

// steps x (cells of a step + what a step costs besides its cells, in cells) x share of the wave x what the register
// budget of the strip width costs in resident waves
static inline double occ_factor(int W) { return W <= 6 ? 1.0 : (W <= 12 ? 1.05 : 1.15); }
constexpr double kStepOverhead = 1.5;

double pack_cost(int n, int C, int lp_shift, int* W_out) {
  const int LP = 1 << lp_shift;
  const int W = (C + LP - 1) / LP;
  if (W_out) *W_out = W;
  if (W > kPackWMax) return 1e300;
  const int L = (C + W - 1) / W;
  return (double)(n - 1 + L - 1 + 1) * ((double)W + kStepOverhead) * occ_factor(W) * (double)LP / 64.0;     // (+ 1: the pair's set-up)
}

PairClass classify_pair(const Rules& R, int64_t n, int64_t m, int64_t hl, bool generic) {
  PairClass pc;
  pc.shortcut = (hl <= 60) || (std::llabs(n - m) > 600);
  double c = 1.0;
  int cls = -1;
  if (!pc.shortcut) {
    int ncb = 1;
    const int W = strip_width_for((int)m, &ncb);
    c = (double)ncb * (double)(n + 63) * (W + kStepOverhead);     // steps x (cells + per-step overhead)
    const int C = (int)m - 1;
    if (!generic && m >= 2 && n >= 2) {
      const bool wide = C > 4 * 64 * (kWg4WideMinW - 1) && C <= 4 * 64 * kWg4MaxW;     // four-wave strips of 15 .. 20 columns
      if (C > R.wg_min_c && C <= 4 * 64 * kWg4MaxW && (wide ? R.wg_wide4 : R.wg_long)) {   // four wavefronts on the pair
        const int Wg = std::max((C + 255) / 256, kWg4MinW);
        cls = kWg4First + Wg - kWg4MinW;
        c = (double)(n + 4 * 64) * (Wg + 2.0);
      } else if (R.wg_long && C > 4 * 64 * (kWg4WideMinW - 1) && C <= 8 * 64 * kWgWMax) {  // eight
        const int Wg = std::max((C + 511) / 512, kWg8MinW);
        cls = kWg8First + Wg - kWg8MinW;
        c = (double)(n + 8 * 64) * (Wg + 2.0);
      } else if (R.wg_short && C <= 64 * kWg1MaxW) {                             // one wavefront, inputs streamed through LDS
        const int Wg = (C + 63) / 64;
        cls = kWg1First + Wg - 1;
        c = (double)(n + 63) * (Wg + 2.0);
      } else if (R.pack_min_shift <= kPackMaxShift && C <= (kPackWMax << kPackMaxShift)) {
        // a read that fits LP lanes x kPackWMax columns can share its wavefront with 64 / LP - 1 other pairs
        int best_shift = 0, best_W = 0;
        double best = (ncb == 1 && R.pack_force_shift == 0) ? c * occ_factor(W) : 1e300;   // (one pair per wave, this wave all to itself)
        for (int s = std::max(std::max(R.pack_min_shift, (int)R.bucket_min_shift[length_bucket(C)]), kPackMinShift); s <= kPackMaxShift; ++s) {
          if (R.pack_force_shift != 0 && s < R.pack_force_shift) continue;
          int Wp = 0;
          const double cp = pack_cost((int)n, C, s, &Wp);
          if (cp < best) { best = cp; best_shift = s; best_W = Wp; }
          if (R.pack_force_shift != 0 && best_shift != 0) break;                  // forced: the narrowest segment from there up that fits
        }
        if (best_shift != 0) { cls = pack_class(best_shift, best_W); c = best; }
      }
    }
  }
  // which exact kernel scores the pair if its certificate fails (push_redo) -- or at once: pairs with bytes
  // outside ACGT (generic list) and, in mode 4, every pair
  const int64_t C = m - 1;
  int xc = kXGeneric;
  if (!generic && R.thr_lists && !pc.shortcut)
    xc = (C <= 64 * kXShortW) ? kXShort : ((C <= 64 * kXMidW) ? kXMid : ((C <= 64 * kXLongW) ? kXLong
         : ((C <= kXWg4MaxC) ? kXWg4 : ((C <= kXWg8MaxC) ? kXWg8 : kXLong))));
  pc.xc = (int8_t)xc;
  pc.x_candidate = !pc.shortcut || generic;
  // (risky pairs: only those a one-wave or packed class would take -- the workgroup classes keep theirs, their exact kernels are fed from the device)
  const bool risky = !pc.shortcut && (n - m >= R.risky_dd_pos || m - n >= R.risky_dd_neg) && (cls < 0 || cls < kWg4First);
  if (generic || (R.mode == 4 && !pc.shortcut) || risky) cls = kNumFast + xc;
  else if (cls < 0) cls = strip_width_for((int)m, nullptr) - 1;
  pc.uses_wg = (cls >= kWg4First && cls < kNumFast);
  pc.cls = (int16_t)cls;
  // (a pair that is scored always has a key >= 1 -- key 0 marks the constant-score pairs -- however small its cost)
  pc.cost = pc.shortcut ? 0.0 : c;
  pc.key = pc.shortcut ? (int16_t)0 : (int16_t)std::min(511, std::max(1, (c > 1.0 ? (int)(std::log2(c) * 16.0) : 0) - 16));
  return pc;
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
    bool any = false;
    {                                                                         // one-wave family
      const int min_fill = fold_rounds * 4 * n_cu;                            // (4 SIMDs per CU; ~3-4 resident wavefronts each: fold_rounds = 3 is one full round)
      int lo_w = 0;                                                           // narrowest strip folded into the running group
      // (the classes of strip widths kMultiMinW and up are one persistent launch when multi_launch is set, ltr_dp_multi_kernel:
      // a class of a few pairs costs nothing there, every pair keeps its own strip width)
      for (int j = 0; j + 1 < (multi_launch == 2 ? 0 : (multi_launch ? kMultiMinW : kNumBins)); ++j) {
        const int k = j, w = j + 1;
        if (counts[k] == 0) { lo_w = 0; continue; }
        if (lo_w == 0) lo_w = w;
        const bool fits = (w + 1 <= 4) || (3 * (w + 1) <= 4 * lo_w);
        // (only towards a class that has pairs of its own: a lone small class keeps its strip width)
        bool target = false;
        for (int j2 = j + 1; j2 < kNumBins && ((j2 + 1 <= 4) || (3 * (j2 + 1) <= 4 * lo_w)); ++j2) if (counts[j2] > 0) { target = true; break; }
        if (counts[k] < min_fill && fits && target) { counts[k + 1] += counts[k]; counts[k] = 0; remap[k] = k + 1; any = true; }
        else lo_w = 0;
      }
    }
    {
      // packed family: a launch is ONE strip width -- the pairs of every lanes-per-pair block of it (ltr_dp_pack.hpp) --
      // so what is folded is a whole width: every (LP, W) class of it into (LP, W + 1), while the wavefronts of the
      // width (groups of 64 / LP pairs) cannot fill the wave slots
      auto waves_of = [&](int w) {
        int64_t v = 0;
        for (int sft = kPackMinShift; sft <= kPackMaxShift; ++sft) { const int per = 64 >> sft; v += (counts[pack_class(sft, w)] + per - 1) / per; }
        return v;
      };
      const int64_t min_fill = (int64_t)fold_rounds * 4 * n_cu;
      int lo_w = 0;
      // (with multi_launch the widths kPackMultiMinW and up are one persistent launch, ltr_dp_pack_multi_kernel: nothing to fold there)
      for (int w = 1; w < (multi_launch == 2 ? 0 : (multi_launch ? kPackMultiMinW : kPackWMax)); ++w) {
        const int64_t wv = waves_of(w);
        if (wv == 0) { lo_w = 0; continue; }
        if (lo_w == 0) lo_w = w;
        const bool fits = (w + 1 <= 4) || (3 * (w + 1) <= 4 * lo_w);
        bool target = false;
        for (int w2 = w + 1; w2 <= kPackWMax && ((w2 <= 4) || (3 * w2 <= 4 * lo_w)); ++w2) if (waves_of(w2) > 0) { target = true; break; }
        if (wv < min_fill && fits && target) {
          for (int sft = kPackMinShift; sft <= kPackMaxShift; ++sft) {
            const int k = pack_class(sft, w);
            if (counts[k] == 0) continue;
            counts[k + 1] += counts[k]; counts[k] = 0; remap[k] = k + 1; any = true;
          }
        } else lo_w = 0;
      }
    }
    // ... and the workgroup families: a class of a few hundred pairs next to another one leaves both launches with a
    // partly filled last round of workgroups (measured on MI355X: 1116 + 420 five-kb pairs as W = 17 and W = 18
    // four-wave classes 2.05e12 cells/s, the neighbouring single-class lengths 2.5 - 2.7e12)
    for (int f = 0; f < 2; ++f) {
      const int first = f == 0 ? kWg4First : kWg8First, nk = f == 0 ? kNumWg4 : kNumWg8, w0 = f == 0 ? kWg4MinW : kWg8MinW;
      const int min_fill = fold_rounds * n_cu;                                // (two or three workgroups per CU: two to three rounds)
      int lo_w = 0;
      for (int j = 0; j + 1 < nk; ++j) {
        const int k = first + j, w = w0 + j;
        if (counts[k] == 0) { lo_w = 0; continue; }
        if (lo_w == 0) lo_w = w;
        const bool fits = 3 * (w + 1) <= 4 * lo_w;
        bool target = false;
        for (int j2 = j + 1; j2 < nk && 3 * (w0 + j2) <= 4 * lo_w; ++j2) if (counts[first + j2] > 0) { target = true; break; }
        if (counts[k] < min_fill && fits && target) { counts[k + 1] += counts[k]; counts[k] = 0; remap[k] = k + 1; any = true; }
        else lo_w = 0;
      }
    }
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

void build_threshold_table(float c32, double* out) {
  const float cabs = std::fabs(c32);
  const int k600 = (cabs * 1.0e9f > 600.0f) ? ((int)(600.0f / cabs) + 2) : 0x3fffffff;   // as the kernels form it
  const double inf = std::numeric_limits<double>::infinity();
  auto bits = [](double v) { int64_t b; std::memcpy(&b, &v, 8); return b; };
  auto dbl = [](int64_t b) { double v; std::memcpy(&v, &b, 8); return v; };
  for (int idx = 0; idx < kPenTabDoubles; ++idx) {
    const int k = std::abs(idx - kPenHalf);
    const volatile double p = (double)((float)k * c32);        // int * float -> float, HapAligner.cpp:298 (volatile: no contraction, no excess precision)
    const double x0 = -600.0 - p;
    double thr = inf;
    if (k < k600 && k <= kPenKMax && x0 < -1e-6) {
      // bisection over the bit patterns between a double that passes and one that fails (both negative: the larger pattern is
      // further down).  Steps of one ulp from x0 do not get there: at k = 597, c = -1 x0 is -3 and the threshold half an ulp
      // of 600 = 128 ulps of 3 below it.
      int64_t lo = bits(x0 + 1e-9), hi = bits(x0 - 1e-9);
      while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        const volatile double sum = dbl(mid) + p;
        if (sum >= -600.0) lo = mid; else hi = mid;
      }
      thr = dbl(lo);
    }
    out[idx] = thr;
  }
}

// ---- haplotype families (ltr_plan.h) -------------------------------------------------------------------------------------------

static int32_t common_prefix(const uint8_t* a, const uint8_t* b2, int32_t len) {
  int32_t k = 0;
  for (; k + 8 <= len; k += 8) {
    uint64_t x, y;
    std::memcpy(&x, a + k, 8); std::memcpy(&y, b2 + k, 8);
    if (x != y) return k + (__builtin_ctzll(x ^ y) >> 3);
  }
  for (; k < len && a[k] == b2[k]; ++k) {}
  return k;
}

void form_families(const ltr_locus_batch* b, const ModelConsts& mc, const int F, const int n_cu, const int knob, const int min_rows_in,
                   const std::vector<int64_t>& pair_base, const BatchScratch& w, std::vector<FamilyRec>* out) {
  RawBuf<PairDesc>& pairs = w.pairs; RawBuf<int16_t>& key = w.key; RawBuf<int16_t>& bin = w.bin;
  const int min_rows = std::max(min_rows_in, 2);                 // (the stem has a row of its own)
  // lpc as the device table holds it (ltr_ctx.hip, build_tables): lpc[1] = 0, lpc[j+1] = lpc[j] + c
  // (as far as a fork row can reach: p <= n - 1 and a member's n <= m + 600 <= kFamilyMaxC + 601)
  std::vector<double> lpc((size_t)kFamilyMaxC + 600 + 4, 0.0);
  for (size_t j = 1; j + 1 < lpc.size(); ++j) lpc[j + 1] = lpc[j] + (double)mc.c;
  const double cg = (double)mc.g, cd = (double)mc.d, ca = (double)mc.a, cc = (double)mc.c, cf = (double)mc.f, MATCH = (double)mc.match;
  constexpr int kMaxH = 64;
  std::vector<std::vector<FamilyRec>> per_locus((size_t)b->n_loci);
  ltr::parallel_for(b->n_loci, 64, [&](int64_t l) {
    const int64_t r0 = b->locus_read_off[l], r1 = b->locus_read_off[l + 1];
    const int64_t h0 = b->locus_hap_off[l], h1 = b->locus_hap_off[l + 1];
    const int64_t H = h1 - h0;
    if (H < 2 || H > kMaxH) return;
    const uint8_t* win[kMaxH]; int32_t wn[kMaxH];
    int32_t lcp[kMaxH][kMaxH];                                   // longest common prefix of two windows, -1: not formed yet
    bool have_windows = false;
    int64_t at = pair_base[(size_t)l];
    for (int64_t r = r0; r < r1; ++r) {
      if (b->realign_read && !b->realign_read[r]) continue;
      const int64_t row_at = at;
      int64_t n_here = 0;
      for (int64_t h = h0; h < h1; ++h) if (!b->realign_hap || b->realign_hap[h]) ++n_here;
      at += n_here;
      const int64_t m = b->read_off[r + 1] - b->read_off[r];
      const int C = (int)m - 1;
      // the narrow band: by rule and on request 2 (knob 1 keeps to the wide band)
      const bool narrow = C >= kFamilyNarrowMinC && C <= kFamilyNarrowMaxC && (knob == 0 || knob >= 2);
      if (!narrow && (C < kFamilyMinC || C > kFamilyMaxC)) continue;
      const int W = (C + 63) / 64, L = (C + W - 1) / W;
      // (the narrow band's pairs as the class rule packs them: two to a wavefront, 32 lanes of Wp columns)
      const int Wp = (C + (1 << kPackMaxShift) - 1) >> kPackMaxShift, Lp = (C + Wp - 1) / Wp;
      const int own_cls = narrow ? pack_class(kPackMaxShift, Wp) : W - 1;
      // candidates: what the class rule left in the one-wave class of the read's own strip width -- the narrow band: in the packed
      // class of 32 lanes; on request 2 also in the one-wave class, where a batch too small to pack leaves them --, with a DP to run
      int cand_h[kMaxH]; int64_t cand_i[kMaxH]; int nc = 0;
      {
        int64_t i = row_at;
        for (int64_t h = h0; h < h1; ++h) {
          if (b->realign_hap && !b->realign_hap[h]) continue;
          if ((bin[(size_t)i] == own_cls || (narrow && knob >= 2 && bin[(size_t)i] == W - 1)) && key[(size_t)i] > 0 && pairs[(size_t)i].generic == 0 && pairs[(size_t)i].n >= 2) { cand_h[nc] = (int)(h - h0); cand_i[nc] = i; ++nc; }
          ++i;
        }
      }
      if (nc < 2) continue;
      if (!have_windows) {
        for (int64_t h = h0; h < h1; ++h) {
          const int64_t hl = b->hap_off[h + 1] - b->hap_off[h];
          int64_t pos = 0;
          const int64_t n = hl > 60 ? ltr::hap_window(hl, F, &pos) : 0;
          win[h - h0] = b->hap_bytes + b->hap_off[h] + pos; wn[h - h0] = (int32_t)std::max<int64_t>(n, 0);
          for (int64_t h2 = h0; h2 < h1; ++h2) lcp[h - h0][h2 - h0] = -1;
        }
        have_windows = true;
      }
      auto lcp_of = [&](int x, int y) {
        if (lcp[x][y] < 0) lcp[x][y] = lcp[y][x] = common_prefix(win[x], win[y], std::min(wn[x], wn[y]));
        return lcp[x][y];
      };
      // the fork of the candidates, then -- once -- of those whose score has a chance against its bound (fewer members: p can only
      // grow and U only fall, so whoever passes the first bound passes the second)
      int p = 0; double U = 0.0;
      for (int pass = 0; pass < 2 && nc >= 2; ++pass) {
        p = 0x7fffffff;
        for (int k = 0; k < nc; ++k) p = std::min(p, std::min(k ? lcp_of(cand_h[0], cand_h[k]) : 0x7fffffff, wn[cand_h[k]] - 1));
        if (p < min_rows) { nc = 0; break; }
        if ((size_t)p >= lpc.size()) { nc = 0; break; }               // (cannot happen: see the table's size)
        U = ((cg + lpc[(size_t)p - 1]) + cd) + MATCH;
        if (pass) break;
        int kept = 0;
        for (int k = 0; k < nc; ++k) {
          const int dd = wn[cand_h[k]] - (int)m;
          // (the haplotype window longer than the read is the insertion state, the read longer the deletion state: make_rules)
          const double gap = dd > 0 ? cf + (double)(dd - 1) * ca : (dd < 0 ? cg + (double)(-dd - 1) * cc : 0.0);
          if (gap > U) { cand_h[kept] = cand_h[k]; cand_i[kept] = cand_i[k]; ++kept; }
        }
        if (kept == nc) break;
        nc = kept;
      }
      if (nc < 2 || nc > kFamilyMaxMembers) continue;
      int64_t fam_steps = (p - 1) + (L - 1), own_steps = 0;
      int dd_min = 0x7fffffff, dd_max = -0x7fffffff;
      for (int k = 0; k < nc; ++k) {
        const int n = wn[cand_h[k]];
        fam_steps += (n - p) + (L - 1); own_steps += (n - 1) + (L - 1);
        dd_min = std::min(dd_min, n - (int)m); dd_max = std::max(dd_max, n - (int)m);
      }
      if (!narrow) {
        if (knob <= 0 && fam_steps >= own_steps) continue;
      } else if (knob <= 0) {
        // the geometries differ, so modelled WORK is compared, not steps: the family's steps on a whole wavefront of strips of W
        // against the members' own steps on half a wavefront of strips of Wp (formed here rather than read back from the pairs'
        // launch-order keys, which hold the packed cost only to 1/16 octave)
        double own_work = 0.0;
        for (int k = 0; k < nc; ++k) own_work += (double)((wn[cand_h[k]] - 1) + (Lp - 1)) * ((double)Wp + kStepOverhead) * (double)(1 << kPackMaxShift) / 64.0;
        if ((double)fam_steps * ((double)W + kStepOverhead) >= own_work) continue;
      }
      const double c = (double)fam_steps * (W + kStepOverhead);
      const int16_t fkey = (int16_t)std::min(511, std::max(1, (c > 1.0 ? (int)(std::log2(c) * 16.0) : 0) - 16));
      FamilyRec rec;
      rec.first_pair = cand_i[0]; rec.U = U; rec.row_at = row_at; rec.members = 0; rec.key = fkey;
      for (int k = 0; k < nc; ++k) rec.members |= 1ull << (cand_i[k] - row_at);
      rec.f.first = 0; rec.f.count = nc; rec.f.p = p; rec.f.W = W; rec.f.dd_min = dd_min; rec.f.dd_max = dd_max;
      per_locus[(size_t)l].push_back(rec);
    }
  });
  out->clear();
  for (const std::vector<FamilyRec>& v : per_locus) out->insert(out->end(), v.begin(), v.end());     // (ascending first_pair: loci, then reads, in batch order)
  // A launch of its own pays once the batch fills the GPU: one wavefront runs a family's stem and all its tails one after the other, so
  // a family lasts as long as ~H pairs on one wave slot, and the families are dealt out statically.  Measured on MI355X (config-3 loci,
  // families on request against none, kernel ms per pass): 16 families 1.52 against 0.38, 272 families 2.37 against 1.07, 533 families
  // (4311 pairs) 2.04 against 1.40 -- the pass stays one family long while the plan kernel spreads the same pairs over idle wave slots.
  // By rule: from a family for every wavefront of a full grid up (kFamPerCu per CU: three workgroups of four); knobs 1 and 2: whenever
  // one can be formed.  The narrow band by rule only when its families ALONE are a full grid's worth: below that a plan keeps the
  // launches it had -- its packed pairs stay with the plan kernel, its wide families are counted as before -- so that a plan of a few
  // hundred loci runs exactly as it did without the band (a 300-locus plain run of config 3 on 256 CUs: 2271 narrow families, not
  // formed; 625 loci: 4571, formed).  Then both bands together against the same count.
  if (knob <= 0) {
    const int64_t want = (int64_t)kFamPerCu * std::max(n_cu, 1);
    const auto is_narrow = [](const FamilyRec& r) { return r.f.W * 64 <= kFamilyNarrowMaxC; };
    if ((int64_t)std::count_if(out->begin(), out->end(), is_narrow) < want) out->erase(std::remove_if(out->begin(), out->end(), is_narrow), out->end());
    if ((int64_t)out->size() < want) out->clear();
  }
  ltr::parallel_for((int64_t)out->size(), 256, [&](int64_t i) {
    const FamilyRec& r = (*out)[(size_t)i];
    for (uint64_t rest = r.members; rest; rest &= rest - 1) {
      const size_t at = (size_t)(r.row_at + __builtin_ctzll(rest));
      bin[at] = (int16_t)kFamClass; key[at] = r.key;
    }
  });
}

// ---- describe_batch: the host half of ltr_plan_create ------------------------------------------------------------------------

// What the batch as a whole decides is decided from these: pairs (upper bound), pairs of reads beyond one wavefront's widest
// strips, pairs by read length (quarter octaves).
static int count_lengths(const ltr_locus_batch* b, int64_t* pairs_upper_out, int64_t* n_long_pairs_out, int64_t* by_bucket, std::string* err) {
  int64_t pairs_upper = 0, n_long_pairs = 0;
  {
    // (blocks of loci on the host cores, partial sums merged under a lock: serial, this loop and the two below were 1.1 ms of the
    // 3.2 ms a 10 000-locus chunk of ltr_calc_hap_aln_probs spends in here)
    std::mutex acc_mu;
    std::atomic<int> bad(0);
    const int64_t n_blk0 = (b->n_loci + 255) / 256;
    ltr::parallel_for(n_blk0, b->n_loci < 2048 ? n_blk0 + 1 : 1, [&](int64_t c) {
      int64_t pu = 0, nlp = 0, bb[ltrp::kLengthBuckets] = {0};
      for (int64_t l = c * 256; l < std::min<int64_t>(b->n_loci, (c + 1) * 256); ++l) {
        const int64_t r0 = b->locus_read_off[l], r1 = b->locus_read_off[l + 1], h0 = b->locus_hap_off[l], h1 = b->locus_hap_off[l + 1];
        if (r0 < 0 || r1 < r0 || r1 > b->n_reads || h0 < 0 || h1 < h0 || h1 > b->n_haps) { bad.store(1, std::memory_order_relaxed); return; }
        pu += (r1 - r0) * (h1 - h0);
        int64_t nl = 0;
        for (int64_t r = r0; r < r1; ++r) {
          const int64_t C = b->read_off[r + 1] - b->read_off[r] - 1;
          nl += (C > 64 * kWMax);
          bb[ltrp::length_bucket((int)std::max<int64_t>(std::min<int64_t>(C, 1 << 24), 0))] += h1 - h0;
        }
        nlp += nl * (h1 - h0);
      }
      std::lock_guard<std::mutex> lk2(acc_mu);
      pairs_upper += pu; n_long_pairs += nlp;
      for (int q = 0; q < ltrp::kLengthBuckets; ++q) by_bucket[q] += bb[q];
    }, 1);
    if (bad.load()) { *err = "locus offsets out of range"; return LTR_ERR_INVALID; }
  }
  *pairs_upper_out = pairs_upper; *n_long_pairs_out = n_long_pairs;
  return LTR_OK;
}

// which sequences are pure upper-case ACGT (the LUT emission of the fast kernels needs that)
// (16 bytes per step with SSE2 -- part of x86-64 --: the byte loop, which hipcc's host pass does not vectorise, was 1.4 - 1.5 ms
// of the 5.3 ms of plan creation per 10 000 catalogue loci; 4.4 x faster per thread here)
static bool acgt_only(const uint8_t* p, int64_t len) {
  int64_t k = 0;
#if defined(__SSE2__)
  const __m128i cA = _mm_set1_epi8('A'), cC = _mm_set1_epi8('C'), cG = _mm_set1_epi8('G'), cT = _mm_set1_epi8('T');
  __m128i all = _mm_set1_epi8((char)0xff);
  for (; k + 16 <= len; k += 16) {
    const __m128i v = _mm_loadu_si128((const __m128i*)(p + k));
    all = _mm_and_si128(all, _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(v, cA), _mm_cmpeq_epi8(v, cC)), _mm_or_si128(_mm_cmpeq_epi8(v, cG), _mm_cmpeq_epi8(v, cT))));
  }
  if (_mm_movemask_epi8(all) != 0xffff) return false;
#endif
  unsigned ok = 1;
  for (; k < len; ++k) { const uint8_t c = p[k]; ok &= (unsigned)((c == 'A') | (c == 'C') | (c == 'G') | (c == 'T')); }
  return ok != 0;
}

// Offsets ascending; which reads and haplotypes are pure ACGT (w.read_acgt, w.hap_acgt).
static int scan_sequences(const ltr_locus_batch* b, const BatchScratch& w, std::string* err) {
  RawBuf<uint8_t>& read_acgt = w.read_acgt; RawBuf<uint8_t>& hap_acgt = w.hap_acgt;
  read_acgt.resize((size_t)b->n_reads); hap_acgt.resize((size_t)b->n_haps);
  {
    std::atomic<int> bad(0);                                              // 1: reads, 2: haplotypes
    ltr::parallel_for((b->n_reads + 4095) / 4096, 1, [&](int64_t c) {
      for (int64_t r = c * 4096; r < std::min<int64_t>(b->n_reads, (c + 1) * 4096); ++r) if (b->read_off[r + 1] < b->read_off[r]) { bad.store(1, std::memory_order_relaxed); return; }
    }, 1);
    ltr::parallel_for((b->n_haps + 4095) / 4096, 1, [&](int64_t c) {
      for (int64_t h = c * 4096; h < std::min<int64_t>(b->n_haps, (c + 1) * 4096); ++h) if (b->hap_off[h + 1] < b->hap_off[h]) { int e = 0; bad.compare_exchange_strong(e, 2); return; }
    }, 1);
    if (bad.load() == 1) { *err = "read offsets not ascending"; return LTR_ERR_INVALID; }
    if (bad.load() == 2) { *err = "haplotype offsets not ascending"; return LTR_ERR_INVALID; }
  }
  LTR_DBG("plan: offsets checked");
  // (the byte scans run on the host cores: ~180 MB per 10 k loci)
  ltr::parallel_for(b->n_reads, 512, [&](int64_t r) {
    read_acgt[(size_t)r] = acgt_only(b->read_bytes + b->read_off[r], b->read_off[r + 1] - b->read_off[r]); });
  ltr::parallel_for(b->n_haps, 512, [&](int64_t h) {
    hap_acgt[(size_t)h] = acgt_only(b->hap_bytes + b->hap_off[h], b->hap_off[h + 1] - b->hap_off[h]); });
  LTR_DBG("plan: bytes scanned");
  return LTR_OK;
}

// One descriptor, launch class and launch-order key per pair (w.pairs, w.bin, w.key, batch order); the per-locus and whole-batch
// figures of *d.
static int enumerate_pairs(const ltr_locus_batch* b, const Rules& rules, const int F, const BatchScratch& w, BatchPlan* d, std::vector<int64_t>* pair_base_out, std::string* err) {
  RawBuf<PairDesc>& pairs = w.pairs;
  RawBuf<int16_t>& key = w.key;      // launch-order key of every pair
  RawBuf<int16_t>& bin = w.bin;      // launch class of every pair
  const RawBuf<uint8_t>& read_acgt = w.read_acgt; const RawBuf<uint8_t>& hap_acgt = w.hap_acgt;
  int64_t ll_off = 0;
  int32_t max_len = 1;
  d->seed.assign((size_t)b->n_reads, -1);
  double in_bytes = 0.0, cells = 0.0;
  // ---- pass 1 (serial, cheap): per-locus output offsets and pair counts -> where every locus' pairs go ----
  std::vector<int64_t>& pair_base = *pair_base_out;
  pair_base.assign((size_t)b->n_loci + 1, 0);
  d->locus_P.reserve((size_t)b->n_loci); d->locus_H.reserve((size_t)b->n_loci); d->locus_ll_off.reserve((size_t)b->n_loci);
  for (int64_t l = 0; l < b->n_loci; ++l) {
    const int64_t r0 = b->locus_read_off[l], r1 = b->locus_read_off[l + 1];
    const int64_t h0 = b->locus_hap_off[l], h1 = b->locus_hap_off[l + 1];
    const int64_t H = h1 - h0;
    d->locus_P.push_back((int32_t)(r1 - r0)); d->locus_H.push_back((int32_t)H); d->locus_ll_off.push_back(ll_off);
    in_bytes += (double)(b->read_off[r1] - b->read_off[r0]) + (double)(b->hap_off[h1] - b->hap_off[h0]) + 8.0 * (double)(r1 - r0) * (double)H;
    int64_t nr = r1 - r0, nh = H;
    if (b->realign_read) { nr = 0; for (int64_t r = r0; r < r1; ++r) nr += b->realign_read[r] ? 1 : 0; }
    if (b->realign_hap) { nh = 0; for (int64_t h = h0; h < h1; ++h) nh += b->realign_hap[h] ? 1 : 0; }
    pair_base[(size_t)l + 1] = pair_base[(size_t)l] + nr * nh;
    ll_off += (r1 - r0) * H;
  }
  const int64_t n_pairs_total = pair_base[(size_t)b->n_loci];
  LTR_DBG("plan: %ld pairs counted", (long)n_pairs_total);
  if (n_pairs_total > 0x7fffffff) { *err = "too many pairs in one batch"; return LTR_ERR_INVALID; }
  // (the plan kernel's per-wave notes carry flags in bits 30 and 31 of a pair index -- kNotePlain, "generic body": a plan of 2^30
  // pairs and more, > 40 GB of descriptors, keeps a launch per class)
  if (n_pairs_total >= ((int64_t)1 << 30)) d->use_plan = false;
  pairs.resize((size_t)n_pairs_total); key.resize((size_t)n_pairs_total); bin.resize((size_t)n_pairs_total);
  LTR_DBG("plan: arrays sized");
  // ---- pass 2 (all host cores): one descriptor, launch class and launch-order key per pair (ltrp::classify_pair) ----
  struct ClassMemo { uint64_t tag = ~0ull, plan_id = 0; ltrp::PairClass pc; };
  constexpr int kClassMemoBits = 12;
  static std::atomic<uint64_t> plan_counter{0};
  const uint64_t plan_id = plan_counter.fetch_add(1) + 1;            // (the rules differ from plan to plan)
  struct LocusAcc { double cells = 0.0; int32_t max_len = 1; int64_t xcand[kNumExact] = {0}, xstart[kNumExact] = {0}; uint8_t uses_wg = 0; int8_t err = 0; };
  std::vector<LocusAcc> acc((size_t)b->n_loci);
  ltr::parallel_for(b->n_loci, 256, [&](int64_t l) {
    const int64_t r0 = b->locus_read_off[l], r1 = b->locus_read_off[l + 1];
    const int64_t h0 = b->locus_hap_off[l], h1 = b->locus_hap_off[l + 1];
    const int64_t H = h1 - h0, ll_base = d->locus_ll_off[(size_t)l];
    LocusAcc& A2 = acc[(size_t)l];
    int64_t at = pair_base[(size_t)l];
    static thread_local std::vector<ClassMemo> memo_store;
    if (memo_store.empty()) memo_store.resize((size_t)1 << kClassMemoBits);
    ClassMemo* memo = memo_store.data();
    for (int64_t r = r0; r < r1; ++r) {
      if (b->realign_read && !b->realign_read[r]) continue;
      const int64_t m = b->read_off[r + 1] - b->read_off[r];
      if (m <= 0 || m > (1 << 20)) { A2.err = 1; return; }
      d->seed[(size_t)r] = (int32_t)m - 1;
      for (int64_t h = h0; h < h1; ++h) {
        if (b->realign_hap && !b->realign_hap[h]) continue;
        const int64_t hl = b->hap_off[h + 1] - b->hap_off[h];
        if (hl < 0 || hl > (1 << 20)) { A2.err = 2; return; }
        PairDesc pd;
        pd.read_off = b->read_off[r]; pd.out_idx = ll_base + (r - r0) * H + (h - h0);
        pd.m = (int32_t)m; pd.hap_full_len = (int32_t)hl;
        pd.generic = (read_acgt[(size_t)r] && hap_acgt[(size_t)h]) ? 0 : 1;
        int64_t pos = 0, n = 0;
        if (hl > 60) {
          n = ltr::hap_window(hl, F, &pos);
          if (n <= 0) { A2.err = 3; return; }
        }
        pd.hap_off = b->hap_off[h] + pos; pd.n = (int32_t)n;
        // (the rule's answer for (n, m, hl, generic) is kept per host thread in a direct-mapped table, tagged with the plan: a
        // catalogue of short repeats asks for the same few thousand combinations over and over, and the rule -- five packed
        // segment widths costed per pair, a logarithm -- was 120 ns per pair, 1.8 ms per 235 000-pair chunk on 16 threads)
        ltrp::PairClass pc;
        {
          const uint64_t tag = (uint64_t)n | ((uint64_t)m << 21) | ((uint64_t)hl << 42) | ((uint64_t)pd.generic << 63);   // (n, m, hl <= 2^20)
          ClassMemo& E = memo[(size_t)((tag * 0x9E3779B97F4A7C15ull) >> (64 - kClassMemoBits))];
          if (E.tag != tag || E.plan_id != plan_id) { E.pc = ltrp::classify_pair(rules, n, m, hl, pd.generic != 0); E.tag = tag; E.plan_id = plan_id; }
          pc = E.pc;
        }
        if (!pc.shortcut) {
          A2.cells += (double)n * (double)m;
          A2.max_len = std::max<int32_t>(A2.max_len, (int32_t)std::max(n, m));
        }
        // (under the plan kernel the one-wave and packed classes score their failed certificates themselves, and so it does the
        // pairs that start out in a list: only the workgroup classes feed the exact launches)
        if (pc.x_candidate && (!d->use_plan || pc.uses_wg)) A2.xcand[pc.xc]++;
        else if (pc.x_candidate && pc.cls >= kNumFast) A2.xstart[pc.xc]++;
        if (pc.uses_wg) A2.uses_wg = 1;
        pairs[(size_t)at] = pd; bin[(size_t)at] = pc.cls; key[(size_t)at] = pc.key;
        ++at;
      }
    }
    // (Launch order inside a class is longest pair first, nothing else.  Keeping the pairs of a locus together --
    // one launch-order key per locus, in steps of 1/16 octave, so that the 30 reads of a haplotype are popped by
    // neighbouring waves -- was measured on MI355X: the L2 fetch volume of the large launches did not move
    // (125 MB each: consecutive pops land on different XCDs, each with its own L2) and the pass went from 245.6
    // to 257.6 ms on the coarser longest-first order.)
  });
  for (int64_t l = 0; l < b->n_loci; ++l) {
    const LocusAcc& A2 = acc[(size_t)l];
    if (A2.err) {
      *err = A2.err == 1 ? "empty or oversized read (the reference is undefined for an empty read)"
                         : (A2.err == 2 ? "bad haplotype length"
                                        : "haplotype window is empty (only possible with indel_flank_len < 5; undefined in the reference)");
      return LTR_ERR_INVALID;
    }
    cells += A2.cells; max_len = std::max(max_len, A2.max_len);
    for (int c = 0; c < kNumExact; ++c) { d->xcand[c] += A2.xcand[c]; d->xstart[c] += A2.xstart[c]; }
    if (A2.uses_wg) d->uses_wg = true;
  }
  d->ll_size = ll_off; d->n_pairs = n_pairs_total;
  d->cells = cells; d->input_bytes = in_bytes; d->max_len = max_len;
  return LTR_OK;
}

int describe_batch(const ltr_locus_batch* b, const ModelConsts& mc, const int F, const int mode, const int n_cu, const ltr::DebugKnobs& dbg,
                   const BatchScratch& w, BatchPlan* d, std::string* err) {
  if (b->n_loci < 0 || b->n_reads < 0 || b->n_haps < 0) { *err = "negative counts"; return LTR_ERR_INVALID; }
  if (b->n_loci > 0 && (!b->locus_read_off || !b->locus_hap_off || !b->read_off || !b->hap_off)) { *err = "null offset array"; return LTR_ERR_INVALID; }
  // ---- what the batch as a whole decides: packing, workgroup kernels, exact kernel flavour (ltr_plan.cpp) ----
  int64_t pairs_upper = 0, n_long_pairs = 0;
  int64_t by_bucket[ltrp::kLengthBuckets] = {0};                          // pairs by read length (quarter octaves)
  int rc = count_lengths(b, &pairs_upper, &n_long_pairs, by_bucket, err);
  if (rc != LTR_OK) return rc;
  LTR_DBG("plan: lengths counted");
  const ltrp::Rules rules = ltrp::make_rules(mc, F, mode, n_cu, pairs_upper, n_long_pairs, by_bucket, dbg.pack_rule, dbg.plan_kernel);
  d->sym_at_create = rules.sym_model;
  d->xlut = rules.xlut;
  // The plan kernel (ltr_dp_plan.hpp): every plan of the automatic mode, whatever its size and whatever the indel model (round 6:
  // the general-model instance; ltrp::make_rules; ltr_ctx_set_debug "plan_kernel": 1 = never).  Measured on MI355X, cost shards of
  // config 3 (tests/manual/gpu_plan_ab.py), plan kernel against round 4's launches: profiles/r05/plan_kernel/.
  d->use_plan = rules.plan_kernel;
  std::vector<int64_t> pair_base;
  if ((rc = scan_sequences(b, w, err)) != LTR_OK || (rc = enumerate_pairs(b, rules, F, w, d, &pair_base, err)) != LTR_OK) return rc;
  RawBuf<PairDesc>& pairs = w.pairs; RawBuf<int16_t>& bin = w.bin;
  const int64_t n_pairs_total = d->n_pairs;
  // haplotype families: their members leave the one-wave classes (the plan kernel never sees them) for a class of their own
  std::vector<FamilyRec> fam_recs;
  if (d->use_plan && rules.sym_model && dbg.families >= 0)
    form_families(b, mc, F, n_cu, dbg.families, dbg.family_min_rows > 0 ? dbg.family_min_rows : kFamMinRows, pair_base, w, &fam_recs);

  // Whole rounds of four-wave workgroups for the reads of 3.6 - 5.1 kb, the rest of them on eight waves (make_rules): the
  // pairs beyond the quota -- the last ones in batch order -- move to the eight-wave class of their length.
  if (rules.wg_wide4 && rules.wide4_quota != INT64_MAX) {
    int64_t seen = 0;
    for (int64_t i = 0; i < n_pairs_total; ++i) {
      const int k = bin[(size_t)i];
      if (k < kWg4First + (ltrp::kWg4WideMinW - kWg4MinW) || k >= kWg8First) continue;
      if (++seen <= rules.wide4_quota) continue;
      const int C = pairs[(size_t)i].m - 1;
      bin[(size_t)i] = (int16_t)(kWg8First + std::max((C + 511) / 512, kWg8MinW) - kWg8MinW);
    }
  }
  LTR_DBG("plan: pairs described");
  // ---- bin by launch class, longest first inside a class (ltrp::sort_by_class; all host cores) ----
  // pairs with bytes outside ACGT ("generic") sit behind every certificate class: they skip the LUT kernels
  // and are pre-seeded into the exact kernel's list
  // Multi-width launches (ltr_dp_multi_kernel, ltr_dp_pack_multi_kernel: the one-wave classes of strip widths 11 .. 20 /
  // the packed widths 13 .. 20 as one persistent launch each) in automatic mode for plans of 512 .. 4096 pairs per CU.
  // Measured on MI355X against a launch per class (tests/manual/gpu_multi_ab.py): a 1250-locus shard of config 3 (717 pairs
  // per CU) 32.7 against 33.5 ms per pass, 8 certificate launches against 17; a 12 500-locus shard of the catalogue 10.6
  // against 11.6.  Below: a 625-locus shard -- 360 pairs per CU -- 18.3 against 17.6: with a handful of launches left the
  // two launch streams have little to fill each other's ends with.  Above: config 3 whole (5730 per CU) 240.0 against 240.4,
  // the catalogue whole 62.3 against 62.3 -- nothing to gain, and every call into a class's body saves its callee-saved
  // registers: ~0.9 GB of scratch write-backs per config-3 pass (rocprofv3 WRITE_SIZE; no time, but 5 x the pass's
  // algorithmic bytes) that a launch per class does not write.
  d->use_multi = !d->use_plan && mode < 0 && dbg.no_multi <= 0 &&
                         (dbg.no_multi < 0 || (n_pairs_total >= (int64_t)512 * n_cu && n_pairs_total < (int64_t)4096 * n_cu));
  RawBuf<int32_t>& order = w.order;
  order.resize(pairs.size());
  ltrp::sort_by_class(bin.data(), w.key.data(), (int64_t)pairs.size(), mode < 0 ? (dbg.fold_rounds > 0 ? dbg.fold_rounds : ltrp::kFoldRounds) : 0, n_cu,
                      order.data(), d->bin_first, d->counts, d->use_plan ? 2 : (d->use_multi ? 1 : 0));
  for (int c = 0; c < kNumExact; ++c) d->x_seed[c] = d->counts[kNumFast + c];
  LTR_DBG("plan: sorted");
  RawBuf<PairDesc>& sorted = w.sorted;
  sorted.resize(pairs.size());
  ltr::parallel_for((int64_t)((pairs.size() + kPlanBlock - 1) / kPlanBlock), 1, [&](int64_t c) {
    for (size_t i = (size_t)c * kPlanBlock; i < std::min(pairs.size(), ((size_t)c + 1) * kPlanBlock); ++i) sorted[i] = pairs[(size_t)order[i]];
  }, 1);
  LTR_DBG("plan: gathered");
  // the families in the order the sort left their members in: a family's members are one run of the family class, its first
  // member first (input order inside a key)
  d->fams.clear(); d->fam_U.clear(); d->fam_members = 0;
  for (int i = d->bin_first[kFamClass]; i < d->bin_first[kFamClass + 1];) {
    const int64_t orig = order[(size_t)i];
    const auto it = std::lower_bound(fam_recs.begin(), fam_recs.end(), orig, [](const FamilyRec& r, int64_t v) { return r.first_pair < v; });
    bool ok = it != fam_recs.end() && it->first_pair == orig && i + it->f.count <= d->bin_first[kFamClass + 1];
    for (int k = 0; ok && k < it->f.count; ++k)
      ok = sorted[(size_t)(i + k)].read_off == sorted[(size_t)i].read_off && sorted[(size_t)(i + k)].m == sorted[(size_t)i].m && sorted[(size_t)(i + k)].n - 1 >= it->f.p;
    if (!ok) { *err = "internal error: a haplotype family's members are not contiguous in the sorted pair list"; return LTR_ERR_INVALID; }
    FamilyDesc f = it->f;
    f.first = i;
    d->fams.push_back(f); d->fam_U.push_back(it->U); d->fam_members += f.count;
    i += f.count;
  }
  return LTR_OK;
}

// ---- class statistics and the launch schedule ----------------------------------------------------------------------------------

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

// ---- test hooks (include/ltr_gpu.h, "planning units"): the rule and the sort without a GPU -------------------
extern "C" {

int ltr_debug_num_classes(void) { return ltrp::kNumKernels; }

int ltr_debug_class_info(int k, int* family, int* strip_width, int* waves_per_pair, int* lanes_per_pair) {
  if (k < 0 || k >= ltrp::kNumKernels) return LTR_ERR_INVALID;
  if (k >= ltrp::kNumFast) {
    const int xc = k - ltrp::kNumFast;
    static const int kXW[kNumExact] = {kExactW, kXShortW, kXMidW, kXLongW, 0, 0};
    if (family) *family = ltrp::kFamExact;
    if (strip_width) *strip_width = kXW[xc];
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
  ModelConsts mc;
  mc.a = p->log_ins_to_ins; mc.b = p->log_ins_to_match; mc.c = p->log_del_to_del; mc.d = p->log_del_to_match;
  mc.e = p->log_match_to_match; mc.f = p->log_match_to_ins; mc.g = p->log_match_to_del;
  mc.match = mc.mismatch = mc.match_plus_f = 0.f;
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
  ModelConsts mc;
  mc.a = p->log_ins_to_ins; mc.b = p->log_ins_to_match; mc.c = p->log_del_to_del; mc.d = p->log_del_to_match;
  mc.e = p->log_match_to_match; mc.f = p->log_match_to_ins; mc.g = p->log_match_to_del;
  mc.match = mc.mismatch = mc.match_plus_f = 0.f;
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
  ModelConsts mc;
  mc.a = p->log_ins_to_ins; mc.b = p->log_ins_to_match; mc.c = p->log_del_to_del; mc.d = p->log_del_to_match;
  mc.e = p->log_match_to_match; mc.f = p->log_match_to_ins; mc.g = p->log_match_to_del;
  mc.match = mc.mismatch = mc.match_plus_f = 0.f;
  try {
    RawBuf<PairDesc> pairs, sorted; RawBuf<int16_t> key, bin; RawBuf<int32_t> order; RawBuf<uint8_t> read_acgt, hap_acgt;
    const ltrp::BatchScratch w{pairs, sorted, key, bin, order, read_acgt, hap_acgt};
    ltrp::BatchPlan d;
    std::string why;
    const int rc = ltrp::describe_batch(b, mc, p->indel_flank_len, mode, n_cu, ltr::DebugKnobs(), w, &d, &why);
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", why.c_str());
    if (rc != LTR_OK) return rc;
    if (out_i64) { out_i64[0] = d.n_pairs; out_i64[1] = d.ll_size; out_i64[2] = d.max_len; }
    if (out_f64) { out_f64[0] = d.cells; out_f64[1] = d.input_bytes; }
    if (class_first) for (int k = 0; k <= ltrp::kNumKernels; ++k) class_first[k] = d.bin_first[k];
    for (int64_t i = 0; i < std::min<int64_t>(pair_cap, d.n_pairs); ++i) {
      if (pair_n) pair_n[i] = sorted[(size_t)i].n;
      if (pair_m) pair_m[i] = sorted[(size_t)i].m;
      if (pair_out_idx) pair_out_idx[i] = sorted[(size_t)i].out_idx;
      if (pair_key) pair_key[i] = key[(size_t)order[(size_t)i]];
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
  ModelConsts mc;
  mc.a = p->log_ins_to_ins; mc.b = p->log_ins_to_match; mc.c = p->log_del_to_del; mc.d = p->log_del_to_match;
  mc.e = p->log_match_to_match; mc.f = p->log_match_to_ins; mc.g = p->log_match_to_del;
  mc.match = mc.mismatch = mc.match_plus_f = 0.f;
  try {
    RawBuf<PairDesc> pairs, sorted; RawBuf<int16_t> key, bin; RawBuf<int32_t> order; RawBuf<uint8_t> read_acgt, hap_acgt;
    const ltrp::BatchScratch w{pairs, sorted, key, bin, order, read_acgt, hap_acgt};
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
  ModelConsts mc;
  mc.a = p->log_ins_to_ins; mc.b = p->log_ins_to_match; mc.c = p->log_del_to_del; mc.d = p->log_del_to_match;
  mc.e = p->log_match_to_match; mc.f = p->log_match_to_ins; mc.g = p->log_match_to_del;
  mc.match = (float)(-0.000100005); mc.mismatch = (float)(-9.0); mc.match_plus_f = 0.f;     // (HapAligner.cpp:260-261; the bound U holds MATCH)
  try {
    RawBuf<PairDesc> pairs, sorted; RawBuf<int16_t> key, bin; RawBuf<int32_t> order; RawBuf<uint8_t> read_acgt, hap_acgt;
    const ltrp::BatchScratch w{pairs, sorted, key, bin, order, read_acgt, hap_acgt};
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
    for (int i = f0; i < f1 && i - f0 < member_cap; ++i) { member_n[i - f0] = sorted[(size_t)i].n; member_out[i - f0] = sorted[(size_t)i].out_idx; }
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}

}  // extern "C"
