// ltr_short.hip -- the SHORT (seeded, stutter-aware) alignment path on the GPU, SURVEY.md row a-7.
//
// Replaces, for period-1 loci under --stutter-align-len (reference HapAligner.cpp:552):
//   HapAligner::process_read, short_ branch           src/SeqAlignment/HapAligner.cpp:855-990 (retrace_aln = false)
//   HapAligner::align_seq_to_hap_short                HapAligner.cpp:27-163
//   HapAligner::compute_aln_logprob                   HapAligner.cpp:165-233
//   StutterAlignerClass::load_read / align_*_reverse  src/SeqAlignment/StutterAlignerClass.cpp:12-166
//   fast_log_sum_exp(vector) with fasterexp/fasterlog src/mathops.cpp:98-107, src/fastonebigheader.h:207-218,349-358
// The path is two units around ltr_short.h: ltr_short_batch.cpp (plain C++) is the host prep -- seeds, the batch with its
// offsets and tables, every libm value, and short_geometry, the rule that picks the launches; THIS file is the kernels and the
// stages that upload a batch, launch them and fetch the scores.  The device only adds, compares and runs the FP32 bit
// tricks on what the host formed like the reference forms it, so results are bit-identical to the CPU restatement.
//
// Mapping: prep kernel (per-read tables) -> flank kernels (one wavefront per (read, haplotype, side),
// rows skewed across lanes with wave_shr:1, strip width 2/4/8 per side) -> block kernel (four-wave workgroups, stutter tables
// in LDS, one (position, artifact) walk per lane) -> final kernel (compute_aln_logprob's log-sum over the seed positions).
// The reference's seed x max_hap matrices are never materialised: only each row's last column is kept, which is all
// compute_aln_logprob reads.  The round-2 lane-per-pair kernel stays behind ltr_ctx_set_debug("short_lane_kernel") and
// for sides wider than 512 bases.  This path is minor (homopolymer loci, ~5e4 cells per pair); see DESIGN.md.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ltr_internal.h"
#include "ltr_lease.h"
#include "ltr_short.h"

namespace {

using ltr::kImpS; using ltr::kMaxIns; using ltr::kMaxDel; using ltr::kNumArt;
using ltr::ShortHap; using ltr::ShortRead;

// What every kernel takes by value.  It stays in this unnamed namespace, not in ltr_short.h: the host unit never sees it, and a
// kernel's symbol spells its parameter's namespace.
struct ShortArgs {
  const ShortRead* reads; const ShortHap* fw; const ShortHap* rv;
  const uint8_t* read_bytes; const uint8_t* hap_bytes; const int32_t* upstream;
  const double* wrong; const double* correct;
  const double* cum;         // ShortRead::cum_off
  const double* art;         // [H][kNumArt] log_prob_pcr_artifact per combination
  const double* int_log;     // log(i)
  const int32_t* pair_read; const int32_t* pair_hap; const int64_t* pair_out;
  int32_t n_pairs, period;
  double* out;
  double* scratch;           // [block][elements][64]
  int64_t scratch_per_block; // doubles
  int32_t S, HS, LP;         // max side length, max haplotype size, log_probs_ capacity of this call
  int32_t n_ilog, maxB;      // entries of int_log; longest repeat block
  int32_t chunk_first, chunk_pairs;   // the pairs this set of launches scores
  double* g_row; double* g_last;      // per (pair of the chunk, side): S doubles (the row handed from launch to launch), HS + 2 doubles (last column of every row)
  double* g_terms;                    // ... and 13 x S doubles: the block row's terms by (artifact size, read position)
  float a, b, c, d, e, f, g;
  double log_thresh;         // log(0.001), mathops.h:36
  // ltr_short_prep_kernel: base qualities -> wrong / correct / cum, on the device
  const uint8_t* qidx;       // per base (ShortRead::q_off, the order of wrong / correct): BaseQuality's table index
  const double* qtab;        // [0, 64): log_error_ by index, [64, 128): log_correct_ (base_quality.h:29-43), from the host's libm
  double* wrong_w; double* correct_w; double* cum_w;
  int32_t n_reads;
};

template <bool V> struct BoolTagS { static constexpr bool value = V; };
__device__ __forceinline__ double dmx(double x, double y) { return x < y ? y : x; }   // std::max
// fastonebigheader.h:207-218
__device__ __forceinline__ float d_fasterexp(float p) {
  p = 1.442695040f * p;
  const float clipp = (p < -126) ? -126.0f : p;
  const uint32_t i = (uint32_t)((1 << 23) * (clipp + 126.94269504f));
  return __uint_as_float(i);
}
// fastonebigheader.h:349-358
__device__ __forceinline__ float d_fasterlog(float x) {
  float y = (float)__float_as_uint(x);
  y *= 8.2629582881927490e-8f;
  return y - 87.989971088f;
}

#define LN(buf, idx) (buf)[(size_t)(idx) * 64 + lane]

// fast_log_sum_exp over lane-private values v[0..n), mathops.cpp:98-107
__device__ __forceinline__ double d_flse(const double* v, int n, int lane, double log_thresh) {
  double mx = LN(v, 0);
  for (int i = 1; i < n; i++) { const double x = LN(v, i); if (mx < x) mx = x; }
  double total = 0;
  for (int i = 0; i < n; i++) { const double diff = LN(v, i) - mx; if (diff > log_thresh) total += d_fasterexp((float)diff); }
  return mx + d_fasterlog((float)total);
}

struct Side {                // per-lane view of one alignment side
  const uint8_t* seq; int seq_len; const double* wrong; const double* correct;
  const uint8_t* hap; int len0, len1, len2; const int32_t* up; int num_del;
};

// align_seq_to_hap_short (HapAligner.cpp:27-163) with rolling rows; lastM[row] = M[row][seq_len-1].
// Returns left_prob (the sum of base_log_correct over the side, :42).
__device__ double short_side(const ShortArgs& A, const Side& sd, const double* art, double* W, int lane, double* lastM) {
  const int S = A.S;
  double* Mp = W;               double* Ip = W + (size_t)S * 64;        double* Dp = W + (size_t)2 * S * 64;
  double* Mc = W + (size_t)3 * S * 64; double* Ic = W + (size_t)4 * S * 64; double* Dc = W + (size_t)5 * S * 64;
  double* insP = W + (size_t)6 * S * 64;          // [seq_len * 6]
  double* delP = W + (size_t)12 * S * 64;         // [seq_len * num_del]
  double* matP = W + (size_t)18 * S * 64;         // [seq_len]
  double* lp = W + (size_t)19 * S * 64;           // log_probs_ scratch, A.LP elements
  const int seq_len = sd.seq_len;
  const uint8_t* seq = sd.seq; const double* wrong = sd.wrong; const double* correct = sd.correct;
  const double ca = A.a, cb = A.b, cc = A.c, cd = A.d, ce = A.e, cf = A.f, cg = A.g;
  const int period = A.period;

  double left_prob = 0.0;
  const uint8_t first_hap_base = sd.hap[0];
  for (int j = 0; j < seq_len; ++j) {                                  // :36-44
    LN(Mp, j) = (seq[j] == first_hap_base ? correct[j] : wrong[j]) + left_prob;
    LN(Ip, j) = correct[j] + left_prob;
    LN(Dp, j) = kImpS;
    left_prob += correct[j];
  }
  LN(lastM, 0) = LN(Mp, seq_len - 1);
  int hap_index = 1, stutter_R = -1;
  const int blen[3] = {sd.len0, sd.len1, sd.len2};
  int boff = 0;
  for (int bi = 0; bi < 3; bi++) {
    const uint8_t* bseq = sd.hap + boff;
    const int block_len = blen[bi];
    boff += block_len;
    if (bi == 1) {                                                     // stutter block, :64-111
      const int max_ins = kMaxIns * period, num_del = sd.num_del, max_del = -period * num_del;
      const uint8_t* blk = bseq + (block_len - 1);                     // block_seq_ points at the LAST base
      // ---- StutterAlignerClass::load_read(seq_len, seq_0+seq_len-1, ...), StutterAlignerClass.cpp:12-53
      {
        const uint8_t* bs = seq + (seq_len - 1); const double* bw = wrong + (seq_len - 1); const double* bc = correct + (seq_len - 1);
        int ins_index = 0, del_index = 0;
        for (int i = 0; i < seq_len; i++) {
          int j; double log_prob = 0.0;
          for (j = 0; j < min(seq_len - i, -max_del); j++) {
            log_prob += (bs[-i - j] == blk[-j] ? bc[-i - j] : bw[-i - j]);
            if ((j + 1) % period == 0) { LN(delP, del_index) = log_prob; del_index++; }
          }
          for (; j < -max_del; j++) if ((j + 1) % period == 0) del_index++;
          for (; j < min(seq_len - i, block_len); j++) log_prob += (bs[-i - j] == blk[-j] ? bc[-i - j] : bw[-i - j]);
          LN(matP, i) = log_prob;
          double log_ins_prob = 0.0;
          for (j = 0; j < min(max_ins, seq_len - i); j++) {
            if (j % period < block_len) log_ins_prob += (bs[-i - j] == blk[-(j % period)] ? bc[-i - j] : bw[-i - j]);
            else log_ins_prob += bc[-i - j];
            if ((j + 1) % period == 0) { LN(insP, ins_index) = log_ins_prob; ins_index++; }
          }
          for (; j < max_ins; j++) if ((j + 1) % period == 0) { LN(insP, ins_index) = log_ins_prob; ins_index++; }
        }
      }
      // Mp currently holds the row before the block (prev_row_index); the block's last row goes to Mc
      int offset = seq_len - 1;
      for (int j = 0; j < seq_len; ++j, --offset) {
        double bp[kNumArt];
        int art_idx = 0;
        for (int asz = -kMaxDel * period; asz <= max_ins; asz += period, ++art_idx) {
          const int base_len = min(block_len + asz, j + 1);
          if (base_len < 0) { bp[art_idx] = kImpS; continue; }
          const uint8_t* bs = seq + j; const double* bw = wrong + j; const double* bc = correct + j;
          double prob;
          if (asz == 0) prob = LN(matP, offset);                       // align_no_artifact_reverse, :55-57
          else if (asz > 0) {                                          // align_pcr_insertion_reverse, :59-104
            const int D = asz; int np = 0;
            const int32_t* up = sd.up + (block_len - 1);               // upstream_match_lengths_[0]
            double log_prob = -A.int_log[block_len + 1] + LN(insP, kMaxIns * offset + D / period - 1) +
                              (base_len > D ? LN(matP, offset + D) : 0);
            LN(lp, np) = log_prob; np++;
            int i = 0;
            for (; i > -min(max(0, base_len - D), block_len); i--) {
              if (-i + period < block_len) {
                if (up[i] == 0) {
                  for (int index = i - period; index >= i - D; index -= period) {
                    log_prob -= (bs[index] == blk[i] ? bc[index] : bw[index]);
                    log_prob += (bs[index] == blk[i - period] ? bc[index] : bw[index]);
                  }
                  LN(lp, np) = log_prob; np++;
                } else {
                  LN(lp, np) = A.int_log[up[i]] + log_prob; np++;
                  i -= (up[i] - 1);
                }
              } else { LN(lp, np) = log_prob; np++; }
            }
            if (i > -block_len) { LN(lp, np) = A.int_log[block_len + i] + log_prob; np++; }
            prob = d_flse(lp, np, lane, A.log_thresh);
          } else {                                                     // align_pcr_deletion_reverse, :106-154
            const int D = asz; int np = 0;
            const int32_t* up = sd.up + (size_t)(-D / period - 1) * block_len + (block_len - 1);
            double log_prob = -A.int_log[block_len + D + 1];
            if (offset + D >= 0) log_prob += LN(matP, offset + D) - LN(delP, (offset + D) * num_del - D / period - 1);
            else for (int jj = 0; jj > -base_len; jj--) log_prob += (blk[jj + D] == bs[jj] ? bc[jj] : bw[jj]);
            LN(lp, np) = log_prob; np++;
            int i;
            for (i = 0; i > -base_len; i--) {
              if (up[i] == 0) {
                log_prob -= (blk[i + D] == bs[i] ? bc[i] : bw[i]);
                log_prob += (blk[i] == bs[i] ? bc[i] : bw[i]);
                LN(lp, np) = log_prob; np++;
              } else {
                LN(lp, np) = A.int_log[up[i]] + log_prob; np++;
                i -= (up[i] - 1);
              }
            }
            if (-i < block_len + D) { LN(lp, np) = A.int_log[block_len + D + i] + log_prob; np++; }
            prob = d_flse(lp, np, lane, A.log_thresh);
          }
          // An EMPTY block's row is the row before it (:72-73: matrix_index == prev_row_index): the reference fills it in place, so an
          // insertion (base_len > 0) reads the block-row values of the positions before j, not the flank row's
          const double* Pv = (block_len == 0 && base_len > 0) ? Mc : Mp;
          const double pre_prob = (j - base_len < 0 ? 0 : LN(Pv, j - base_len));
          bp[art_idx] = art[art_idx] + prob + pre_prob;                // :91
        }
        // fast_log_sum_exp(block_probs), :103
        double mx = bp[0];
        for (int q = 1; q < kNumArt; q++) if (mx < bp[q]) mx = bp[q];
        double total = 0;
        for (int q = 0; q < kNumArt; q++) { const double diff = bp[q] - mx; if (diff > A.log_thresh) total += d_fasterexp((float)diff); }
        LN(Mc, j) = mx + d_fasterlog((float)total);
        LN(Ic, j) = kImpS; LN(Dc, j) = kImpS;
      }
      stutter_R = hap_index + block_len - 1;
      hap_index += block_len;
      LN(lastM, stutter_R) = LN(Mc, seq_len - 1);
      double* t;
      t = Mp; Mp = Mc; Mc = t; t = Ip; Ip = Ic; Ic = t; t = Dp; Dp = Dc; Dc = t;
    } else {                                                           // flank block, :112-159
      for (int coord = (bi == 0 ? 1 : 0); coord < block_len; ++coord, ++hap_index) {
        const uint8_t hap_char = bseq[coord];
        const bool after = (hap_index == stutter_R + 1);
        LN(Mc, 0) = (seq[0] == hap_char ? correct[0] : wrong[0]);
        LN(Ic, 0) = after ? kImpS : correct[0];
        LN(Dc, 0) = after ? kImpS : dmx(LN(Dp, 0) + cc, LN(Mp, 0) + cd);
        if (after) {                                                   // a stutter block must be followed by a match, :132-141
          for (int j = 1; j < seq_len; ++j) {
            const double emit = (seq[j] == hap_char ? correct[j] : wrong[j]);
            LN(Mc, j) = emit + LN(Mp, j - 1);
            LN(Ic, j) = kImpS; LN(Dc, j) = kImpS;
          }
        } else {
          double Mdiag = LN(Mp, 0), Ddiag = LN(Dp, 0), Ileft = LN(Ic, 0);
          for (int j = 1; j < seq_len; ++j) {
            const double Mup = LN(Mp, j), Dup = LN(Dp, j);
            const double p0 = Ileft + cf, p1 = Mdiag + ce, p2 = Ddiag + cg;
            const double emit = (seq[j] == hap_char ? correct[j] : wrong[j]);
            const double Mn = emit + dmx(p0, dmx(p1, p2));
            const double In = correct[j] + dmx(Mdiag + cb, Ileft + ca);
            const double Dn = dmx(Mup + cd, Dup + cc);
            LN(Mc, j) = Mn; LN(Ic, j) = In; LN(Dc, j) = Dn;
            Mdiag = Mup; Ddiag = Dup; Ileft = In;
          }
        }
        LN(lastM, hap_index) = LN(Mc, seq_len - 1);
        double* t;
        t = Mp; Mp = Mc; Mc = t; t = Ip; Ip = Ic; Ic = t; t = Dp; Dp = Dc; Dc = t;
      }
    }
  }
  return left_prob;
}

__global__ __launch_bounds__(64) void ltr_short_kernel(ShortArgs A) {
  const int lane = threadIdx.x;
  double* base = A.scratch + (size_t)blockIdx.x * A.scratch_per_block;
  double* W = base;                                        // 19*S work elements + LP log_probs_ elements, x 64
  double* lastL = base + (size_t)(19 * A.S + A.LP) * 64;
  double* lastR = lastL + (size_t)(A.HS + 2) * 64;
  for (int p = blockIdx.x * 64 + lane; p < A.n_pairs; p += gridDim.x * 64) {
    const ShortRead rd = A.reads[A.pair_read[p]];
    const int k = A.pair_hap[p];
    const ShortHap hf = A.fw[k], hr = A.rv[k];
    const double* art = A.art + (size_t)k * kNumArt;
    const int seed = rd.seed, len = rd.len, rlen = len - seed - 1;
    Side L, R;
    L.seq = A.read_bytes + rd.seq_off; L.seq_len = seed; L.wrong = A.wrong + rd.q_off; L.correct = A.correct + rd.q_off;
    L.hap = A.hap_bytes + hf.seq_off; L.len0 = hf.len[0]; L.len1 = hf.len[1]; L.len2 = hf.len[2];
    L.up = A.upstream + hf.up_off; L.num_del = hf.num_deletions;
    R.seq = A.read_bytes + rd.rev_off; R.seq_len = rlen; R.wrong = A.wrong + rd.q_off + seed + 1; R.correct = A.correct + rd.q_off + seed + 1;
    R.hap = A.hap_bytes + hr.seq_off; R.len0 = hr.len[0]; R.len1 = hr.len[1]; R.len2 = hr.len[2];
    R.up = A.upstream + hr.up_off; R.num_del = hr.num_deletions;
    const double l_prob = short_side(A, L, art, W, lane, lastL);       // :905
    const double r_prob = short_side(A, R, art, W, lane, lastR);       // :908
    // ---- compute_aln_logprob, HapAligner.cpp:165-233 ----
    const int hapsize = hf.len[0] + hf.len[1] + hf.len[2];
    const uint8_t* hs = A.hap_bytes + hf.seq_off;
    const uint8_t seed_char = (A.read_bytes + rd.seq_off)[seed];
    const double sw = A.wrong[rd.q_off + seed], sc = A.correct[rd.q_off + seed];
    const double PRIOR = -A.int_log[hf.len[0] + hf.len[2]];             // num_seeds = non-stutter bases, :175-179
    double* lp = W + (size_t)19 * A.S * 64;
    int np = 0;
    LN(lp, np) = PRIOR + (seed_char == hs[0] ? sc : sw) + l_prob + LN(lastR, hapsize - 2); np++;               // :184-185
    LN(lp, np) = PRIOR + (seed_char == hs[hapsize - 1] ? sc : sw) + r_prob + LN(lastL, hapsize - 2); np++;     // :190-191
    int lrow = 0, rrow = hapsize - 3, coord_abs = 0;
    for (int b = 0; b < 3; ++b) {
      const int bl = hf.len[b];
      if (b == 1) { lrow += bl; rrow -= bl; coord_abs += bl; continue; }
      const int c0 = (b == 0 ? 1 : 0), c1 = (b == 2 ? bl - 1 : bl);
      for (int cidx = c0; cidx < c1; ++cidx) {
        LN(lp, np) = PRIOR + (seed_char == hs[coord_abs + cidx] ? sc : sw) + LN(lastL, lrow) + LN(lastR, rrow); np++;   // :220
        lrow++; rrow--;
      }
      coord_abs += bl;
    }
    A.out[A.pair_out[p]] = d_flse(lp, np, lane, A.log_thresh);         // :230
  }
}


// =============================================================================================================
// The seeded path as THREE kinds of work, each with the mapping that suits it (five launches per set of pairs: 0. the reads'
// quality tables and prefix sums, ltr_short_prep_kernel, then 1. - 4.):
//
//  1. flank rows before the stutter block (HapAligner.cpp:112-159) -- ltr_short_flank_kernel<false>: one wavefront
//     per (pair, side).  A Viterbi recurrence with base-quality emissions whose only same-row dependency is the insertion
//     chain I(i,j-1) -> I(i,j): lane l owns W consecutive read positions and the haplotype rows stream through the lanes
//     skewed by one row per lane -- the K1 geometry of ltr_dp_kernel.hpp -- with the three values a lane needs from its
//     left neighbour (I of the same row, M and D of the row before) handed over by DPP wave_shr:1.  The previous row
//     lives in registers (2 W doubles); nothing per cell touches memory.  Out: the row before the block (one double per
//     read position) and the last column of every row.
//  2. the stutter-block row (:64-111) -- ltr_short_block_kernel: one workgroup of four wavefronts per (pair, side).
//     load_read's match table (StutterAlignerClass.cpp:12-53), one read position per thread, in LDS; then per read
//     position the log-sum over 13 artifact sizes of pmf + stutter-aligner LL + the match value `base_len` positions back
//     in the row before the block.  Every (position, size) term is independent: a row of 16 lanes takes one position,
//     lane a of the row the term of artifact size a -- the reference's walk over the block (.cpp:59-154) run twice, once
//     for the maximum and once for the sum, instead of keeping its log_probs_ list, with load_read's deletion / insertion
//     tables re-summed where they are used (same terms, same order) -- and the row's log-sum is a 16-lane reduction.
//     Block bases, upstream-match tables and integer logs come from LDS: a walk is a chain of dependent look-ups.
//  3. flank rows after the block -- ltr_short_flank_kernel<true>: as 1., starting from the block row; its first row
//     must follow the block with a match (:132-141).
//  4. compute_aln_logprob (:165-233) -- ltr_short_final_kernel: one wavefront per pair, one seed position per lane.
//
// fast_log_sum_exp (mathops.cpp:98-107) adds floats of (0.001, 1.06] into a double -- 24-bit values whose exponents
// span 11 binades: up to half a million of them add EXACTLY, so the order of the sum does not matter and the log-sums of
// 2. and 4. are lane reductions.  The FP operation order of every value the reference rounds is untouched: bit-identical
// to the lane-per-pair kernel above (and to the restatement, whose stutter-block rows are pinned to the compiled reference).
// Between the launches a (pair, side) keeps 8 bytes per read position and per haplotype row in HBM (written once, read
// once); no per-cell traffic anywhere.
// =============================================================================================================
__device__ __forceinline__ double w_shr1(double v) {          // lane l <- lane l-1 (lane 0: 0)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double w_max(double v, const int width) {     // maximum over aligned groups of `width` lanes
  for (int o = width >> 1; o > 0; o >>= 1) { const double x = __shfl_xor(v, o); v = v < x ? x : v; }
  return v;
}
__device__ __forceinline__ double w_sum(double v, const int width) {     // sum over aligned groups of `width` lanes (callers: exact sums only)
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
constexpr int kShortThreads = 256;

// (pair, side) -> the side's view of the read and of the haplotype
__device__ __forceinline__ void pair_side(const ShortArgs& A, const int p, const int side, Side* sd, const double** cum) {
  const ShortRead rd = A.reads[A.pair_read[p]];
  const int k = A.pair_hap[p];
  const int seed = rd.seed;
  if (side == 0) {
    const ShortHap hf = A.fw[k];
    sd->seq = A.read_bytes + rd.seq_off; sd->seq_len = seed; sd->wrong = A.wrong + rd.q_off; sd->correct = A.correct + rd.q_off;
    sd->hap = A.hap_bytes + hf.seq_off; sd->len0 = hf.len[0]; sd->len1 = hf.len[1]; sd->len2 = hf.len[2];
    sd->up = A.upstream + hf.up_off; sd->num_del = hf.num_deletions;
    *cum = A.cum + rd.cum_off;
  } else {
    const ShortHap hr = A.rv[k];
    sd->seq = A.read_bytes + rd.rev_off; sd->seq_len = rd.len - seed - 1; sd->wrong = A.wrong + rd.q_off + seed + 1; sd->correct = A.correct + rd.q_off + seed + 1;
    sd->hap = A.hap_bytes + hr.seq_off; sd->len0 = hr.len[0]; sd->len1 = hr.len[1]; sd->len2 = hr.len[2];
    sd->up = A.upstream + hr.up_off; sd->num_del = hr.num_deletions;
    *cum = A.cum + rd.cum_off + seed + 1;
  }
}

// 0.: one wavefront per read: BaseQuality's log tables looked up per base (base_quality.h:53-75), and left_prob of
// align_seq_to_hap_short's first row (HapAligner.cpp:36-44: left_prob += base_log_correct[j], base by base) for both
// sides -- it depends on the read alone, so it is summed once here, in the reference's order (one lane per side), not
// once per haplotype.  The host sends one byte per base instead of three doubles.
__global__ __launch_bounds__(kShortThreads) void ltr_short_prep_kernel(ShortArgs A) {
  const int lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * (kShortThreads / 64) + (int)(threadIdx.x >> 6);
  if (r >= A.n_reads) return;
  const ShortRead rd = A.reads[r];
  const uint8_t* q = A.qidx + rd.q_off;
  for (int j = lane; j < rd.len; j += 64) { const int k = q[j]; A.wrong_w[rd.q_off + j] = A.qtab[k]; A.correct_w[rd.q_off + j] = A.qtab[64 + k]; }
  if (lane < 2) {
    const int j0 = lane == 0 ? 0 : rd.seed + 1, j1 = lane == 0 ? rd.seed : rd.len;
    double* cum = A.cum_w + rd.cum_off + j0;
    double acc = 0.0;
    for (int j = j0; j < j1; j++) { *cum++ = acc; acc += A.qtab[64 + q[j]]; }
    *cum = acc;
  }
}

// 1. / 3.: one wavefront per (pair, side).  g_row: the row handed from launch to launch (the row before the block, then
// the block's row); g_last: M[row][seq_len - 1] of every haplotype row.
template <int W, bool SECOND>
__device__ __forceinline__ void short_flank_rows(const ShortArgs& A, const Side& sd, const double* cum, double* g_row, double* last, const int lane) {
  const int S = sd.seq_len;
  const double ca = A.a, cb = A.b, cc = A.c, cd = A.d, ce = A.e, cf = A.f, cg = A.g;
  const int nl = (S + W - 1) / W;                              // lanes that own read positions
  const int j0 = lane * W;
  const int own_last = (S - 1) - (nl - 1) * W;                 // slot of the last read position, in lane nl - 1
  double Mp[W], Dp[W], cw[W], ww[W];
  uint32_t sq[W];
  const int block_len = sd.len1;
#pragma unroll
  for (int s = 0; s < W; ++s) {
    const int j = min(j0 + s, S - 1);                          // (slack positions: clamped loads, values nobody reads)
    cw[s] = sd.correct[j]; ww[s] = sd.wrong[j]; sq[s] = sd.seq[j];
    Dp[s] = kImpS;
    if (SECOND) Mp[s] = g_row[j];                              // the block's row; I = D = IMPOSSIBLE there (:104-105)
    else {
      const double lp = cum[j];                                // left_prob before base j, :36-44
      Mp[s] = (sq[s] == (uint32_t)sd.hap[0] ? cw[s] : ww[s]) + lp;
    }
  }
  if (!SECOND && lane == nl - 1) {
#pragma unroll
    for (int s = 0; s < W; ++s) if (s == own_last) last[0] = Mp[s];
  }
  // what my right neighbour takes from me at its next step: I of my last position in the row I have just finished, M and
  // D of that position in the row before (to begin with: row 0, or the block's row)
  double pubI = 0.0, pubM2 = Mp[W - 1], pubD2 = Dp[W - 1];
  const uint8_t* hap_chars = SECOND ? sd.hap + sd.len0 + block_len : sd.hap + 1;
  const int nrows = SECOND ? sd.len2 : sd.len0 - 1;
  const int hap_row0 = SECOND ? sd.len0 + block_len : 1;
  const int T = nrows > 0 ? nrows + nl - 1 : 0;
  for (int t = 0; t < T; ++t) {
    const double nI = w_shr1(pubI), nM = w_shr1(pubM2), nD = w_shr1(pubD2);
    const int r = t - lane;
    const bool active = (r >= 0) & (r < nrows) & (lane < nl);
    if (active) {
      const uint32_t hap_char = hap_chars[r];
      const bool after = SECOND && r == 0;                     // a stutter block must be followed by a match, :132-141
      double Mdiag = nM, Ddiag = nD, Ileft = nI;
      const double keepM = Mp[W - 1], keepD = Dp[W - 1];
#pragma unroll
      for (int s = 0; s < W; ++s) {
        const double Mup = Mp[s], Dup = Dp[s];
        const double emit = (sq[s] == hap_char ? cw[s] : ww[s]);
        const double p0 = Ileft + cf, p1 = Mdiag + ce, p2 = Ddiag + cg;
        double Mn = emit + dmx(p0, dmx(p1, p2));
        double In = cw[s] + dmx(Mdiag + cb, Ileft + ca);
        double Dn = dmx(Mup + cd, Dup + cc);
        if (SECOND) { if (after) { Mn = emit + Mdiag; In = kImpS; Dn = kImpS; } }
        if (s == 0) {                                          // the read's first base, :124-129
          if (lane == 0) { Mn = emit; In = after ? kImpS : cw[0]; Dn = after ? kImpS : dmx(Dup + cc, Mup + cd); }
        }
        Mdiag = Mup; Ddiag = Dup; Ileft = In;
        Mp[s] = Mn; Dp[s] = Dn;
      }
      pubI = Ileft; pubM2 = keepM; pubD2 = keepD;
      if (lane == nl - 1) {
#pragma unroll
        for (int s = 0; s < W; ++s) if (s == own_last) last[hap_row0 + r] = Mp[s];
      }
    }
  }
  if (!SECOND) {
#pragma unroll
    for (int s = 0; s < W; ++s) if (j0 + s < S) g_row[j0 + s] = Mp[s];       // the row before the block
  }
}

// The strip width is picked per (pair, side), wave-uniformly: the narrowest of 2 / 4 / 8 read positions per lane that covers
// the side with 64 lanes -- a flank is ~35 haplotype rows, so a side of 230 positions on 8-wide strips would run 63 steps on
// 29 lanes, on 4-wide strips 91 steps of half the work on 58.  (Registers: those of the widest body.)
template <bool SECOND>
__global__ __launch_bounds__(kShortThreads) void ltr_short_flank_kernel(ShortArgs A) {
  const int lane = threadIdx.x & 63;
  const int ps = (int)blockIdx.x * (kShortThreads / 64) + (int)(threadIdx.x >> 6);     // (pair, side) of my wavefront
  if (ps >= 2 * A.chunk_pairs) return;
  const int p = A.chunk_first + (ps >> 1), side = ps & 1;
  Side sd; const double* cum;
  pair_side(A, p, side, &sd, &cum);
  double* g_row = A.g_row + (size_t)ps * A.S;
  double* last = A.g_last + (size_t)ps * (A.HS + 2);
  const int S = __builtin_amdgcn_readfirstlane(sd.seq_len);
  if (S <= 64 * 2) short_flank_rows<2, SECOND>(A, sd, cum, g_row, last, lane);
  else if (S <= 64 * 4) short_flank_rows<4, SECOND>(A, sd, cum, g_row, last, lane);
  else short_flank_rows<8, SECOND>(A, sd, cum, g_row, last, lane);
}

// 2.: one workgroup per (pair, side): g_row (the row before the block) -> g_row (the block's row); last[stutter_R].
// (eight wavefronts a SIMD: a walk is a chain of dependent LDS look-ups, other wavefronts are what hides their latency)
// (the repeat period as a compile-time 1 -- the only period HapAligner.cpp:552 sends down this path -- was measured: no gain,
// the walks themselves are the instructions: ~900 per (position, artifact size), VALU issue 0.92 - 0.97 by the PMC pass)
__global__ __launch_bounds__(kShortThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void ltr_short_block_kernel(ShortArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_raw[];
  const int tid = threadIdx.x;
  double* s_cor = (double*)s_raw; double* s_wr = s_cor + A.S; double* s_matP = s_wr + A.S; double* s_prev = s_matP + A.S;
  double* s_ilog = s_prev + A.S;
  int32_t* s_up = (int32_t*)(s_ilog + A.n_ilog);
  uint8_t* s_seq = (uint8_t*)(s_up + (size_t)kMaxDel * A.maxB + 8); uint8_t* s_hap = s_seq + ((A.S + 7) & ~7);
  for (int i = tid; i < A.n_ilog; i += kShortThreads) s_ilog[i] = A.int_log[i];
  const int period = A.period;
  for (int ps = blockIdx.x; ps < 2 * A.chunk_pairs; ps += gridDim.x) {
    const int p = A.chunk_first + (ps >> 1), side = ps & 1;
    Side sd; const double* cum;
    pair_side(A, p, side, &sd, &cum);
    const double* art = A.art + (size_t)A.pair_hap[p] * kNumArt;
    double* g_row = A.g_row + (size_t)ps * A.S;
    const int S = sd.seq_len, block_len = sd.len1, num_del = sd.num_del;
    const int max_del = -period * num_del;
    // An EMPTY block's row is the row before it (HapAligner.cpp:72-73: matrix_index == prev_row_index) and the reference fills it in
    // place, left to right: an insertion's pre_prob (:90, base_len > 0) is the BLOCK row's value base_len positions back.  Then the
    // row is a recurrence over the read positions: the terms without pre_prob in parallel, the row itself by one thread.
    const bool in_place = block_len == 0;
    __syncthreads();                                           // (the previous (pair, side)'s readers are done with the LDS arrays)
    for (int j = tid; j < S; j += kShortThreads) { s_seq[j] = sd.seq[j]; s_cor[j] = sd.correct[j]; s_wr[j] = sd.wrong[j]; s_prev[j] = g_row[j]; }
    {
      const int hs = sd.len0 + sd.len1 + sd.len2, nup = max(num_del, 1) * block_len;
      for (int j = tid; j < hs; j += kShortThreads) s_hap[j] = sd.hap[j];
      for (int j = tid; j < nup; j += kShortThreads) s_up[j] = sd.up[j];
    }
    __syncthreads();
    const uint8_t* seq = s_seq; const double* correct = s_cor; const double* wrong = s_wr;
    const uint8_t* blk = s_hap + sd.len0 + (block_len - 1);     // block_seq_ points at the LAST base of the block
    const uint8_t* bsE = seq + (S - 1); const double* bwE = wrong + (S - 1); const double* bcE = correct + (S - 1);   // ... like the read's arrays
    // ---- StutterAlignerClass::load_read (StutterAlignerClass.cpp:12-53): the match table, one read position per thread ----
    for (int i = tid; i < S; i += kShortThreads) {
      double log_prob = 0.0;
      const int n = min(S - i, block_len);
      for (int j = 0; j < n; j++) log_prob += (bsE[-i - j] == blk[-j] ? bcE[-i - j] : bwE[-i - j]);
      s_matP[i] = log_prob;
    }
    // del_probs_[i * num_deletions_ + q]: the match sum of read position i over the first (q + 1) * period block bases (:34-38)
    auto del_sum = [&](const int i, const int q) __attribute__((always_inline)) {
      double log_prob = 0.0;
      const int n = min(min(S - i, -max_del), (q + 1) * period);
      for (int j = 0; j < n; j++) log_prob += (bsE[-i - j] == blk[-j] ? bcE[-i - j] : bwE[-i - j]);
      return log_prob;
    };
    // ins_probs_[i * num_insertions_ + q]: (q + 1) * period inserted bases copied from the block's last repeat unit (:43-52)
    auto ins_sum = [&](const int i, const int q) __attribute__((always_inline)) {
      double log_ins_prob = 0.0;
      const int n = min(min(kMaxIns * period, S - i), (q + 1) * period);
      for (int j = 0; j < n; j++) {
        if (j % period < block_len) log_ins_prob += (bsE[-i - j] == blk[-(j % period)] ? bcE[-i - j] : bwE[-i - j]);
        else log_ins_prob += bcE[-i - j];
      }
      return log_ins_prob;
    };
    __syncthreads();
    const int32_t* up_base = s_up;                             // [max(num_del, 1)][block_len]
    const double* ilog = s_ilog;
    // VISIT(v): what fast_log_sum_exp does with one entry of the reference's log_probs_ list -- pass 0 its maximum, pass 1 its sum
#define LTR_VISIT(v) do { const double v_ = (v); if (pass == 0) { if (mx < v_) mx = v_; } else { const double diff_ = v_ - mx; if (diff_ > A.log_thresh) total += d_fasterexp((float)diff_); } } while (0)
    // item = (artifact size, read position), size-major: the lanes of a wavefront walk the same kind of artifact
    double* terms = A.g_terms + (size_t)ps * kNumArt * A.S;
    for (int item = tid; item < kNumArt * S; item += kShortThreads) {
      const int ai = item / S, j = item - ai * S;              // artifact size (ai - 6) * period at read position j
      double term;
      {
        const int asz = (ai - kMaxDel) * period;
        const int base_len = min(block_len + asz, j + 1);
        term = kImpS;
        if (base_len >= 0) {
          const int offset = S - 1 - j;
          const uint8_t* bs = seq + j; const double* bw = wrong + j; const double* bc = correct + j;
          double prob;
          if (asz == 0) prob = s_matP[offset];                 // align_no_artifact_reverse, :55-57
          else if (asz > 0) {                                  // align_pcr_insertion_reverse, :59-104
            const int D = asz;
            const int32_t* up0 = up_base + (block_len - 1);    // upstream_match_lengths_[0]
            const double first = -ilog[block_len + 1] + ins_sum(offset, D / period - 1) + (base_len > D ? s_matP[offset + D] : 0);
            double mx = first, total = 0;
            for (int pass = 0; pass < 2; ++pass) {
              double log_prob = first;
              LTR_VISIT(log_prob);
              int i = 0;
              for (; i > -min(max(0, base_len - D), block_len); i--) {
                if (-i + period < block_len) {
                  const int u = up0[i];
                  if (u == 0) {
                    for (int index = i - period; index >= i - D; index -= period) {
                      log_prob -= (bs[index] == blk[i] ? bc[index] : bw[index]);
                      log_prob += (bs[index] == blk[i - period] ? bc[index] : bw[index]);
                    }
                    LTR_VISIT(log_prob);
                  } else {
                    LTR_VISIT(ilog[u] + log_prob);
                    i -= (u - 1);
                  }
                } else LTR_VISIT(log_prob);
              }
              if (i > -block_len) LTR_VISIT(ilog[block_len + i] + log_prob);
            }
            prob = mx + d_fasterlog((float)total);             // fast_log_sum_exp(log_probs_)
          } else {                                             // align_pcr_deletion_reverse, :106-154
            const int D = asz;
            const int32_t* up = up_base + (size_t)(-D / period - 1) * block_len + (block_len - 1);
            double first = -ilog[block_len + D + 1];
            if (offset + D >= 0) first += s_matP[offset + D] - del_sum(offset + D, -D / period - 1);
            else for (int jj = 0; jj > -base_len; jj--) first += (blk[jj + D] == bs[jj] ? bc[jj] : bw[jj]);
            double mx = first, total = 0;
            for (int pass = 0; pass < 2; ++pass) {
              double log_prob = first;
              LTR_VISIT(log_prob);
              int i;
              for (i = 0; i > -base_len; i--) {
                const int u = up[i];
                if (u == 0) {
                  log_prob -= (blk[i + D] == bs[i] ? bc[i] : bw[i]);
                  log_prob += (blk[i] == bs[i] ? bc[i] : bw[i]);
                  LTR_VISIT(log_prob);
                } else {
                  LTR_VISIT(ilog[u] + log_prob);
                  i -= (u - 1);
                }
              }
              if (-i < block_len + D) LTR_VISIT(ilog[block_len + D + i] + log_prob);
            }
            prob = mx + d_fasterlog((float)total);
          }
          const double pre_prob = (j - base_len < 0 ? 0 : s_prev[j - base_len]);
          term = in_place && base_len > 0 ? art[ai] + prob : art[ai] + prob + pre_prob;       // :91 (in place: pre_prob joins below)
        }
      }
      terms[item] = term;
    }
    __syncthreads();                                           // (workgroup scope: orders the global stores above, too)
    if (in_place) {
      if (tid == 0) {
        for (int j = 0; j < S; ++j) {
          double bp[kNumArt];
#pragma unroll
          for (int a = 0; a < kNumArt; ++a) {
            const int base_len = min((a - kMaxDel) * period, j + 1);
            bp[a] = terms[(size_t)a * S + j];
            if (base_len > 0) bp[a] += (j - base_len < 0 ? 0 : s_prev[j - base_len]);       // (positions before j: already the block's row)
          }
          double mx = bp[0];
#pragma unroll
          for (int a = 1; a < kNumArt; ++a) if (mx < bp[a]) mx = bp[a];
          double total = 0;
#pragma unroll
          for (int a = 0; a < kNumArt; ++a) { const double diff = bp[a] - mx; if (diff > A.log_thresh) total += d_fasterexp((float)diff); }
          const double v = mx + d_fasterlog((float)total);
          s_prev[j] = v; g_row[j] = v;
          if (j == S - 1) A.g_last[(size_t)ps * (A.HS + 2) + (sd.len0 - 1)] = v;                // last[stutter_R], stutter_R = len0 - 1
        }
      }
      continue;                                                // (the loop's first __syncthreads separates s_prev's next writers)
    }
    for (int j = tid; j < S; j += kShortThreads) {             // fast_log_sum_exp(block_probs), :103
      double mx = terms[j];
#pragma unroll
      for (int a = 1; a < kNumArt; ++a) { const double v = terms[(size_t)a * S + j]; if (mx < v) mx = v; }
      double total = 0;
#pragma unroll
      for (int a = 0; a < kNumArt; ++a) { const double diff = terms[(size_t)a * S + j] - mx; if (diff > A.log_thresh) total += d_fasterexp((float)diff); }
      const double v = mx + d_fasterlog((float)total);
      g_row[j] = v;
      if (j == S - 1) A.g_last[(size_t)ps * (A.HS + 2) + (sd.len0 - 1) + block_len] = v;       // last[stutter_R], stutter_R = len0 + block_len - 1
    }
#undef LTR_VISIT
  }
}

// 4.: compute_aln_logprob, HapAligner.cpp:165-233: one wavefront per pair, one seed position per lane
__global__ __launch_bounds__(kShortThreads) void ltr_short_final_kernel(ShortArgs A) {
  const int lane = threadIdx.x & 63;
  const int q = (int)blockIdx.x * (kShortThreads / 64) + (int)(threadIdx.x >> 6);
  if (q >= A.chunk_pairs) return;
  const int p = A.chunk_first + q;
  const ShortRead rd = A.reads[A.pair_read[p]];
  const ShortHap hf = A.fw[A.pair_hap[p]];
  const int seed = rd.seed;
  const double* lastL = A.g_last + (size_t)(2 * q) * (A.HS + 2);
  const double* lastR = lastL + (A.HS + 2);
  const double l_prob = A.cum[rd.cum_off + seed], r_prob = A.cum[rd.cum_off + seed + 1 + (rd.len - seed - 1)];     // left_prob of either side, :42
  const int hapsize = hf.len[0] + hf.len[1] + hf.len[2];
  const uint8_t* hs = A.hap_bytes + hf.seq_off;
  const uint8_t seed_char = (A.read_bytes + rd.seq_off)[seed];
  const double sw = A.wrong[rd.q_off + seed], sc = A.correct[rd.q_off + seed];
  const double PRIOR = -A.int_log[hf.len[0] + hf.len[2]];               // num_seeds = non-stutter bases, :175-179
  // entry e: 0 and 1 are the two ends (:184-185, :190-191); then the flank positions in order (:193-225):
  // block 0 coords 1 .. len0-1 (rows lrow = 0.., rrow = hapsize-3 downwards), block 2 coords 0 .. len2-2
  const int n0 = hf.len[0] - 1, n2 = hf.len[2] - 1, ne = 2 + n0 + n2;
  auto entry = [&](const int e) -> double {
    if (e == 0) return PRIOR + (seed_char == hs[0] ? sc : sw) + l_prob + lastR[hapsize - 2];
    if (e == 1) return PRIOR + (seed_char == hs[hapsize - 1] ? sc : sw) + r_prob + lastL[hapsize - 2];
    int k = e - 2, coord, lrow, rrow;
    if (k < n0) { coord = 1 + k; lrow = k; rrow = hapsize - 3 - k; }
    else { k -= n0; coord = hf.len[0] + hf.len[1] + k; lrow = n0 + hf.len[1] + k; rrow = hapsize - 3 - n0 - hf.len[1] - k; }
    return PRIOR + (seed_char == hs[coord] ? sc : sw) + lastL[lrow] + lastR[rrow];
  };
  double mx = -1.7976931348623157e308;
  for (int e = lane; e < ne; e += 64) { const double v = entry(e); if (mx < v) mx = v; }
  mx = w_max(mx, 64);
  double total = 0;
  for (int e = lane; e < ne; e += 64) { const double diff = entry(e) - mx; if (diff > A.log_thresh) total += d_fasterexp((float)diff); }
  total = w_sum(total, 64);                                             // (exact: see the header of this section)
  if (lane == 0) A.out[A.pair_out[p]] = mx + d_fasterlog((float)total); // :230
}

}  // namespace

namespace ltr {

namespace {   // ---- short_batch_run: one set of launches for everything queued, in stages over one per-call struct ----
// One call.  The ORDER of the members carries the invariant of DevLease (ltr_lease.h): the host memory queued copies read or write
// comes first (the batch's arrays are the caller's and outlive the call) and the lease last.
struct ShortCall {
  ShortBatch* B; const int n_pairs;
  std::vector<double> int_log, qtab; std::vector<int64_t> pout;           // short_host_tables
  std::vector<double> out;
  ShortGeom g; ShortArgs A;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const bool trace; const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  DevLease lease;
  ShortCall(ltr_ctx* ctx, ShortBatch* b) : B(b), n_pairs((int)b->pread.size()), trace(ctx_debug(ctx).trace != 0), lease(ctx, (hipStream_t)ctx_stream(ctx)) {}
  void mark(const char* what) const {
    if (trace) std::fprintf(stderr, "[ltr] short_batch_run %8.2f ms: %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), what);
  }
};

// n objects in a block of the context's pool (no hipMalloc / hipFree per call), the copy queued
template <class T> hipError_t short_up(DevLease& lease, const T* src, size_t n, const T** dst) {
  T* d = nullptr;
  const hipError_t e = lease.alloc(&d, std::max<size_t>(n * sizeof(T), 8) + 64);
  *dst = d;
  if (e != hipSuccess) return e;
  return n ? hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, lease.st) : hipSuccess;
}

// uploads queued, work arrays allocated, every field of ShortArgs but the chunk's
int short_upload(ltr_ctx* ctx, ShortCall& c) {
  const ShortBatch* B = c.B; ShortArgs& A = c.A; DevLease& lease = c.lease; const ShortGeom& g = c.g;
  std::memset(&A, 0, sizeof(A));
  DEV_TRY(ctx, short_up(lease, B->reads.data(), B->reads.size(), &A.reads));
  DEV_TRY(ctx, short_up(lease, B->fw.data(), B->fw.size(), &A.fw));
  DEV_TRY(ctx, short_up(lease, B->rv.data(), B->rv.size(), &A.rv));
  DEV_TRY(ctx, short_up(lease, B->rbytes.data(), B->rbytes.size(), &A.read_bytes));
  DEV_TRY(ctx, short_up(lease, B->hbytes.data(), B->hbytes.size(), &A.hap_bytes));
  DEV_TRY(ctx, short_up(lease, B->upstream.data(), B->upstream.size(), &A.upstream));
  c.mark("tables and pairs uploaded");
  DEV_TRY(ctx, short_up(lease, B->qidx.data(), B->qidx.size(), &A.qidx));
  DEV_TRY(ctx, short_up(lease, c.qtab.data(), c.qtab.size(), &A.qtab));
  DEV_TRY(ctx, lease.alloc(&A.wrong_w, B->qidx.size() * sizeof(double) + 64));
  DEV_TRY(ctx, lease.alloc(&A.correct_w, B->qidx.size() * sizeof(double) + 64));
  DEV_TRY(ctx, lease.alloc(&A.cum_w, (size_t)B->n_cum * sizeof(double) + 64));
  DEV_TRY(ctx, short_up(lease, B->art.data(), B->art.size(), &A.art));
  DEV_TRY(ctx, short_up(lease, c.int_log.data(), c.int_log.size(), &A.int_log));
  DEV_TRY(ctx, short_up(lease, B->pread.data(), B->pread.size(), &A.pair_read));
  DEV_TRY(ctx, short_up(lease, B->phap.data(), B->phap.size(), &A.pair_hap));
  DEV_TRY(ctx, short_up(lease, c.pout.data(), c.pout.size(), &A.pair_out));
  DEV_TRY(ctx, lease.alloc(&A.out, c.out.size() * sizeof(double) + 64));
  if (!g.wave_kernel) DEV_TRY(ctx, lease.alloc(&A.scratch, (size_t)g.grid * g.per_block * sizeof(double)));
  c.mark("uploads queued (+ work arrays allocated)");
  const ltr_align_params prm = ctx_params(ctx);
  A.wrong = A.wrong_w; A.correct = A.correct_w; A.cum = A.cum_w;
  A.n_pairs = c.n_pairs; A.period = B->period; A.scratch_per_block = g.per_block;
  A.S = g.S; A.HS = g.HS; A.LP = g.LP; A.n_ilog = (int32_t)c.int_log.size(); A.maxB = B->maxB;
  A.a = prm.log_ins_to_ins; A.b = prm.log_ins_to_match; A.c = prm.log_del_to_del; A.d = prm.log_del_to_match;
  A.e = prm.log_match_to_match; A.f = prm.log_match_to_ins; A.g = prm.log_match_to_del;
  A.log_thresh = std::log(0.001);
  A.n_reads = (int32_t)B->reads.size();
  return LTR_OK;
}

// the four launches of every chunk of pairs (wavefront per (pair, side)); ltr_ctx_set_debug "short_split": events between the
// launches -- the seeded path's time kernel by kernel, ltr_ctx_short_kernel_split
int short_launch_chunks(ltr_ctx* ctx, ShortCall& c) {
  ShortArgs& A = c.A; const ShortGeom& g = c.g; const hipStream_t st = c.lease.st; const int n_pairs = c.n_pairs;
  DEV_TRY(ctx, c.lease.alloc(&A.g_row, (size_t)g.chunk_cap * 2 * g.S * sizeof(double) + 64));
  DEV_TRY(ctx, c.lease.alloc(&A.g_last, (size_t)g.chunk_cap * 2 * (g.HS + 2) * sizeof(double) + 64));
  DEV_TRY(ctx, c.lease.alloc(&A.g_terms, (size_t)g.chunk_cap * 2 * kNumArt * g.S * sizeof(double) + 64));
  const bool split = ctx_debug(ctx).short_split != 0;
  hipEvent_t evs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (split) { for (hipEvent_t& e : evs) DEV_TRY(ctx, c.lease.event(&e, true)); DEV_TRY(ctx, hipEventRecord(evs[0], st)); }
  for (int first = 0; first < n_pairs; first += g.chunk_cap) {
    A.chunk_first = first; A.chunk_pairs = std::min(g.chunk_cap, n_pairs - first);
    const unsigned side_blocks = (unsigned)((2 * (int64_t)A.chunk_pairs + kShortThreads / 64 - 1) / (kShortThreads / 64));
    const unsigned pair_blocks = (unsigned)(((int64_t)A.chunk_pairs + kShortThreads / 64 - 1) / (kShortThreads / 64));
    const unsigned block_grid = (unsigned)(2 * (int64_t)A.chunk_pairs);      // (one workgroup per (pair, side): the sides differ tenfold in length; the dispatcher balances them)
    const bool sp = split && first == 0;                         // (the first chunk: every bounded workload is one chunk)
    hipLaunchKernelGGL((ltr_short_flank_kernel<false>), dim3(side_blocks), dim3(kShortThreads), 0, st, A);
    if (sp) DEV_TRY(ctx, hipEventRecord(evs[1], st));
    hipLaunchKernelGGL(ltr_short_block_kernel, dim3(block_grid), dim3(kShortThreads), g.lds_bytes, st, A);
    if (sp) DEV_TRY(ctx, hipEventRecord(evs[2], st));
    hipLaunchKernelGGL((ltr_short_flank_kernel<true>), dim3(side_blocks), dim3(kShortThreads), 0, st, A);
    if (sp) DEV_TRY(ctx, hipEventRecord(evs[3], st));
    hipLaunchKernelGGL(ltr_short_final_kernel, dim3(pair_blocks), dim3(kShortThreads), 0, st, A);
    if (sp) DEV_TRY(ctx, hipEventRecord(evs[4], st));
  }
  if (split) {
    DEV_TRY(ctx, hipStreamSynchronize(st));
    double ms4[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) { float ms = 0.f; if (hipEventElapsedTime(&ms, evs[k], evs[k + 1]) == hipSuccess) ms4[k] = (double)ms; }
    ctx_note_short_split(ctx, ms4);                              // [prep + flank rows before the block, block row, flank rows after, seed log-sum]
  }
  return LTR_OK;
}

// the per-read tables on the device, then the chunk launches or the lane-per-pair launch
int short_launch(ltr_ctx* ctx, ShortCall& c) {
  const hipStream_t st = c.lease.st;
  DEV_TRY(ctx, c.lease.event(&c.ev0, true)); DEV_TRY(ctx, c.lease.event(&c.ev1, true));
  DEV_TRY(ctx, hipEventRecord(c.ev0, st));
  hipLaunchKernelGGL(ltr_short_prep_kernel, dim3((unsigned)((c.B->reads.size() + kShortThreads / 64 - 1) / (kShortThreads / 64))), dim3(kShortThreads), 0, st, c.A);
  if (c.g.wave_kernel) { const int rc = short_launch_chunks(ctx, c); if (rc != LTR_OK) return rc; }
  else hipLaunchKernelGGL(ltr_short_kernel, dim3((unsigned)c.g.grid), dim3(64), 0, st, c.A);
  DEV_TRY(ctx, hipGetLastError());
  DEV_TRY(ctx, hipEventRecord(c.ev1, st));
  c.mark("launches queued");
  return LTR_OK;
}

// scores back (the call's one wait), device time to the timers, every score to its queued host destination
int short_fetch(ltr_ctx* ctx, ShortCall& c) {
  DEV_TRY(ctx, hipMemcpyAsync(c.out.data(), c.A.out, c.out.size() * sizeof(double), hipMemcpyDeviceToHost, c.lease.st));
  DEV_TRY(ctx, c.lease.drain());
  c.mark("scores back");
  { float ms = 0.f; if (hipEventElapsedTime(&ms, c.ev0, c.ev1) == hipSuccess) add_time(ctx, kTimerShortKernel, 0.0, (double)ms); }
  for (int q = 0; q < c.n_pairs; q++) *c.B->pdst[(size_t)q] = c.out[(size_t)q];
  return LTR_OK;
}
}  // namespace

// One set of launches for everything queued; results go to the queued host destinations.  (Both ways here -- ltr_process_reads
// through process_reads_short, ltr_calc_hap_aln_probs -- are inside LTR_GUARD: an exception unwinds through the lease.)
int short_batch_run(ltr_ctx* ctx, ShortBatch* B) {
  const int64_t n_pairs64 = (int64_t)B->pread.size();
  if (n_pairs64 == 0) return LTR_OK;
  if (n_pairs64 > 0x7fffffff) { set_error(ctx, "short path: too many pairs in one batch"); return LTR_ERR_INVALID; }
  ShortCall c(ctx, B);
  short_host_tables(*B, &c.int_log, &c.qtab, &c.pout);
  c.out.assign((size_t)c.n_pairs, 0.0);
  c.g = short_geometry(*B, c.n_pairs, ctx_debug(ctx).short_lane_kernel != 0);
  (void)hipSetDevice(ctx_device(ctx));
  c.mark("start");
  int rc = short_upload(ctx, c);
  if (rc == LTR_OK) rc = short_launch(ctx, c);
  if (rc == LTR_OK) rc = short_fetch(ctx, c);
  return rc;
}

// HapAligner::process_reads with short_ == 1 (HapAligner.cpp:545-581) for one locus.
int process_reads_short(ltr_ctx* ctx, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap,
                        const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                        const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions) {
  ShortBatch B;
  int rc = short_batch_add(ctx, &B, hap, realign_to_hap, alns, n_alns, init_read_index, realign_read, aln_probs, seed_positions);
  if (rc == LTR_OK) rc = short_batch_run(ctx, &B);
  return rc;
}

}  // namespace ltr
