// ltr_short_batch.cpp -- the host half of the SHORT (seeded, stutter-aware) alignment path: plain C++, no device call.
// What it builds is what the kernels of ltr_short.hip follow offset by offset; it compiles alone, so the host sanitizer
// harness (tests/host_sanitize) runs it as it is.
//
// Integer / libm work of the reference done here: calc_seed_base (HapAligner.cpp:494-542), BaseQuality tables
// (base_quality.h:29-75), StutterModel::log_stutter_pmf (stutter_model.cpp:29-53),
// RepeatStutterInfo::log_prob_pcr_artifact (RepeatStutterInfo.h:53-61), upstream-match tables
// (StutterAlignerClass.h:34-41), int_log (mathops.cpp:14-22).  Every libm value (log, pow) is
// formed here exactly like the reference forms it; the device only adds, compares and runs
// the FP32 bit tricks, so results are bit-identical to the CPU restatement.
// Also here: short_geometry, the rule that picks the launches, the LDS size and the chunk capacity of a call
// (test hook: ltr_debug_short_geometry).

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ltr_internal.h"
#include "ltr_short.h"

namespace {

using namespace ltr;

// HapAligner::calc_best_seed_position, HapAligner.cpp:467-493
void best_seed_position(const std::vector<int32_t>& rs, const std::vector<int32_t>& re, int32_t region_start, int32_t region_end,
                        int32_t* best_dist, int32_t* best_pos) {
  *best_dist = *best_pos = -1;
  int32_t pos = region_start;
  size_t ri = 0;
  while (ri < rs.size() && pos <= region_end) {
    if (pos < rs[ri]) {
      const int32_t dist = 1 + (std::min(region_end, rs[ri] - 1) - pos) / 2;
      if (dist >= *best_dist) { *best_dist = dist; *best_pos = dist - 1 + pos; }
      pos = re[ri++];
    } else if (pos < re[ri]) pos = re[ri++];
    else ri++;
  }
  if (pos <= region_end) {
    const int32_t dist = 1 + (region_end - pos) / 2;
    if (dist >= *best_dist) { *best_dist = dist; *best_pos = dist - 1 + pos; }
  }
}

// HapAligner::calc_seed_base, HapAligner.cpp:494-542; -2 = CIGAR op the reference dies on
int calc_seed_base(const ltr_alignment* aln, const ltr_haplotype_blocks* hap) {
  std::vector<int32_t> rs, re;
  for (int b = 0; b < hap->n_blocks; b++) if (hap->is_repeat[b]) { rs.push_back(hap->block_start[b]); re.push_back(hap->block_end[b]); }
  const int32_t first_start = hap->block_start[0], last_end = hap->block_end[hap->n_blocks - 1];
  int32_t pos = aln->start;
  int best_seed = -1, cur_base = 0, max_dist = 5;                      // MIN_SEED_DIST, :17
  for (int k = 0; k < aln->n_cigar; k++) {
    const int num = aln->cigar_num[k];
    switch (aln->cigar_type[k]) {
      case '=': {
        const int32_t min_region = std::max(pos, first_start), max_region = std::min(pos + num - 1, last_end - 1);
        if (min_region <= max_region) {
          int32_t distance, dist_pos;
          best_seed_position(rs, re, min_region, max_region, &distance, &dist_pos);
          if (distance >= max_dist) { max_dist = distance; best_seed = cur_base + (dist_pos - pos); }
        }
        pos += num; cur_base += num; break;
      }
      case 'I': cur_base += num; break;
      case 'X': pos += num; cur_base += num; break;
      case 'D': pos += num; break;
      default: return -2;
    }
  }
  if (best_seed < -1 || best_seed == 0 || best_seed >= aln->seq_len - 1) return -1;
  return best_seed;
}

struct StutterLogs { double in_nostep, in_step, in_up, in_down, equal, out_nostep, out_step, out_up, out_down; };
// StutterModel::log_stutter_pmf, stutter_model.cpp:29-53
double stutter_pmf(const StutterLogs& s, int motif_len, int sample_bps, int read_bps) {
  const int bp_diff = read_bps - sample_bps;
  if (bp_diff % motif_len != 0) {
    const int eff = bp_diff - (bp_diff / motif_len);
    return eff < 0 ? s.out_down + s.out_nostep + s.out_step * (-eff - 1) : s.out_up + s.out_nostep + s.out_step * (eff - 1);
  }
  const int rep = bp_diff / motif_len;
  if (rep == 0) return s.equal;
  return rep < 0 ? s.in_down + s.in_nostep + s.in_step * (-rep - 1) : s.in_up + s.in_nostep + s.in_step * (rep - 1);
}

}  // namespace

namespace ltr {

ShortBatch* short_batch_new() { return new ShortBatch(); }
// dst += src (src is left empty): loci are prepared one batch each on the host's cores and strung together here --
// offsets into the byte / table arrays and the pairs' read / haplotype indices move by what dst already holds.
int short_batch_merge(ltr_ctx* ctx, ShortBatch* dst, ShortBatch* src) {
  if (src->reads.empty() && src->pread.empty()) return LTR_OK;
  if (dst->period == 0) dst->period = src->period;
  if (src->period != 0 && dst->period != src->period) { set_error(ctx, "short path: loci of one batch must share the repeat period"); return LTR_ERR_UNSUPPORTED; }
  const int64_t rb0 = (int64_t)dst->rbytes.size(), hb0 = (int64_t)dst->hbytes.size(), q0 = (int64_t)dst->qidx.size(), c0 = dst->n_cum;
  const int64_t up0 = (int64_t)dst->upstream.size();
  const int32_t r0 = (int32_t)dst->reads.size(), h0 = (int32_t)dst->fw.size();
  if ((uint64_t)up0 + src->upstream.size() > 0x7fffff00u || (uint64_t)r0 + src->reads.size() > 0x7fffff00u) { set_error(ctx, "short path: batch too large"); return LTR_ERR_INVALID; }
  for (ShortRead sr : src->reads) { sr.seq_off += rb0; sr.rev_off += rb0; sr.q_off += q0; sr.cum_off += c0; dst->reads.push_back(sr); }
  for (ShortHap h : src->fw) { h.seq_off += hb0; h.up_off += (int32_t)up0; dst->fw.push_back(h); }
  for (ShortHap h : src->rv) { h.seq_off += hb0; h.up_off += (int32_t)up0; dst->rv.push_back(h); }
  dst->rbytes.insert(dst->rbytes.end(), src->rbytes.begin(), src->rbytes.end());
  dst->hbytes.insert(dst->hbytes.end(), src->hbytes.begin(), src->hbytes.end());
  dst->qidx.insert(dst->qidx.end(), src->qidx.begin(), src->qidx.end());
  dst->upstream.insert(dst->upstream.end(), src->upstream.begin(), src->upstream.end());
  dst->art.insert(dst->art.end(), src->art.begin(), src->art.end());
  for (int32_t v : src->pread) dst->pread.push_back(v + r0);
  for (int32_t v : src->phap) dst->phap.push_back(v + h0);
  dst->pdst.insert(dst->pdst.end(), src->pdst.begin(), src->pdst.end());
  dst->n_cum += src->n_cum;
  dst->maxS = std::max(dst->maxS, src->maxS); dst->maxHS = std::max(dst->maxHS, src->maxHS); dst->maxB = std::max(dst->maxB, src->maxB);
  *src = ShortBatch();
  return LTR_OK;
}
void short_batch_free(ShortBatch* b) { delete b; }

// ... its haplotype combinations, both directions: bytes, upstream-match tables, artifact terms; the first of them is B->fw[hap0]
static int short_add_haps(ltr_ctx* ctx, ShortBatch* B, const ltr_haplotype_blocks* hap, const std::vector<int32_t>& counts, int64_t H, size_t hap0) {
  const ltr_stutter_params sp = ctx_stutter_params(ctx);
  const int period = hap->period[1];
  StutterLogs sl;
  sl.in_step = std::log(1 - sp.in_geom); sl.in_nostep = std::log(sp.in_geom); sl.in_up = std::log(sp.in_up); sl.in_down = std::log(sp.in_down);
  sl.out_step = std::log(1 - sp.out_geom); sl.out_nostep = std::log(sp.out_geom); sl.out_up = std::log(sp.out_up); sl.out_down = std::log(sp.out_down);
  sl.equal = std::log(1 - sp.in_up - sp.in_down - sp.out_up - sp.out_down);
  B->fw.resize(hap0 + (size_t)H); B->rv.resize(hap0 + (size_t)H); B->art.resize((hap0 + (size_t)H) * kNumArt);
  std::vector<int32_t>& upstream = B->upstream;
  auto slot = [&](int b, int al) { int64_t k = 0; for (int q = 0; q < b; q++) k += hap->n_alleles[q]; return k + al; };
  auto add_upstream = [&](const std::vector<uint8_t>& blk, ShortHap* h) {      // StutterAlignerClass ctor, .h:45-79
    const int len = (int)blk.size();
    int nd = kMaxDel;
    while (nd * period > len) nd--;
    h->num_deletions = nd; h->up_off = (int32_t)upstream.size();
    auto one = [&](int per) {                                                    // num_upstream_matches, .h:34-41
      const size_t base = upstream.size();
      upstream.resize(base + (size_t)std::max(len, 1), 0);
      for (int i = per; i < len; i++) upstream[base + i] = (blk[i - per] != blk[i]) ? 0 : 1 + upstream[base + i - 1];
    };
    for (int i = 1; i <= nd; i++) one(i * period);
    if (nd == 0) one(period);
  };
  for (int64_t k = 0; k < H; k++) {
    std::vector<uint8_t> blk[3];
    for (int b = 0; b < 3; b++) {
      const int64_t s = slot(b, counts[(size_t)(k * 3 + b)]);
      blk[b].assign(hap->allele_bytes + hap->allele_off[s], hap->allele_bytes + hap->allele_off[s + 1]);
    }
    if (blk[0].empty() || blk[2].empty()) { set_error(ctx, "short path: empty flank block"); return LTR_ERR_INVALID; }
    ShortHap& f = B->fw[hap0 + (size_t)k]; ShortHap& r = B->rv[hap0 + (size_t)k];
    f.seq_off = (int64_t)B->hbytes.size(); f.pad = 0;
    for (int b = 0; b < 3; b++) { f.len[b] = (int32_t)blk[b].size(); B->hbytes.insert(B->hbytes.end(), blk[b].begin(), blk[b].end()); }
    add_upstream(blk[1], &f);
    r.seq_off = (int64_t)B->hbytes.size(); r.pad = 0;                           // Haplotype::reverse: blocks and bases reversed
    for (int b = 0; b < 3; b++) { std::vector<uint8_t> t(blk[2 - b].rbegin(), blk[2 - b].rend()); r.len[b] = (int32_t)t.size(); B->hbytes.insert(B->hbytes.end(), t.begin(), t.end()); if (b == 1) add_upstream(t, &r); }
    const int bl = (int)blk[1].size();
    for (int q = 0; q < kNumArt; q++) {                                          // log_prob_pcr_artifact, RepeatStutterInfo.h:53-61
      const int asz = (q - kMaxDel) * period, read_size = bl + asz;
      B->art[(hap0 + (size_t)k) * kNumArt + q] = (asz < 0 && read_size < 0) ? -10e6 : stutter_pmf(sl, period, bl, read_size);   // (asz <= max_ins always)
    }
    B->maxHS = std::max(B->maxHS, (int)(blk[0].size() + blk[1].size() + blk[2].size()));
    B->maxB = std::max(B->maxB, bl);
  }
  if (upstream.size() > 0x7fffff00u) { set_error(ctx, "short path: batch too large"); return LTR_ERR_INVALID; }
  return LTR_OK;
}

// HapAligner::process_reads with short_ == 1 (HapAligner.cpp:545-581), host half, for one locus:
// seeds and the all-zero rows of seedless reads are written at once, the pairs are queued.
// aln_probs must stay valid until short_batch_run.
int short_batch_add(ltr_ctx* ctx, ShortBatch* B, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap,
                    const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                    const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions) {
  if (hap->n_blocks != 3 || hap->is_repeat[0] || !hap->is_repeat[1] || hap->is_repeat[2]) {
    set_error(ctx, "short path: expected [flank][repeat][flank] blocks (Haplotype.cpp:8 asserts the same)");
    return LTR_ERR_UNSUPPORTED;
  }
  const int period = hap->period[1];
  if (B->period == 0) B->period = period;
  if (B->period != period) { set_error(ctx, "short path: loci of one batch must share the repeat period"); return LTR_ERR_UNSUPPORTED; }
  std::vector<int32_t> counts; int64_t H = 0;
  int rc = haplotype_counts(hap, &counts, &H);
  if (rc != LTR_OK) return rc;

  // ---- reads: seeds, quality table indices (BaseQuality, base_quality.h:45-75; the tables themselves: short_host_tables) ----
  auto qidx = [](uint8_t q) { const char c = (char)q; return c < '!' ? 0 : (c > 'J' ? 'J' - '!' : c - '!'); };
  std::vector<int32_t> read_of_aln((size_t)n_alns, -1);
  double* prob_ptr = aln_probs + (int64_t)init_read_index * H;
  const size_t reads0 = B->reads.size();
  for (int32_t r = 0; r < n_alns; r++) {
    if (realign_read && !realign_read[r]) continue;
    const ltr_alignment& a = alns[r];
    const int seed = calc_seed_base(&a, hap);                                     // :568
    if (seed == -2) { set_error(ctx, "Unrecognized CIGAR char in calc_seed_base()"); return LTR_ERR_CIGAR; }
    seed_positions[init_read_index + r] = seed;
    if (seed == -1) { for (int64_t k = 0; k < H; k++) prob_ptr[(int64_t)r * H + k] = 0; continue; }   // :570-574
    if (!a.qual) { set_error(ctx, "short path needs base qualities (ltr_alignment.qual)"); return LTR_ERR_INVALID; }
    ShortRead sr; sr.len = a.seq_len; sr.seed = seed;
    const int len = a.seq_len;
    sr.seq_off = (int64_t)B->rbytes.size(); sr.rev_off = sr.seq_off + len;
    B->rbytes.resize(B->rbytes.size() + (size_t)len + (size_t)(len - 1 - seed));
    {
      uint8_t* fwd = B->rbytes.data() + sr.seq_off; uint8_t* rev = fwd + len;
      std::memcpy(fwd, a.seq, (size_t)len);
      for (int j = len - 1; j > seed; j--) *rev++ = a.seq[j];                     // rev_rseq, :887-888
    }
    sr.q_off = (int64_t)B->qidx.size(); sr.cum_off = B->n_cum;
    B->qidx.resize(B->qidx.size() + (size_t)len); B->n_cum += (int64_t)len + 1;
    {
      uint8_t* qi = B->qidx.data() + sr.q_off;
      for (int j = 0; j <= seed; j++) *qi++ = (uint8_t)qidx(a.qual[j]);
      for (int j = len - 1; j > seed; j--) *qi++ = (uint8_t)qidx(a.qual[j]);      // :889-890
    }
    read_of_aln[(size_t)r] = (int32_t)B->reads.size();
    B->reads.push_back(sr);
    B->maxS = std::max(B->maxS, std::max(seed, a.seq_len - seed - 1));
  }
  if (B->reads.size() == reads0) return LTR_OK;
  const size_t hap0 = B->fw.size();
  if ((rc = short_add_haps(ctx, B, hap, counts, H, hap0)) != LTR_OK) return rc;
  // ---- pairs -----------------------------------------------------------------------------
  for (int32_t r = 0; r < n_alns; r++) {
    if (read_of_aln[(size_t)r] < 0) continue;
    for (int64_t k = 0; k < H; k++) {
      if (realign_to_hap && !realign_to_hap[k]) continue;                        // :896-900
      B->pread.push_back(read_of_aln[(size_t)r]); B->phap.push_back((int32_t)(hap0 + (size_t)k));
      B->pdst.push_back(prob_ptr + (int64_t)r * H + k);
    }
  }
  return LTR_OK;
}

ShortGeom short_geometry(const ShortBatch& B, int n_pairs, bool lane_knob) {
  ShortGeom g;
  g.S = std::max(B.maxS, std::max(B.maxB + 2, kNumArt)) + 2; g.HS = B.maxHS + 4;
  g.LP = std::max(g.S, g.HS) + 8;
  g.per_block = (int64_t)(19 * g.S + g.LP + 2 * (g.HS + 2)) * 64;
  // one wave per block; enough blocks to keep a few waves per SIMD busy with other pairs while a
  // lane waits for its work arrays (scratch capped at 8 GB)
  const int64_t cap_blocks = std::max<int64_t>(1, ((int64_t)8 << 30) / (g.per_block * (int64_t)sizeof(double)));
  g.grid = (int)std::min<int64_t>(std::min<int64_t>((n_pairs + 63) / 64, 4096), cap_blocks);
  // The four-launch path whenever a side fits 64 lanes x 8 read positions and the block kernel's tables fit 64 KB of LDS;
  // beyond that (reads cut wider than the reference's +-200 bp) the lane-per-pair kernel with its global work arrays.
  g.lds_bytes = ((size_t)4 * g.S + B.n_ilog()) * sizeof(double) + ((size_t)kMaxDel * B.maxB + 8) * sizeof(int32_t) +
                (size_t)((g.S + 7) & ~7) + (size_t)g.HS + 64;
  g.wave_kernel = std::max(B.maxS, 1) <= 64 * 8 && g.lds_bytes <= 64 * 1024 && !lane_knob;
  // pairs per set of launches: the block row's terms (13 x S doubles per side) fit ONE GB -- a block the context's pool keeps
  // between calls (beyond 2 GB a block is a hipMalloc / hipFree per call: 15-20 ms each on MI355X, and a device-wide wait)
  const size_t terms_side_bytes = (size_t)kNumArt * g.S * sizeof(double);
  g.chunk_cap = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pairs, (((size_t)1 << 30) - 64) / (2 * terms_side_bytes)));
  return g;
}

void short_host_tables(const ShortBatch& B, std::vector<double>* int_log, std::vector<double>* qtab, std::vector<int64_t>* pout) {
  int_log->resize(B.n_ilog());
  (*int_log)[0] = -1000;                                                         // mathops.cpp:17
  for (size_t i = 1; i < int_log->size(); i++) (*int_log)[i] = std::log((double)i);
  const int MAXQ = 'J' - '!';                                                    // BaseQuality's tables, base_quality.h:29-43
  qtab->assign(128, 0.0);
  (*qtab)[64] = -100; (*qtab)[0] = 0;
  for (int i = 1; i <= MAXQ; ++i) { (*qtab)[64 + i] = std::log(1.0 - std::pow(10.0, i / (-10.0))); (*qtab)[i] = std::log(std::pow(10.0, i / (-10.0) / 5.0)); }
  pout->resize(B.pread.size());
  for (size_t q = 0; q < pout->size(); q++) (*pout)[q] = (int64_t)q;
}

}  // namespace ltr

// test hook (include/ltr_gpu.h): the host calc_seed_base above, for the pin against the compiled reference
extern "C" int ltr_debug_calc_seed_base(const ltr_alignment* aln, const ltr_haplotype_blocks* hap) {
  if (!aln || !hap || hap->n_blocks <= 0) return LTR_ERR_INVALID;
  return calc_seed_base(aln, hap);
}

// test hook (ltr_short.h): short_geometry of a batch with these maxima
extern "C" int ltr_debug_short_geometry(int32_t max_side, int32_t max_block, int32_t max_hap, int32_t n_pairs, int32_t lane_knob, int64_t out[8]) {
  if (!out || max_side < 0 || max_block < 0 || max_hap < 0 || n_pairs < 0) return LTR_ERR_INVALID;
  ltr::ShortBatch B;
  B.maxS = max_side; B.maxB = max_block; B.maxHS = max_hap;
  const ltr::ShortGeom g = ltr::short_geometry(B, n_pairs, lane_knob != 0);
  out[0] = g.S; out[1] = g.HS; out[2] = g.LP; out[3] = (int64_t)g.lds_bytes; out[4] = g.chunk_cap; out[5] = g.wave_kernel; out[6] = g.grid; out[7] = g.per_block;
  return LTR_OK;
}
