// ltr_host.cpp -- host-side mirror of the reference objects either side of the DP, per locus:
// Haplotype iteration, HapAligner::trim_alignment, HapAligner::process_reads (long branch),
// ReadPooler, and the pool->read scatter of SeqStutterGenotyper::calc_hap_aln_probs (for many loci in one call: ltr_hap_aln.cpp).
// Integer / string work only; every DP cell is scored on the GPU through ltr_align_batch.
// Citations are to the LongTR reference (paths under its repository root).

#include <algorithm>
#include <thread>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "ltr_internal.h"

namespace ltr {

// Haplotype::init()/next(), forward direction (Haplotype.cpp:123-196): a mixed-radix
// reflected Gray walk.  factors_[i] = prod_{k<i} nopts_[k]; the block that moves at step
// `counter` is the LAST j with ((counter+1) mod factors_[j..]) == 0 taken right to left;
// it moves by dirs_[j], which flips at either end.
int haplotype_counts(const ltr_haplotype_blocks* hap, std::vector<int32_t>* counts_out, int64_t* ncombs_out) {
  if (!hap || hap->n_blocks <= 0) return LTR_ERR_INVALID;
  const int nb = hap->n_blocks;
  std::vector<int64_t> factors(nb);
  std::vector<int32_t> dirs(nb, 1), counts(nb, 0);
  int64_t ncombs = 1;
  for (int i = 0; i < nb; ++i) {
    if (hap->n_alleles[i] <= 0) return LTR_ERR_INVALID;
    factors[i] = ncombs;
    ncombs *= hap->n_alleles[i];
    if (ncombs > (1 << 24)) return LTR_ERR_INVALID;
  }
  counts_out->assign((size_t)(ncombs * nb), 0);
  for (int64_t c = 0;; ++c) {
    for (int i = 0; i < nb; ++i) (*counts_out)[(size_t)(c * nb + i)] = counts[i];
    if (c == ncombs - 1) break;
    int64_t t = c + 1;
    int idx = -1;
    for (int j = nb - 1; j >= 0; --j) { t %= factors[j]; if (t == 0) { idx = j; break; } }
    counts[idx] += dirs[idx];
    if (counts[idx] == 0 || counts[idx] == hap->n_alleles[idx] - 1) dirs[idx] *= -1;
  }
  *ncombs_out = ncombs;
  return LTR_OK;
}

int64_t allele_slot(const ltr_haplotype_blocks* hap, int block, int allele) {
  int64_t k = 0;
  for (int b = 0; b < block; ++b) k += hap->n_alleles[b];
  return k + allele;
}

static void hap_string(const ltr_haplotype_blocks* hap, const int32_t* counts, std::string* out) {
  out->clear();
  for (int b = 0; b < hap->n_blocks; ++b) {                    // Haplotype::get_seq(), Haplotype.h:99-104
    const int64_t k = allele_slot(hap, b, counts[b]);
    out->append(reinterpret_cast<const char*>(hap->allele_bytes) + hap->allele_off[k],
                (size_t)(hap->allele_off[k + 1] - hap->allele_off[k]));
  }
}

// HapAligner::trim_alignment (HapAligner.cpp:346-465).  The reference copies the CIGAR and consumes it ONE BASE at a
// time from the front (left region :360-382, then left flank :385-408) and from the back (right region :411-433,
// right flank :436-458).  Inside one CIGAR element every base does the same thing, so each of the four walks is
// done element by element here: an element gives up min(its remaining bases, the bases the walk still wants).
// `rem` (scratch, n_cigar ints) holds what is left of every element; front and back cursors share it like the
// reference's list.  Same results, O(#elements) instead of O(read length) (checked against the compiled
// reference's trims: tests/golden/process_locus.json, and against the base-by-base restatement on random CIGARs).
static inline int cigar_klass(char t) {                          // 0: M/=/X  1: D  2: I/S  3: H  -1: invalid
  switch (t) { case 'M': case '=': case 'X': return 0; case 'D': return 1; case 'I': case 'S': return 2; case 'H': return 3; default: return -1; }
}
int trim_alignment_into(const ltr_alignment* aln, int32_t repeat_start, int32_t repeat_end, int32_t padding,
                               int32_t* rem, int32_t* ltrim_out, int32_t* rtrim_out) {
  // A CIGAR element of length < 1 never runs out in the reference's one-base-at-a-time walk
  // (get_num() == 1 is its only exit, :376-379): rejected here instead of looping.
  for (int32_t k = 0; k < aln->n_cigar; ++k) { if (aln->cigar_num[k] < 1) return LTR_ERR_CIGAR; rem[k] = aln->cigar_num[k]; }
  const int64_t lo = (int64_t)repeat_start - padding, hi = (int64_t)repeat_end + padding;      // :349-350
  int64_t start_pos = (int64_t)aln->start + 1, end_pos = (int64_t)aln->stop + 1;               // :351,:353
  int64_t ltrim = 0, rtrim = 0;
  int fi = 0, bi = aln->n_cigar - 1;
  while (start_pos <= lo && fi <= bi) {                        // left region, :360-382
    const int k = cigar_klass(aln->cigar_type[fi]);
    if (k < 0) return LTR_ERR_CIGAR;
    int64_t take = rem[fi];
    if (k <= 1) { take = std::min<int64_t>(take, lo - start_pos + 1); start_pos += take; }
    if (k == 0 || k == 2) ltrim += take;
    if ((rem[fi] -= (int32_t)take) == 0) ++fi;
  }
  for (int64_t mid = start_pos; mid > lo && mid <= lo + padding && fi <= bi;) {   // left flank, :385-408
    const int k = cigar_klass(aln->cigar_type[fi]);
    if (k < 0) return LTR_ERR_CIGAR;
    int64_t take = rem[fi];
    if (k <= 1) { take = std::min<int64_t>(take, lo + padding - mid + 1); mid += take; }
    if (k == 1) ltrim -= take;
    if ((rem[fi] -= (int32_t)take) == 0) ++fi;
  }
  while (end_pos > hi && fi <= bi) {                           // right region, :411-433
    const int k = cigar_klass(aln->cigar_type[bi]);
    if (k < 0) return LTR_ERR_CIGAR;
    int64_t take = rem[bi];
    if (k <= 1) { take = std::min<int64_t>(take, end_pos - hi); end_pos -= take; }
    if (k == 0 || k == 2) rtrim += take;
    if ((rem[bi] -= (int32_t)take) == 0) --bi;
  }
  for (int64_t mid = end_pos; mid > hi - padding && mid <= hi && fi <= bi;) {     // right flank, :436-458
    const int k = cigar_klass(aln->cigar_type[bi]);
    if (k < 0) return LTR_ERR_CIGAR;
    int64_t take = rem[bi];
    if (k <= 1) { take = std::min<int64_t>(take, mid - (hi - padding)); mid -= take; }
    if (k == 1) rtrim -= take;
    if ((rem[bi] -= (int32_t)take) == 0) --bi;
  }
  if (ltrim < 0) ltrim = 0;                                    // :461-462
  if (rtrim < 0) rtrim = 0;
  *ltrim_out = (int32_t)ltrim; *rtrim_out = (int32_t)rtrim;
  return (ltrim + rtrim <= aln->seq_len) ? LTR_OK : LTR_ERR_INVALID;         // assert, :463
}
static int trim_alignment(const ltr_alignment* aln, int32_t repeat_start, int32_t repeat_end, int32_t padding,
                          int32_t* ltrim_out, int32_t* rtrim_out) {
  std::vector<int32_t> rem((size_t)std::max(aln->n_cigar, 1));
  return trim_alignment_into(aln, repeat_start, repeat_end, padding, rem.data(), ltrim_out, rtrim_out);
}

const char* trim_error_text(int rc) {
  return rc == LTR_ERR_CIGAR ? "Invalid CIGAR option encountered in trim_alignment" : "trim_alignment: ltrim+rtrim exceeds the read length";
}

int32_t empty_trim_len(const ltr_haplotype_blocks* hap) {
  const int64_t aL = allele_slot(hap, hap->n_blocks - 1, 0);
  if (hap->allele_off[1] - hap->allele_off[0] < 5) return -1;
  return (int32_t)(5 + std::min<int64_t>(hap->allele_off[aL + 1] - hap->allele_off[aL], 5));
}
void write_empty_trim(const ltr_haplotype_blocks* hap, uint8_t* dst) {
  const int64_t aL = allele_slot(hap, hap->n_blocks - 1, 0);
  std::memcpy(dst, hap->allele_bytes + hap->allele_off[1] - 5, 5);
  std::memcpy(dst + 5, hap->allele_bytes + hap->allele_off[aL], (size_t)std::min<int64_t>(hap->allele_off[aL + 1] - hap->allele_off[aL], 5));
}

// trimmed read of one alignment appended to a byte pool: trim_alignment (:819) or, for an empty trim, its substitute
static int append_trimmed(std::string* err, const ltr_haplotype_blocks* hap, int rb, const ltr_alignment* aln, int32_t padding,
                          std::vector<uint8_t>* read_bytes, std::vector<int64_t>* read_off) {
  int32_t lt = 0, rt = 0;
  const int rc = trim_alignment(aln, hap->block_start[rb], hap->block_end[rb], padding, &lt, &rt);
  if (rc != LTR_OK) { *err = trim_error_text(rc); return rc; }
  const int64_t len = (int64_t)aln->seq_len - lt - rt;
  if (len > 0) {
    read_bytes->insert(read_bytes->end(), aln->seq + lt, aln->seq + lt + len);
  } else {
    const int32_t sub = empty_trim_len(hap);
    if (sub < 0) { *err = kShortLeftFlank; return LTR_ERR_INVALID; }
    read_bytes->resize(read_bytes->size() + (size_t)sub);
    write_empty_trim(hap, read_bytes->data() + read_bytes->size() - sub);
  }
  read_off->push_back((int64_t)read_bytes->size());
  return LTR_OK;
}

// One multi-allele block (every locus the genotyper builds: [flank][repeat][flank]) means haplotype k == allele k of that block
// (Haplotype.cpp:151-206): no table of Haplotype::next() needed
static bool one_multi_block(const ltr_haplotype_blocks* hap) {
  int multi = 0;
  for (int b = 0; b < hap->n_blocks; ++b) if (hap->n_alleles[b] > 1) ++multi;
  return multi <= 1;
}
int haplotype_sizes(const ltr_haplotype_blocks* hap, std::vector<int32_t>* counts, int64_t* n_haps, int64_t* n_bytes) {
  if (hap->n_blocks <= 0) return LTR_ERR_INVALID;
  int64_t H = 1;
  for (int b = 0; b < hap->n_blocks; ++b) {
    if (hap->n_alleles[b] <= 0) return LTR_ERR_INVALID;
    H *= hap->n_alleles[b];
    if (H > (1 << 24)) return LTR_ERR_INVALID;
  }
  int64_t tot = 0;
  if (one_multi_block(hap)) {
    int64_t k = 0, fixed = 0, var = 0;
    for (int b = 0; b < hap->n_blocks; ++b) {
      const int na = hap->n_alleles[b];
      if (na == 1) fixed += hap->allele_off[k + 1] - hap->allele_off[k];
      else var = hap->allele_off[k + na] - hap->allele_off[k];
      k += na;
    }
    tot = fixed * H + var;
  } else {
    int64_t nc = 0;
    if (haplotype_counts(hap, counts, &nc) != LTR_OK) return LTR_ERR_INVALID;
    for (int64_t c = 0; c < nc; ++c)
      for (int b = 0; b < hap->n_blocks; ++b) { const int64_t a = allele_slot(hap, b, (*counts)[(size_t)(c * hap->n_blocks + b)]); tot += hap->allele_off[a + 1] - hap->allele_off[a]; }
  }
  *n_haps = H; *n_bytes = tot;
  return LTR_OK;
}
int64_t write_haplotypes(const ltr_haplotype_blocks* hap, int64_t n_haps, std::vector<int32_t>* counts, uint8_t* bytes, int64_t at, int64_t* off) {
  const int nb = hap->n_blocks;
  const bool simple = one_multi_block(hap);
  if (!simple) { int64_t nc = 0; (void)haplotype_counts(hap, counts, &nc); }
  for (int64_t h = 0; h < n_haps; ++h) {
    off[h] = at;
    int64_t slot0 = 0;
    for (int b = 0; b < nb; ++b) {                               // Haplotype::get_seq(), Haplotype.h:99-104
      const int na = hap->n_alleles[b];
      const int a = simple ? (na > 1 ? (int)h : 0) : (*counts)[(size_t)(h * nb + b)];
      const int64_t s0 = hap->allele_off[slot0 + a], s1 = hap->allele_off[slot0 + a + 1];
      std::memcpy(bytes + at, hap->allele_bytes + s0, (size_t)(s1 - s0));
      at += s1 - s0; slot0 += na;
    }
  }
  return at;
}

int sum_mate_rows(double* rows, int32_t n_reads, int64_t n_haps, const uint8_t* second_mate, const uint8_t* copy_read, const uint8_t* realign_to_hap) {
  if (!second_mate) return LTR_OK;
  for (int32_t i = 0; i < n_reads; ++i) {
    if (!second_mate[i] || (copy_read && !copy_read[i])) continue;
    if (i == 0) return LTR_ERR_INVALID;
    double* m1 = rows + (int64_t)(i - 1) * n_haps;
    double* m2 = rows + (int64_t)i * n_haps;
    for (int64_t j = 0; j < n_haps; ++j)
      if (!realign_to_hap || realign_to_hap[j]) { const double tot = m1[j] + m2[j]; m1[j] = tot; m2[j] = tot; }
  }
  return LTR_OK;
}

}  // namespace ltr

extern "C" {

int64_t ltr_haplotype_num_combs(const ltr_haplotype_blocks* hap) {
  if (!hap || hap->n_blocks <= 0) return LTR_ERR_INVALID;
  int64_t n = 1;
  for (int i = 0; i < hap->n_blocks; ++i) n *= hap->n_alleles[i];
  return n;
}

int64_t ltr_haplotype_seq(const ltr_haplotype_blocks* hap, int64_t index, uint8_t* out, int64_t cap) {
  std::vector<int32_t> counts; int64_t ncombs = 0;
  const int rc = ltr::haplotype_counts(hap, &counts, &ncombs);
  if (rc != LTR_OK) return rc;
  if (index < 0 || index >= ncombs) return LTR_ERR_INVALID;
  std::string s;
  ltr::hap_string(hap, counts.data() + index * hap->n_blocks, &s);
  if ((int64_t)s.size() > cap) return LTR_ERR_INVALID;
  std::memcpy(out, s.data(), s.size());
  return (int64_t)s.size();
}

int ltr_trim_alignment(const ltr_alignment* aln, int32_t repeat_start, int32_t repeat_end,
                       int32_t indel_flank_len, int32_t* ltrim, int32_t* rtrim) {
  if (!aln || !ltrim || !rtrim) return LTR_ERR_INVALID;
  return ltr::trim_alignment(aln, repeat_start, repeat_end, indel_flank_len, ltrim, rtrim);
}

// HapAligner::process_reads (HapAligner.cpp:545-581) + process_read's long branch (:814-854).
int ltr_process_reads(ltr_ctx* ctx, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap,
                      const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                      const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions) {
  if (!ctx || !hap || (!alns && n_alns > 0) || n_alns < 0 || !aln_probs || !seed_positions) return LTR_ERR_INVALID;
  for (int32_t i = 0; i < n_alns; ++i)
    if (!ltr::alignment_record_ok(alns[i])) { ltr::set_error(ctx, ltr::kBadAlignmentRecord); return LTR_ERR_INVALID; }
  ltr::TimedCall timed(ctx, ltr::kTimerHapAln);                // total_hap_aln_time_, seq_stutter_genotyper.cpp:515,:561-562
  LTR_GUARD_BEGIN
  // repeat_starts_[0] / repeat_ends_[0]: the first block that carries repeat info (HapAligner.h:103-109)
  int rb = -1;
  for (int b = 0; b < hap->n_blocks; ++b) if (hap->is_repeat[b]) { rb = b; break; }
  if (rb < 0) { ltr::set_error(ctx, "haplotype has no repeat block"); return LTR_ERR_INVALID; }
  // short_ = (block 1 period == 1 && SWITCH_OLD_ALIGN_LEN), :552: the seeded stutter path
  if (ltr::ctx_params(ctx).use_short_path && hap->n_blocks > 1 && hap->period[1] == 1)
    return ltr::process_reads_short(ctx, hap, realign_to_hap, alns, n_alns, init_read_index, realign_read,
                                    aln_probs, seed_positions);
  // haplotype strings in Haplotype::next() order
  std::vector<int32_t> counts; int64_t H = 0, n_hb = 0;
  int rc = ltr::haplotype_sizes(hap, &counts, &H, &n_hb);
  if (rc != LTR_OK) { ltr::set_error(ctx, "bad haplotype block structure"); return rc; }
  std::vector<uint8_t> hap_bytes((size_t)std::max<int64_t>(n_hb, 1)); std::vector<int64_t> hap_off((size_t)H + 1);
  hap_off[(size_t)H] = ltr::write_haplotypes(hap, H, &counts, hap_bytes.data(), 0, hap_off.data());
  std::vector<uint8_t> read_bytes; std::vector<int64_t> read_off(1, 0);
  std::vector<uint8_t> mask_r((size_t)n_alns, 1);
  const int32_t padding = ltr::ctx_params(ctx).indel_flank_len;
  for (int32_t i = 0; i < n_alns; ++i) {
    if (realign_read && !realign_read[i]) { mask_r[(size_t)i] = 0; read_bytes.push_back('N'); read_off.push_back((int64_t)read_bytes.size()); continue; }
    std::string err;
    if ((rc = ltr::append_trimmed(&err, hap, rb, &alns[i], padding, &read_bytes, &read_off)) != LTR_OK) { ltr::set_error(ctx, err); return rc; }
  }
  ltr_locus_batch b;
  std::memset(&b, 0, sizeof(b));
  const int64_t lro[2] = {0, n_alns}, lho[2] = {0, H};
  b.n_loci = 1; b.locus_read_off = lro; b.locus_hap_off = lho;
  b.n_reads = n_alns; b.read_bytes = read_bytes.data(); b.read_off = read_off.data();
  b.n_haps = H; b.hap_bytes = hap_bytes.data(); b.hap_off = hap_off.data();
  b.realign_read = mask_r.data(); b.realign_hap = realign_to_hap;
  double* prob_ptr = aln_probs + (int64_t)init_read_index * H;                // :550
  rc = ltr_align_batch(ctx, &b, prob_ptr, nullptr);
  if (rc != LTR_OK) return rc;
  for (int32_t i = 0; i < n_alns; ++i)
    if (mask_r[(size_t)i]) seed_positions[init_read_index + i] = alns[i].seq_len - 1;   // :562-563 (UNtrimmed length - 1)
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

// ReadPooler::add_alignment (read_pooler.cpp:3-20): pools keyed by the exact sequence,
// numbered by first occurrence.
int32_t ltr_pool_reads(const uint8_t* const* seqs, const int32_t* seq_lens, int32_t n_reads, int32_t* pool_index) {
  if (n_reads < 0 || ((!seqs || !seq_lens || !pool_index) && n_reads > 0)) return LTR_ERR_INVALID;
  for (int32_t i = 0; i < n_reads; ++i) if (seq_lens[i] < 0 || (seq_lens[i] > 0 && !seqs[i])) return LTR_ERR_INVALID;
  // (the reference keys a std::map by the sequence; the same pools, in the same order, come out of an open-addressing
  // table of 64-bit hashes with the byte comparison only on a hash match -- no key copies, no tree of kilobase strings)
  auto hash_seq = [](const uint8_t* p, int32_t len) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)len;
    int32_t k = 0;
    for (; k + 8 <= len; k += 8) { uint64_t w; std::memcpy(&w, p + k, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    uint64_t w = 0;
    if (k < len) std::memcpy(&w, p + k, (size_t)(len - k));
    h = (h ^ w) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    return h;
  };
  size_t cap = 16;
  while (cap < (size_t)n_reads * 2) cap <<= 1;
  std::vector<int32_t> slot(cap, -1);                           // -> first read of the pool stored there
  std::vector<uint64_t> hashes((size_t)n_reads);
  int32_t n_pools = 0;
  for (int32_t i = 0; i < n_reads; ++i) {
    const uint64_t h = hashes[(size_t)i] = hash_seq(seqs[i], seq_lens[i]);
    size_t at = (size_t)h & (cap - 1);
    for (;; at = (at + 1) & (cap - 1)) {
      const int32_t f = slot[at];
      if (f < 0) { slot[at] = i; pool_index[i] = n_pools++; break; }
      if (hashes[(size_t)f] == h && seq_lens[f] == seq_lens[i] && (seq_lens[i] == 0 || std::memcmp(seqs[f], seqs[i], (size_t)seq_lens[i]) == 0)) {
        pool_index[i] = pool_index[f]; break;
      }
    }
  }
  return n_pools;
}

// SeqStutterGenotyper::calc_hap_aln_probs, the part after process_reads
// (seq_stutter_genotyper.cpp:526-559).
int ltr_scatter_pool_probs(const double* log_pool_aln_probs, const int32_t* pool_seed_positions,
                           const int32_t* pool_index, int32_t n_reads, int32_t n_alleles,
                           const uint8_t* realign_to_hap, const uint8_t* copy_read, const uint8_t* second_mate,
                           double* log_aln_probs, int32_t* seed_positions) {
  if (!log_pool_aln_probs || !pool_index || !log_aln_probs || n_reads < 0 || n_alleles <= 0) return LTR_ERR_INVALID;
  for (int32_t i = 0; i < n_reads; ++i) {                      // :527-538
    if (copy_read && !copy_read[i]) continue;
    if (seed_positions && pool_seed_positions) seed_positions[i] = pool_seed_positions[pool_index[i]];
    const double* src = log_pool_aln_probs + (int64_t)n_alleles * pool_index[i];
    double* dst = log_aln_probs + (int64_t)n_alleles * i;
    for (int32_t j = 0; j < n_alleles; ++j) if (!realign_to_hap || realign_to_hap[j]) dst[j] = src[j];
  }
  return ltr::sum_mate_rows(log_aln_probs, n_reads, n_alleles, second_mate, copy_read, realign_to_hap);
}

// ---- host-thread budget (ltr_internal.h; reference README.md:78-82: one thread per process, N processes per node) ----
int ltr_ctx_set_host_threads(ltr_ctx* ctx, int n) {
  if (!ctx || n < 0 || n > (1 << 16)) { if (ctx) ltr::set_error(ctx, "ltr_ctx_set_host_threads: n >= 1 (the budget) or 0 (the rule)"); return LTR_ERR_INVALID; }
  ltr::host_thread_setting().store(n, std::memory_order_relaxed);
  return LTR_OK;
}
int ltr_ctx_host_threads(const ltr_ctx* ctx) { return ctx ? ltr::host_thread_budget() : LTR_ERR_INVALID; }
int ltr_host_threads_rule(int local_world_size) { return ltr::host_threads_rule(local_world_size); }

// test hook (no GPU): the number of distinct threads a loop of n items really ran on under a budget of `n_threads` (0: the rule).
// The budget is handed to the loop; the process's setting is not touched.
int ltr_debug_parallel_threads(int n_threads, int64_t n_items, int which_pool) {
  if (n_threads < 0 || n_items < 0) return LTR_ERR_INVALID;
  std::mutex mu;
  std::vector<std::thread::id> seen;
  try {
    ltr::parallel_for_on(n_threads > 0 ? std::min(n_threads, ltr::kMaxHostThreads) : ltr::host_threads_rule(0), n_items, 1, [&](int64_t) {
      const std::thread::id me = std::this_thread::get_id();
      {
        std::lock_guard<std::mutex> lk(mu);
        if (std::find(seen.begin(), seen.end(), me) == seen.end()) seen.push_back(me);
      }
      std::this_thread::sleep_for(std::chrono::microseconds(200));       // (long enough for every thread of the team to take a share)
    }, 1, which_pool);
    return (int)seen.size();
  } catch (...) { return LTR_ERR_NOMEM; }
}

}  // extern "C"
