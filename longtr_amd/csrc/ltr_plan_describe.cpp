// ltr_plan_describe.cpp -- describe_batch, the host half of ltr_plan_create (ltr_plan.h): the batch validated, its bytes
// scanned, one descriptor, class and key per pair, the families formed, the pairs sorted.

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <cstring>

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace ltrp {

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

// Whole rounds of four-wave workgroups for the reads of 3.6 - 5.1 kb, the rest of them on eight waves (make_rules): the
// pairs beyond the quota -- the last ones in batch order -- move to the eight-wave class of their length.
static void move_beyond_quota_to_eight_waves(const int64_t quota, const BatchScratch& w) {
  int64_t seen = 0;
  for (size_t i = 0; i < w.pairs.size(); ++i) {
    const int k = w.bin[i];
    if (k < kWg4First + (ltrp::kWg4WideMinW - kWg4MinW) || k >= kWg8First) continue;
    if (++seen <= quota) continue;
    const int C = w.pairs[i].m - 1;
    w.bin[i] = (int16_t)(kWg8First + std::max((C + 511) / 512, kWg8MinW) - kWg8MinW);
  }
}

// d->fams: the families in the order the sort left their members in: a family's members are one run of the family class, its first
// member first (input order inside a key).  Three passes: which sorted pairs are a family's first member (all host cores: a lookup by
// batch position), the list of those runs (serial, a scan of one int per member), then every family's records written at their
// final place (all host cores: the records are read in sorted order, which is scattered over the family list and the spine lists).
static int resolve_families(const std::vector<FamilyRec>& fam_recs, const FamilySide& side, const BatchScratch& w, BatchPlan* d, std::string* err) {
  const RawBuf<PairDesc>& sorted = w.sorted;
  d->fams.clear(); d->fam_U.clear(); d->fam_members = 0;
  d->fam_spines.clear(); d->fam_forks.clear(); d->fam_with_spine = d->fam_rows_saved = 0;
  const int f0 = d->bin_first[kFamClass], f1 = d->bin_first[kFamClass + 1];
  if (f1 <= f0) return LTR_OK;
  std::vector<int32_t> rec_of_pair(w.pairs.size(), -1);            // batch position of a family's first member -> its record
  ltr::parallel_for((int64_t)fam_recs.size(), 4096, [&](int64_t r) { rec_of_pair[(size_t)fam_recs[(size_t)r].first_pair] = (int32_t)r; });
  std::vector<int32_t> rec_at((size_t)(f1 - f0));
  ltr::parallel_for((int64_t)(f1 - f0), 4096, [&](int64_t k) { rec_at[(size_t)k] = rec_of_pair[(size_t)w.order[(size_t)(f0 + k)]]; });
  std::vector<int32_t> first_at; first_at.reserve(fam_recs.size() + 1);
  for (int k = 0; k < f1 - f0; ++k) if (rec_at[(size_t)k] >= 0) first_at.push_back(k);
  const size_t nf = first_at.size();
  first_at.push_back(f1 - f0);
  FamilySpine plain;
  std::memset(&plain, 0, sizeof(plain));
  plain.spine = -1;
  d->fams.resize(nf); d->fam_U.resize(nf); d->fam_spines.resize(nf);
  if (d->keep_forks) d->fam_forks.resize(nf);
  std::atomic<int> bad((nf == 0 && f1 > f0) || (nf > 0 && first_at[0] != 0) ? 1 : 0);
  std::vector<int32_t> saved(nf, 0);                               // modelled steps a family's spine saves
  ltr::parallel_for((int64_t)nf, 1024, [&](int64_t j) {
    const int i = f0 + first_at[(size_t)j];
    const FamilyRec& rec = fam_recs[(size_t)rec_at[(size_t)first_at[(size_t)j]]];
    bool ok = first_at[(size_t)j + 1] - first_at[(size_t)j] == rec.f.count;      // (its run ends where the next family's begins)
    for (int k = 0; ok && k < rec.f.count; ++k)
      ok = sorted[(size_t)(i + k)].read_off == sorted[(size_t)i].read_off && sorted[(size_t)(i + k)].m == sorted[(size_t)i].m && sorted[(size_t)(i + k)].n - 1 >= rec.f.p;
    if (!ok) { bad.store(1, std::memory_order_relaxed); return; }
    FamilyDesc f = rec.f;
    f.first = i;
    d->fams[(size_t)j] = f; d->fam_U[(size_t)j] = rec.U;
    d->fam_spines[(size_t)j] = rec.spine_at < 0 ? plain : side.sp[(size_t)rec.locus][(size_t)rec.spine_at];
    if (rec.spine_at >= 0) saved[(size_t)j] = rec.plain_steps - rec.steps;
    if (d->keep_forks) {
      FamilyForks fk;
      std::memset(&fk, 0, sizeof(fk));
      fk.steps = rec.steps;
      if (rec.spine_at >= 0) std::memcpy(fk.fork, side.fork[(size_t)rec.locus].data() + (size_t)rec.spine_at * kFamilyMaxMembers, sizeof(fk.fork));
      d->fam_forks[(size_t)j] = fk;
    }
  });
  if (bad.load()) {
    d->fams.clear(); d->fam_U.clear(); d->fam_spines.clear(); d->fam_forks.clear();
    *err = "internal error: a haplotype family's members are not contiguous in the sorted pair list"; return LTR_ERR_INVALID;
  }
  for (size_t j = 0; j < nf; ++j) { d->fam_members += d->fams[j].count; d->fam_with_spine += d->fam_spines[j].spine >= 0; d->fam_rows_saved += saved[j]; }
  return LTR_OK;
}

int describe_batch(const ltr_locus_batch* b, const ModelConsts& mc, const int F, const int mode, const int n_cu, const ltr::DebugKnobs& dbg,
                   const BatchScratch& w, BatchPlan* d, std::string* err) {
  if (b->n_loci < 0 || b->n_reads < 0 || b->n_haps < 0) { *err = "negative counts"; return LTR_ERR_INVALID; }
  if (b->n_loci > 0 && (!b->locus_read_off || !b->locus_hap_off || !b->read_off || !b->hap_off)) { *err = "null offset array"; return LTR_ERR_INVALID; }
  // ---- what the batch as a whole decides: packing, workgroup kernels, exact kernel flavour (ltrp::make_rules) ----
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
  FamilySide fam_side;
  fam_side.keep_forks = d->keep_forks;
  if (d->use_plan && rules.sym_model && dbg.families >= 0)
    form_families(b, mc, F, n_cu, dbg.families, dbg.family_min_rows > 0 ? dbg.family_min_rows : kFamMinRows, dbg.family_spine, pair_base, w, &fam_recs, &fam_side);
  if (rules.wg_wide4 && rules.wide4_quota != INT64_MAX) move_beyond_quota_to_eight_waves(rules.wide4_quota, w);
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
  return resolve_families(fam_recs, fam_side, w, d, err);
}

}  // namespace ltrp
