// ltr_hap_aln.cpp -- SeqStutterGenotyper::calc_hap_aln_probs (seq_stutter_genotyper.cpp:514-563) for MANY loci in one GPU pass:
// ltr_calc_hap_aln_probs, in stages over one per-call struct (HapAlnCall).  The per-locus primitives are ltr_host.cpp's.
//
// Per locus, like the reference: pool the reads (ReadPooler, read_pooler.cpp:3-20: exact sequence, the pool keeps the
// FIRST read's start/stop/CIGAR), trim each pool (HapAligner::trim_alignment), score every pool x haplotype pair, fan
// the pool rows out to the reads and sum mate-pair rows (:526-559).  Period-1 loci under --stutter-align-len take the
// short path with the pools' median base qualities (ReadPooler::pool, read_pooler.h:42-48).
//
// What is added here -- none of it changes a bit of the result:
//  * the long-path score of a pair is a function of the TRIMMED read's bytes and the haplotype's alone
//    (HapAligner.cpp:236-343), and pools that differ only outside the trimmed window (a sequencing error in the
//    +-200 bp of flank a HiFi read carries) trim to the same bytes: the pools of a locus are de-duplicated by their
//    trimmed bytes, each distinct trimmed read is scored once, and its row is copied to every pool that shares it
//    (30x HiFi over a 20-bp repeat: ~18 pools, ~5 distinct trimmed reads);
//  * no per-locus heap traffic: the per-read / per-pool results of a chunk live in flat arrays indexed by the prefix sum
//    of the loci's read counts, hash tables and CIGAR scratch are per worker thread;
//  * chunks of loci: while the GPU scores chunk c the host cores prepare chunk c+1.

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "ltr_internal.h"

namespace {

// Keys of the pooling tables: equal bytes -> equal hash is all that is needed (a hit is confirmed by memcmp).  Four
// independent multiply-xor lanes over 32-byte blocks: one lane's chain (load, xor, 64-bit multiply, shift-xor) is ~6 cycles
// per 8 bytes, and hashing the 390 MB of raw reads of a 30 000-locus call with ONE chain was the longest host phase of
// ltr_calc_hap_aln_probs (3.3 ms of 9 per 10 000-locus chunk on 16 cores).
inline uint64_t hash_bytes(const uint8_t* p, int64_t len) {
  constexpr uint64_t k0 = 0xFF51AFD7ED558CCDull, k1 = 0xC4CEB9FE1A85EC53ull, k2 = 0x9E3779B97F4A7C15ull, k3 = 0xD6E8FEB86659FD93ull;
  uint64_t h0 = k2 ^ (uint64_t)len, h1 = k0, h2 = k1, h3 = k3;
  int64_t k = 0;
  for (; k + 32 <= len; k += 32) {
    uint64_t w0, w1, w2, w3;
    std::memcpy(&w0, p + k, 8); std::memcpy(&w1, p + k + 8, 8); std::memcpy(&w2, p + k + 16, 8); std::memcpy(&w3, p + k + 24, 8);
    h0 = (h0 ^ w0) * k0; h0 ^= h0 >> 32;
    h1 = (h1 ^ w1) * k1; h1 ^= h1 >> 32;
    h2 = (h2 ^ w2) * k2; h2 ^= h2 >> 32;
    h3 = (h3 ^ w3) * k3; h3 ^= h3 >> 32;
  }
  uint64_t h = ((h0 * k1) ^ (h1 >> 29)) + ((h2 * k3) ^ (h3 >> 31)) + (h1 << 17) + h3;
  for (; k + 8 <= len; k += 8) { uint64_t w; std::memcpy(&w, p + k, 8); h = (h ^ w) * k0; h ^= h >> 32; }
  uint64_t w = 0;
  if (k < len) std::memcpy(&w, p + k, (size_t)(len - k));
  h = (h ^ w) * k1; h ^= h >> 29;
  return h;
}

struct WorkerScratch {                     // one per host thread, kept between loci and calls
  std::vector<int32_t> slot;               // open-addressing table: -> item index, -1 empty
  std::vector<int32_t> used;               // slots written for the current locus (reset list)
  std::vector<uint64_t> hashes;
  std::vector<int32_t> cigar_rem;
  std::vector<int32_t> counts;             // haplotype_counts
  void table(size_t n_items) {
    size_t cap = 64;
    while (cap < n_items * 2) cap <<= 1;
    if (slot.size() < cap) slot.assign(cap, -1);
    if (hashes.size() < n_items) hashes.resize(n_items);
  }
  void reset() { for (int32_t at : used) slot[(size_t)at] = -1; used.clear(); }
};
WorkerScratch& scratch() { static thread_local WorkerScratch W; return W; }

struct LocusInfo {
  int32_t rc = LTR_OK; const char* err = nullptr;
  int32_t rb = -1, P = 0, U = 0; int64_t H = 0;
  bool short_path = false;
  int64_t rbytes = 0, hbytes = 0;          // trimmed bytes of the distinct reads / haplotype string bytes
  int64_t ubase = 0, hbase = 0, rbyte0 = 0, hbyte0 = 0, ll0 = 0;   // prefix sums inside the chunk (long-path loci only)
};

// Per read: its pool; per pool (stored at the locus's read base + pool number): first read, trim, distinct trimmed read.  One
// allocation for the call (uninitialised: every entry is written by prepare_locus before it is read); of(rb0) = the six
// columns of the locus whose reads start at rb0.
struct LocusPools {
  int32_t* index;        // [read]  -> pool
  int32_t* first;        // [pool]  -> its first read
  int32_t* lt;           // [pool]  ltrim; -1: empty trim -> the 5 + 5 flank bases (:820-823)
  int32_t* len;          // [pool]  trimmed length
  int32_t* uniq;         // [pool]  distinct trimmed read of the pool, -1: not realigned
  int32_t* uniq_pool;    // [distinct trimmed read] -> its first pool
};
struct PoolTable {
  std::unique_ptr<int32_t[]> cells; int64_t n = 0;
  void alloc(int64_t n_reads) { n = std::max<int64_t>(n_reads, 1); cells.reset(new int32_t[(size_t)(6 * n)]); }
  LocusPools of(int64_t rb0) const { int32_t* p = cells.get() + rb0; return {p, p + n, p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n}; }
};

// BaseQuality::median_base_qualities (base_quality.cpp:11-28): per position, the upper median
std::vector<uint8_t> median_qualities(const std::vector<const ltr_alignment*>& members) {
  const int32_t len = members[0]->seq_len;
  std::vector<uint8_t> out((size_t)len, 'N'), col;
  if (members.size() == 2) {                                          // upper median of two: the larger
    for (int32_t i = 0; i < len; ++i) { const char x = (char)members[0]->qual[i], y = (char)members[1]->qual[i]; out[(size_t)i] = (uint8_t)(x < y ? y : x); }
    return out;
  }
  for (int32_t i = 0; i < len; ++i) {
    col.clear();
    for (const ltr_alignment* m : members) col.push_back((uint8_t)(char)m->qual[i]);
    std::sort(col.begin(), col.end(), [](uint8_t x, uint8_t y) { return (char)x < (char)y; });
    out[(size_t)i] = col[col.size() / 2];
  }
  return out;
}

// a period-1 locus under use_short_path: prepared like the others on the host's cores -- pools' median qualities, its own
// little batch of the seeded path (ltr_short.hip) -- and strung onto the call's batch in locus order
struct ShortBatchDel { void operator()(ltr::ShortBatch* p) const { ltr::short_batch_free(p); } };
struct ShortLocus {
  int64_t locus = 0, H = 0; std::vector<double> pool_probs; std::vector<int32_t> pool_seeds;
  std::unique_ptr<ltr::ShortBatch, ShortBatchDel> batch;
};

struct PlanDel { void operator()(ltr_plan* p) const { ltr_plan_destroy(p); } };
// chunks of loci: while the GPU scores chunk c the host prepares chunk c+1
struct Chunk {
  int64_t l0 = 0, l1 = 0;                     // loci [l0, l1)
  std::vector<int64_t> read_off, hap_off, lro, lho;
  std::vector<uint8_t> mask_h;
  std::vector<int64_t> slot_locus;            // long-path loci of the chunk, in order
  std::unique_ptr<ltr_plan, PlanDel> plan;    // (the one owner: destroyed with the chunk, whichever way the call ends)
  std::unique_ptr<double[]> ll;
  // what staging the chunk leaves for the calling thread
  int64_t n_u = 0, n_h = 0, n_rb = 0, n_hb = 0;
  bool any_mask = false;
  uint8_t* read_bytes = nullptr; uint8_t* hap_bytes = nullptr;
  std::vector<int64_t> short_l;               // short-path loci of the chunk before its first error, in order
  int rc = LTR_OK; const char* err = nullptr; // the chunk's first error in locus order
};

// The chunk rule: where the chunks begin, the streams their plans alternate between, and whether chunk c + 1 is staged by a thread
// of its own (on ahead_threads threads) while the calling thread plans chunk c.  A pure function of its arguments (plan_chunks).
struct ChunkPlan { std::vector<int64_t> bounds; int n_streams = 2; bool prep_ahead = false; int ahead_threads = 1; };

// One call.  The ORDER of the members is the lifetime rule: they are destroyed last to first, so the helper thread (`ahead`, last)
// is joined first, then the chunks go with their plans, and only then the arrays the helper wrote into (info, pools, read_base);
// the call lock, first, is released last.  Params, knobs and the thread budget are read once, under the lock.
struct HapAlnCall {
  // one call at a time per context (the chunks are staged in the context's host arrays): a second host thread waits here
  const std::unique_lock<std::mutex> call_lock;
  ltr_ctx* const ctx; const ltr_locus* const loci; const int64_t n_loci;
  double* const* const log_aln_probs; int32_t* const* const seed_positions;
  const ltr_align_params prm; const ltr::DebugKnobs knobs;
  const int budget;                                             // the host-thread budget of every loop of this call
  const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  std::vector<int64_t> read_base;                               // prefix sum of the loci's read counts
  PoolTable pools;
  std::vector<LocusInfo> info;
  std::vector<std::unique_ptr<ShortLocus>> short_of;            // (heap objects: the queued result pointers stay valid)
  std::vector<ShortLocus*> short_loci;                          // ... in locus order
  std::unique_ptr<ltr::ShortBatch, ShortBatchDel> short_batch;
  ChunkPlan plan;
  std::vector<Chunk> chunks;
  // (set when the call is on its way out with an error: a chunk being staged ahead stops pooling and trimming loci nobody will score)
  std::atomic<bool> cancel{false};
  struct Ahead {
    std::atomic<bool>& cancel; std::thread th; std::exception_ptr err; bool done = false;
    explicit Ahead(std::atomic<bool>& flag) : cancel(flag) {}
    void join() { if (th.joinable()) th.join(); }
    ~Ahead() { if (!done) cancel.store(true); join(); }         // (an early exit: the thread stops at its next locus)
  } ahead{cancel};

  HapAlnCall(ltr_ctx* c, const ltr_locus* l, int64_t n, double* const* probs, int32_t* const* seeds)
      : call_lock(ltr::ctx_call_lock(c)), ctx(c), loci(l), n_loci(n), log_aln_probs(probs), seed_positions(seeds), prm(ltr::ctx_params(c)),
        knobs(ltr::ctx_debug(c)), budget(ltr::host_thread_budget()) {}
  __attribute__((format(printf, 2, 3))) void mark(const char* fmt, ...) const {
    if (!knobs.trace) return;
    std::fprintf(stderr, "[ltr] calc_hap_aln_probs %8.2f ms: ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
    std::fprintf(stderr, "\n");
  }
};

// ---- validation: the loci here, their alignment records where they are first read (prepare_locus, on all host cores) ----
int validate_loci(HapAlnCall& c) {
  c.read_base.assign((size_t)c.n_loci + 1, 0);
  for (int64_t l = 0; l < c.n_loci; ++l) {
    const ltr_locus& L = c.loci[l];
    if (!L.hap || (!L.alns && L.n_alns > 0) || L.n_alns < 0 || !c.log_aln_probs[l] || !c.seed_positions[l]) return LTR_ERR_INVALID;
    c.read_base[(size_t)l + 1] = c.read_base[(size_t)l] + L.n_alns;
  }
  c.pools.alloc(c.read_base[(size_t)c.n_loci]);
  c.info.resize((size_t)c.n_loci); c.short_of.resize((size_t)c.n_loci);
  c.mark("validated %ld loci, %ld reads", (long)c.n_loci, (long)c.read_base[(size_t)c.n_loci]);
  return LTR_OK;
}

// ---- per locus, on all host cores: pools, trims, distinct trimmed reads, sizes ---------------------
// ReadPooler::add_alignment: pools keyed by the exact sequence, numbered by first occurrence
int32_t pool_locus_reads(const ltr_locus& L, const LocusPools& p, WorkerScratch& W) {
  W.table((size_t)std::max(L.n_alns, 1));
  int32_t P = 0;
  const size_t mask = W.slot.size() - 1;
  for (int32_t i = 0; i < L.n_alns; ++i) {
    const ltr_alignment& A = L.alns[i];
    const uint64_t h = W.hashes[(size_t)i] = hash_bytes(A.seq, A.seq_len);
    for (size_t at = (size_t)h & mask;; at = (at + 1) & mask) {
      const int32_t f = W.slot[at];
      if (f < 0) { W.slot[at] = i; W.used.push_back((int32_t)at); p.first[P] = i; p.index[i] = P++; break; }
      if (W.hashes[(size_t)f] == h && L.alns[f].seq_len == A.seq_len && (A.seq_len == 0 || std::memcmp(L.alns[f].seq, A.seq, (size_t)A.seq_len) == 0)) {
        p.index[i] = p.index[f]; break;
      }
    }
  }
  W.reset();
  return P;
}

// per-locus short path on the pooled alignments (ReadPooler::pool: the pool's reads with their median qualities, read_pooler.h:42-48)
void prepare_short_locus(HapAlnCall& c, int64_t l, const LocusPools& p) {
  const ltr_locus& L = c.loci[l];
  LocusInfo& I = c.info[(size_t)l];
  const int32_t P = I.P;
  std::vector<ltr_alignment> pooled((size_t)P);
  std::vector<std::vector<uint8_t>> quals((size_t)P);
  for (int32_t q = 0; q < P; ++q) {
    pooled[(size_t)q] = L.alns[p.first[q]];
    std::vector<const ltr_alignment*> members;
    for (int32_t i = 0; i < L.n_alns; ++i) if (p.index[i] == q) members.push_back(&L.alns[i]);
    for (const ltr_alignment* m : members) if (!m->qual) { I.err = "short path needs base qualities"; I.rc = LTR_ERR_INVALID; return; }
    if (members.size() == 1) continue;                            // (a pool of one read: its own qualities, already in place)
    quals[(size_t)q] = median_qualities(members);
    pooled[(size_t)q].qual = quals[(size_t)q].data();
  }
  std::unique_ptr<ShortLocus> SL(new ShortLocus());
  SL->locus = l; SL->H = ltr_haplotype_num_combs(L.hap);
  SL->pool_probs.assign((size_t)P * (size_t)SL->H, 0.0); SL->pool_seeds.assign((size_t)P, 0);
  SL->batch.reset(ltr::short_batch_new());
  // queued: every short-path locus of the call is scored in ONE set of launches after the chunks are on their way
  const int rc2 = ltr::short_batch_add(c.ctx, SL->batch.get(), L.hap, L.realign_to_hap, pooled.data(), P, 0, L.realign_pool,
                                       SL->pool_probs.data(), SL->pool_seeds.data());
  if (rc2 != LTR_OK) { I.rc = rc2; I.err = nullptr; return; }       // (the message is the one short_batch_add left in the context)
  c.short_of[(size_t)l] = std::move(SL);
}

// haplotype count and bytes; trims (HapAligner.cpp:819), then the distinct trimmed reads among the realigned pools
void size_and_trim_locus(HapAlnCall& c, int64_t l, const LocusPools& p, WorkerScratch& W) {
  const ltr_locus& L = c.loci[l];
  LocusInfo& I = c.info[(size_t)l];
  if (ltr::haplotype_sizes(L.hap, &W.counts, &I.H, &I.hbytes) != LTR_OK) { I.err = "bad haplotype block structure"; I.rc = LTR_ERR_INVALID; return; }
  const int32_t sub_len = ltr::empty_trim_len(L.hap);
  W.table((size_t)std::max(I.P, 1));
  const size_t mask = W.slot.size() - 1;
  int32_t U = 0, sub_uniq = -1;
  int64_t rbytes = 0;
  for (int32_t q = 0; q < I.P; ++q) {
    p.uniq[q] = -1; p.lt[q] = 0; p.len[q] = 0;
    if (L.realign_pool && !L.realign_pool[q]) continue;              // not realigned: no pair, its rows stay as they are
    const ltr_alignment& A = L.alns[p.first[q]];
    if ((size_t)std::max(A.n_cigar, 1) > W.cigar_rem.size()) W.cigar_rem.resize((size_t)A.n_cigar * 2);
    int32_t lt = 0, rt = 0;
    const int rc = ltr::trim_alignment_into(&A, L.hap->block_start[I.rb], L.hap->block_end[I.rb], c.prm.indel_flank_len, W.cigar_rem.data(), &lt, &rt);
    if (rc != LTR_OK) { I.err = ltr::trim_error_text(rc); I.rc = rc; W.reset(); return; }
    const int32_t len = A.seq_len - lt - rt;
    if (len <= 0) {                                                  // empty trim: one substitute read for all such pools of the locus
      if (sub_len < 0) { I.err = ltr::kShortLeftFlank; I.rc = LTR_ERR_INVALID; W.reset(); return; }
      p.lt[q] = -1; p.len[q] = sub_len;
      if (sub_uniq < 0) { sub_uniq = U; p.uniq_pool[U] = q; ++U; rbytes += sub_len; }
      p.uniq[q] = sub_uniq;
      continue;
    }
    p.lt[q] = lt; p.len[q] = len;
    const uint8_t* tb = A.seq + lt;
    const uint64_t h = W.hashes[(size_t)q] = hash_bytes(tb, len);
    for (size_t at = (size_t)h & mask;; at = (at + 1) & mask) {
      const int32_t f = W.slot[at];                                   // -> a pool whose trimmed read is distinct so far
      if (f < 0) { W.slot[at] = q; W.used.push_back((int32_t)at); p.uniq_pool[U] = q; p.uniq[q] = U++; rbytes += len; break; }
      if (W.hashes[(size_t)f] == h && p.len[f] == len && std::memcmp(L.alns[p.first[f]].seq + p.lt[f], tb, (size_t)len) == 0) { p.uniq[q] = p.uniq[f]; break; }
    }
  }
  W.reset();
  I.U = U; I.rbytes = rbytes;
}

void prepare_locus(HapAlnCall& c, int64_t l) {
  WorkerScratch& W = scratch();
  const ltr_locus& L = c.loci[l];
  LocusInfo& I = c.info[(size_t)l];
  const LocusPools p = c.pools.of(c.read_base[(size_t)l]);
  // (checked here, chunk by chunk, not in a pass of its own over the 900 000 records of a 30 000-locus call before anything else
  // starts -- 1.2 ms with the GPU idle; nothing is written to the caller's matrices before every chunk is through here, except
  // the rows of short-path loci, as with every other error prepare_locus finds)
  for (int32_t i = 0; i < L.n_alns; ++i)
    if (!ltr::alignment_record_ok(L.alns[i])) { I.err = ltr::kBadAlignmentRecord; I.rc = LTR_ERR_INVALID; return; }
  for (int b = 0; b < L.hap->n_blocks; ++b) if (L.hap->is_repeat[b]) { I.rb = b; break; }
  if (L.hap->n_blocks <= 0 || I.rb < 0) { I.err = "haplotype has no repeat block"; I.rc = LTR_ERR_INVALID; return; }
  I.P = pool_locus_reads(L, p, W);
  I.short_path = c.prm.use_short_path && L.hap->n_blocks > 1 && L.hap->period[1] == 1;      // HapAligner.cpp:552
  if (I.short_path) prepare_short_locus(c, l, p);
  else size_and_trim_locus(c, l, p, W);
}

// ---- the chunk rule ----
// DP cells of the call, estimated from what is known before any read is touched -- reads, alleles and allele lengths -- on every
// 16th locus.  (Made before prepare_locus validates the blocks: a malformed locus is skipped here and rejected there.)
constexpr int64_t kEstimateMinLoci = 6000;                            // below: the estimate is not read (plan_chunks)
double estimate_cells(const ltr_locus* loci, int64_t n_loci) {
  double cells = 0.0;
  if (n_loci < kEstimateMinLoci) return cells;
  for (int64_t l = 0; l < n_loci; l += 16) {
    const ltr_haplotype_blocks* hb = loci[l].hap;
    if (!hb || hb->n_blocks <= 0) continue;
    int64_t hap_len = 0, H = 1, k = 0;
    bool ok = hb->n_alleles && hb->allele_off;
    for (int b = 0; ok && b < hb->n_blocks; ++b) {
      const int na = hb->n_alleles[b];
      if (na <= 0 || na > (1 << 24) || H > (1 << 24)) { ok = false; break; }
      hap_len += hb->allele_off[k + 1] - hb->allele_off[k]; H *= na; k += na;
    }
    if (!ok) continue;
    const double side = (double)std::max<int64_t>(hap_len - 60, 1);
    cells += 16.0 * (double)std::max(loci[l].n_alns, 1) / 3.0 * (double)std::min<int64_t>(H, 1 << 20) * side * side;   // (about a third of the reads survive pooling + trimming)
  }
  return cells;
}

// Two chunks, 1 : 3 -- the GPU starts on the first quarter while the host cores prepare the rest; the plans
// run on two streams, so the tail of the first plan's launches overlaps the head of the second's.
// Measured on MI355X (round 2), 6000 raw config-3 loci: one plan 210.5 ms per call; 1 : 1 202.7; 1 : 2 197.6; 1 : 3
// 194.9; three chunks 1 : 2 : 3 202.9; eight chunks on three streams 233 (every plan is a chain of launches, each at
// least as long as its longest pair: small plans leave the GPU part empty).  1000 loci: one plan 45.6 ms, two 46.5.
// (ltr_ctx_set_debug "chunks" / "chunk_streams" / "chunk_growth" override the rule: tests/manual/gpu_chunk_sweep.py.)
// (When the call is host-bound -- a catalogue of short repeats: ~1 microsecond of host work per locus, a few hundred
// nanoseconds of DP -- three equal chunks keep the GPU fed: 30 000 catalogue loci 42.8 ms as 1 : 3, 37.8 ms as 1 : 1 : 1;
// config 3 / config3skew, where the DP is the longer side, lose 4 - 8 % that way.  The split is decided on an estimate of
// both sides: estimate_cells.)
ChunkPlan plan_chunks(int64_t n_loci, double est_cells, const ltr::DebugKnobs& knobs, int budget) {
  // Chunk c + 1 is pooled, trimmed and laid out by a thread of its own (with the second worker pool, into the second pair of staging
  // arrays) WHILE the calling thread plans and launches chunk c: planning has serial stretches (prefix sums, the sort's merge, the
  // uploads) that leave the host cores idle, and on a catalogue of short repeats the host, not the GPU, is the longer side of every
  // chunk.  Measured on MI355X, 30 000 catalogue loci (tests/manual/gpu_prep_ahead_ab.py): profiles/r05/e2e_prep_ahead.log.
  // Round 6: only from a host-thread budget of 12 up (ltr_ctx_set_host_threads; rule: affinity mask, cgroup quota, ranks on this
  // host) -- two thread teams on four or eight cores are slower than one (same log: 55.8 / 35.0 ms against 30.2 with the helper off).
  const bool helper = knobs.prep_ahead > 0 || (knobs.prep_ahead == 0 && budget >= ltr::kPrepAheadMinThreads);
  int64_t n_chunks = n_loci >= 1500 ? 2 : 1;
  double growth = 3.0;                                                // 0: weights 1, 2, 3, ...; g > 0: 1, g, g^2, ...; g < 0: 1, 2, .., k, k, .., 2, 1
  if (n_loci >= kEstimateMinLoci && est_cells / 2.5e12 < 1.5 * ((double)n_loci * 0.8e-6)) {     // GPU seconds < 1.5 x host seconds
    n_chunks = 3; growth = 1.0;
    // (Round 5: with the next chunk staged ahead by a thread of its own, DMA-only uploads and a cheaper plan creation the host
    // side of a chunk is SHORTER than its GPU side -- 0.45 + 0.27 microseconds per locus on two threads against 0.65 -- and the
    // lead-in, the first chunk's staging + planning with the GPU idle, is what is left to shorten: a first chunk of ~2400 loci,
    // every next one 1.3 x longer (the growth at which staging + planning chunk c + 1 still fits under chunk c's launch).
    // Measured on MI355X, 30 000 catalogue loci, tests/manual/gpu_chunk_sweep_ahead.py: three equal chunks 30.3 - 31.5 ms per
    // call; 4 / 5 / 6 / 8 chunks at 1.3: 26.5 - 27.8 / 26.2 - 26.4 / 25.7 - 26.0 / 27.2 - 27.6; growth 1.5 - 1.6: 27.9 - 30.2;
    // without the thread three equal chunks stay the best, 30.1 - 33.4 against 33.7 - 34.3 for 4 - 5 chunks at 1.3.)
    if (helper) {
      growth = 1.3;
      while (n_chunks < 8 && 2400.0 * (std::pow(1.3, (double)n_chunks) - 1.0) / 0.3 < (double)n_loci) ++n_chunks;
    }
  }
  ChunkPlan P;
  if (knobs.chunks > 0) n_chunks = std::max<int64_t>(1, std::min<int64_t>(knobs.chunks, std::max<int64_t>(n_loci, 1)));
  if (knobs.chunk_streams > 0) P.n_streams = knobs.chunk_streams;
  if (knobs.chunk_growth_set) growth = knobs.chunk_growth;
  std::vector<double> cum((size_t)n_chunks + 1, 0.0);                 // cumulative chunk weights
  double w = 1.0;
  for (int64_t k = 0; k < n_chunks; ++k) {
    const double wk = growth > 0.0 ? w : (growth < 0.0 ? (double)(std::min(k, n_chunks - 1 - k) + 1) : (double)(k + 1));
    cum[(size_t)k + 1] = cum[(size_t)k] + wk; w *= growth;
  }
  P.bounds.assign((size_t)n_chunks + 1, n_loci);
  for (int64_t k = 0; k < n_chunks; ++k) P.bounds[(size_t)k] = (int64_t)((double)n_loci * cum[(size_t)k] / cum[(size_t)n_chunks]);
  P.prep_ahead = n_chunks > 1 && helper;
  P.ahead_threads = knobs.prep_ahead > 0 ? knobs.prep_ahead : budget;
  return P;
}
void plan_chunks(HapAlnCall& c) {
  c.plan = plan_chunks(c.n_loci, estimate_cells(c.loci, c.n_loci), c.knobs, c.budget);
  c.chunks.resize(c.plan.bounds.size() - 1);
  for (size_t k = 0; k < c.chunks.size(); ++k) { c.chunks[k].l0 = c.plan.bounds[k]; c.chunks[k].l1 = c.plan.bounds[k + 1]; }
}

// ---- staging a chunk (the calling thread, or the helper thread for the chunk after the one being planned) ----
// in locus order: the first error ends the chunk; short-path loci are noted for the calling thread; prefix sums place the rest
void order_chunk(HapAlnCall& c, Chunk& C) {
  int64_t n_ll = 0;
  for (int64_t l = C.l0; l < C.l1; ++l) {
    LocusInfo& I = c.info[(size_t)l];
    if (I.rc != LTR_OK) { C.err = I.err; C.rc = I.rc; return; }
    if (I.short_path) { C.short_l.push_back(l); continue; }
    I.ubase = C.n_u; I.hbase = C.n_h; I.rbyte0 = C.n_rb; I.hbyte0 = C.n_hb; I.ll0 = n_ll;
    C.n_u += I.U; C.n_h += I.H; C.n_rb += I.rbytes; C.n_hb += I.hbytes; n_ll += (int64_t)I.U * I.H;
    C.any_mask |= (c.loci[l].realign_to_hap != nullptr);
    C.slot_locus.push_back(l);
  }
}

// the chunk's batch: bytes and offsets written in place, all cores
void layout_chunk(HapAlnCall& c, Chunk& C, int64_t index, int pool, int threads) {
  C.read_bytes = ltr::ctx_host_bytes(c.ctx, 2 * (int)(index & 1), (size_t)std::max<int64_t>(C.n_rb, 1));
  C.hap_bytes = ltr::ctx_host_bytes(c.ctx, 2 * (int)(index & 1) + 1, (size_t)std::max<int64_t>(C.n_hb, 1));
  const int64_t n_slots = (int64_t)C.slot_locus.size();
  C.read_off.resize((size_t)C.n_u + 1); C.hap_off.resize((size_t)C.n_h + 1); C.lro.resize((size_t)n_slots + 1); C.lho.resize((size_t)n_slots + 1);
  if (C.any_mask) C.mask_h.assign((size_t)C.n_h, 1);
  C.read_off[(size_t)C.n_u] = C.n_rb; C.hap_off[(size_t)C.n_h] = C.n_hb; C.lro[(size_t)n_slots] = C.n_u; C.lho[(size_t)n_slots] = C.n_h;
  ltr::parallel_for_on(threads, n_slots, 64, [&c, &C](int64_t k) {
    const int64_t l = C.slot_locus[(size_t)k];
    const ltr_locus& L = c.loci[l];
    const LocusInfo& I = c.info[(size_t)l];
    const LocusPools p = c.pools.of(c.read_base[(size_t)l]);
    C.lro[(size_t)k] = I.ubase; C.lho[(size_t)k] = I.hbase;
    int64_t at = I.rbyte0;
    for (int32_t u = 0; u < I.U; ++u) {
      const int32_t q = p.uniq_pool[u];
      C.read_off[(size_t)(I.ubase + u)] = at;
      if (p.lt[q] >= 0) std::memcpy(C.read_bytes + at, L.alns[p.first[q]].seq + p.lt[q], (size_t)p.len[q]);
      else ltr::write_empty_trim(L.hap, C.read_bytes + at);
      at += p.len[q];
    }
    (void)ltr::write_haplotypes(L.hap, I.H, &scratch().counts, C.hap_bytes, I.hbyte0, C.hap_off.data() + I.hbase);
    if (L.realign_to_hap) for (int64_t h = 0; h < I.H; ++h) if (!L.realign_to_hap[h]) C.mask_h[(size_t)(I.hbase + h)] = 0;
  }, 32, pool);
}

// Chunk `index` into staging arrays 2 * (index & 1) and 2 * (index & 1) + 1, on `threads` threads of worker pool `pool`
void stage_chunk(HapAlnCall& c, Chunk& C, int64_t index, int pool, int threads) {
  threads = std::min(c.budget, std::max(threads, 1));
  ltr::parallel_for_on(threads, C.l1 - C.l0, 64, [&c, &C](int64_t k) { if (!c.cancel.load(std::memory_order_relaxed)) prepare_locus(c, C.l0 + k); }, 32, pool);
  if (c.cancel.load(std::memory_order_relaxed)) { C.rc = LTR_ERR_INVALID; return; }
  c.mark("chunk %ld: %ld loci pooled + trimmed", (long)index, (long)(C.l1 - C.l0));
  order_chunk(c, C);
  if (C.rc != LTR_OK || C.slot_locus.empty()) return;
  layout_chunk(c, C, index, pool, threads);
  c.mark("chunk %ld: batch of %ld distinct trimmed reads (%ld B), %ld haplotypes (%ld B) laid out", (long)index, (long)C.n_u, (long)C.n_rb, (long)C.n_h, (long)C.n_hb);
}

// ---- a staged chunk on the calling thread: its short-path loci, its error, its plan on the GPU ----
int queue_chunk(HapAlnCall& c, Chunk& C, int64_t index) {
  // in locus order: the short-path loci before the chunk's first error queue up, then the error, if any
  for (const int64_t l : C.short_l) {
    if (!c.short_batch) c.short_batch.reset(ltr::short_batch_new());
    ShortLocus* SL = c.short_of[(size_t)l].get();
    const int rc = ltr::short_batch_merge(c.ctx, c.short_batch.get(), SL->batch.get());
    SL->batch.reset();
    c.short_loci.push_back(SL);
    if (rc != LTR_OK) return rc;
  }
  if (C.rc != LTR_OK) { if (C.err) ltr::set_error(c.ctx, C.err); return C.rc; }
  if (C.slot_locus.empty()) return LTR_OK;
  ltr_locus_batch b;
  std::memset(&b, 0, sizeof(b));
  b.n_loci = (int64_t)C.slot_locus.size(); b.locus_read_off = C.lro.data(); b.locus_hap_off = C.lho.data();
  b.n_reads = C.n_u; b.read_bytes = C.read_bytes; b.read_off = C.read_off.data();
  b.n_haps = C.n_h; b.hap_bytes = C.hap_bytes; b.hap_off = C.hap_off.data();
  if (C.any_mask) b.realign_hap = C.mask_h.data();
  ltr_plan* plan = nullptr;
  int rc = ltr_plan_create(c.ctx, &b, &plan);
  C.plan.reset(plan);
  c.mark("chunk %ld: planned (%ld pairs)", (long)index, plan ? (long)ltr_plan_num_pairs(plan) : 0L);
  // asynchronous: returns once the launches are queued.  Chunks alternate between two streams: the first
  // kernels of chunk c+1 run next to the exact kernels and the tail of chunk c.
  if (rc == LTR_OK) rc = ltr_plan_execute(plan, nullptr, ltr::ctx_side_stream(c.ctx, (int)(index % c.plan.n_streams)));
  c.mark("chunk %ld: launches queued", (long)index);
  return rc;
}

// every short-path locus of the call in one set of launches, its pool rows fanned out to the reads
int run_short_path(HapAlnCall& c) {
  if (!c.short_batch) return LTR_OK;
  c.mark("short path: %ld loci queued", (long)c.short_loci.size());
  int rc = ltr::short_batch_run(c.ctx, c.short_batch.get());
  c.mark("short path: scored");
  for (const ShortLocus* SL : c.short_loci) {
    if (rc != LTR_OK) break;
    const ltr_locus& L = c.loci[SL->locus];
    rc = ltr_scatter_pool_probs(SL->pool_probs.data(), SL->pool_seeds.data(), c.pools.of(c.read_base[(size_t)SL->locus]).index, L.n_alns,
                                (int32_t)SL->H, L.realign_to_hap, L.copy_read, L.second_mate, c.log_aln_probs[SL->locus], c.seed_positions[SL->locus]);
  }
  if (rc == LTR_OK) c.mark("short path: rows fanned out");
  return rc;
}

// the rows of one locus ([U x H], one per distinct trimmed read) to its reads (seq_stutter_genotyper.cpp:527-538), mates summed
int fan_out_locus(const HapAlnCall& c, int64_t l, const double* rows) {
  const ltr_locus& L = c.loci[l];
  const LocusPools p = c.pools.of(c.read_base[(size_t)l]);
  const int64_t H = c.info[(size_t)l].H;
  double* out = c.log_aln_probs[l];
  int32_t* seeds = c.seed_positions[l];
  for (int32_t i = 0; i < L.n_alns; ++i) {
    if (L.copy_read && !L.copy_read[i]) continue;
    const int32_t q = p.index[i];
    seeds[i] = L.alns[p.first[q]].seq_len - 1;                               // pool_seed_positions: HapAligner.cpp:562-563
    const int32_t u = p.uniq[q];
    double* dst = out + (int64_t)H * i;
    if (u >= 0) {
      const double* src = rows + (int64_t)H * u;
      if (!L.realign_to_hap) std::memcpy(dst, src, (size_t)H * sizeof(double));
      else for (int64_t j = 0; j < H; ++j) if (L.realign_to_hap[j]) dst[j] = src[j];
    } else {                                                                 // a pool that was not realigned: the reference copies an unwritten row, here zeros
      for (int64_t j = 0; j < H; ++j) if (!L.realign_to_hap || L.realign_to_hap[j]) dst[j] = 0.0;
    }
  }
  return ltr::sum_mate_rows(out, L.n_alns, H, L.second_mate, L.copy_read, L.realign_to_hap);
}

// in chunk order: rows of chunk c are fanned out to its reads while the later chunks still run
int fan_out_chunk(HapAlnCall& c, Chunk& C) {
  if (!C.plan) return LTR_OK;
  C.ll.reset(new double[(size_t)std::max<int64_t>(ltr_plan_ll_size(C.plan.get()), 1)]);
  const int rc = ltr_plan_fetch(C.plan.get(), C.ll.get(), nullptr);            // waits for THIS plan's kernels only
  c.mark("a chunk's rows fetched");
  // (the plan is destroyed with the others at the end: releasing its buffers waits for the streams it ran on, and a later
  // chunk shares its stream -- the rows of chunk c would be fanned out only after chunk c + 2 has finished on the GPU)
  if (rc != LTR_OK) return rc;
  std::atomic<int> first_rc(LTR_OK);
  ltr::parallel_for_on(c.budget, (int64_t)C.slot_locus.size(), 128, [&c, &C, &first_rc](int64_t k) {
    const int64_t l = C.slot_locus[(size_t)k];
    const int rc_l = fan_out_locus(c, l, C.ll.get() + c.info[(size_t)l].ll0);
    if (rc_l != LTR_OK) { int expect = LTR_OK; first_rc.compare_exchange_strong(expect, rc_l); }
  }, 32);
  if (first_rc.load() == LTR_OK) C.ll.reset();
  return first_rc.load();
}

}  // namespace

extern "C" {

int ltr_calc_hap_aln_probs(ltr_ctx* ctx, const ltr_locus* loci, int64_t n_loci,
                           double* const* log_aln_probs, int32_t* const* seed_positions) {
  if (!ctx || (!loci && n_loci > 0) || n_loci < 0 || !log_aln_probs || !seed_positions) return LTR_ERR_INVALID;
  ltr::TimedCall timed(ctx, ltr::kTimerHapAln);                        // total_hap_aln_time_, seq_stutter_genotyper.cpp:515,:561-562
  LTR_GUARD_BEGIN
  HapAlnCall c(ctx, loci, n_loci, log_aln_probs, seed_positions);
  int rc = validate_loci(c);
  if (rc != LTR_OK) return rc;
  plan_chunks(c);
  const int64_t n_chunks = (int64_t)c.chunks.size();
  if (c.plan.prep_ahead) stage_chunk(c, c.chunks[0], 0, 0, c.budget);
  for (int64_t k = 0; k < n_chunks && rc == LTR_OK; ++k) {
    if (c.plan.prep_ahead) {                       // chunk k was staged while chunk k - 1 was planned; chunk k + 1 starts now
      c.ahead.join();
      if (c.ahead.err) std::rethrow_exception(c.ahead.err);
      if (k + 1 < n_chunks)
        c.ahead.th = std::thread([&c, k]() { try { stage_chunk(c, c.chunks[(size_t)k + 1], k + 1, 1, c.plan.ahead_threads); } catch (...) { c.ahead.err = std::current_exception(); } });
    } else stage_chunk(c, c.chunks[(size_t)k], k, 0, c.budget);
    rc = queue_chunk(c, c.chunks[(size_t)k], k);
  }
  if (rc != LTR_OK) return rc;                     // (c.ahead cancels and joins the helper, then the chunks destroy their plans)
  c.ahead.join(); c.ahead.done = true;
  if ((rc = run_short_path(c)) != LTR_OK) return rc;
  for (Chunk& C : c.chunks) if ((rc = fan_out_chunk(c, C)) != LTR_OK) break;
  c.mark("rows fanned out to the reads");
  return rc;
  LTR_GUARD_END(ctx)
}

// test hooks (no GPU, declared in ltr_internal.h): the chunk rule on made-up numbers.  knobs[5] = chunks, chunk_streams,
// chunk_growth, chunk_growth_set, prep_ahead; budget 0 = the process's.  bounds[bounds_cap] receives n_chunks + 1 entries;
// out[4] = n_chunks, n_streams, prep_ahead, ahead_threads.
int ltr_debug_chunk_plan(int64_t n_loci, double est_cells, const double* knobs, int budget, int64_t* bounds, int bounds_cap, int32_t* out) {
  if (n_loci < 0 || !knobs || budget < 0 || !bounds || !out) return LTR_ERR_INVALID;
  ltr::DebugKnobs k;
  k.chunks = (int64_t)knobs[0]; k.chunk_streams = (int)knobs[1]; k.chunk_growth = knobs[2]; k.chunk_growth_set = knobs[3] != 0.0; k.prep_ahead = (int)knobs[4];
  try {
    const ChunkPlan P = plan_chunks(n_loci, est_cells, k, ltr::host_thread_budget_or(budget));
    if ((int64_t)P.bounds.size() > bounds_cap) return LTR_ERR_INVALID;
    std::copy(P.bounds.begin(), P.bounds.end(), bounds);
    out[0] = (int32_t)P.bounds.size() - 1; out[1] = P.n_streams; out[2] = P.prep_ahead ? 1 : 0; out[3] = P.ahead_threads;
    return LTR_OK;
  } catch (...) { return LTR_ERR_NOMEM; }
}
// ... whether a call of two chunks would use its helper thread under that budget
int ltr_debug_prep_ahead_rule(int n_threads) {
  try { return plan_chunks(1500, 0.0, ltr::DebugKnobs(), ltr::host_thread_budget_or(n_threads)).prep_ahead ? 1 : 0; } catch (...) { return LTR_ERR_NOMEM; }
}

}  // extern "C"
