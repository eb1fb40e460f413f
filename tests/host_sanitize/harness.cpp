// tests/host_sanitize/harness.cpp -- TEST INFRASTRUCTURE.
// Fuzzes the host-only entry points of the C-ABI library (ltr_host.cpp, ltr_hap_aln.cpp, ltr_genotype.cpp, the planning units of ltr_plan_*.cpp, the
// seeded path's batch builder ltr_short_batch.cpp) under
// AddressSanitizer + UBSan on the CPU: trimming, haplotype enumeration, pooling, scatter, genotype
// fields, and ltr_process_reads' host half (trim + haplotype strings) up to the point where it
// would hand the batch to the GPU.  The four library-internal symbols those files need from the HIP
// translation units are defined here (a context that holds parameters, a batch scorer that
// reports "no device").  Built and run by tests/test_host_sanitizers.py.
#include <cmath>
#include <cstdio>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../longtr_amd/csrc/ltr_internal.h"
#include "../../longtr_amd/csrc/ltr_plan.h"
#include "../../longtr_amd/csrc/ltr_short.h"

struct ltr_ctx { ltr_align_params p; std::string err; std::vector<uint8_t> host_bytes[4]; std::mutex call_mu, err_mu; ltr::DebugKnobs knobs; bool fake_device = false;
                 ltr_stutter_params stutter = {0.95, 0.05, 0.05, 0.95, 0.01, 0.01}; };    // (the library's defaults, ltr_default_stutter_params)
struct ltr_plan { int64_t ll_size = 0, pairs = 0; std::vector<double> ll; };   // (the fake device's plan: its "scores")
namespace ltr {
std::atomic<int> g_trace{0};                                      // (the trace switch and its clock live with the context, ltr_ctx.hip)
double dbg_ms() { return 0.0; }
void set_error(ltr_ctx* ctx, const std::string& msg) { if (ctx) { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->err = msg; } }
ltr_align_params ctx_params(const ltr_ctx* ctx) { return ctx->p; }
DebugKnobs ctx_debug(const ltr_ctx* ctx) { return ctx->knobs; }
void add_time(ltr_ctx*, int, double, double) {}
void* ctx_side_stream(const ltr_ctx*, int) { return nullptr; }
std::unique_lock<std::mutex> ctx_call_lock(ltr_ctx* ctx) { return std::unique_lock<std::mutex>(ctx->call_mu); }
uint8_t* ctx_host_bytes(ltr_ctx* ctx, int which, size_t bytes) { ctx->host_bytes[which & 3].resize(bytes); return ctx->host_bytes[which & 3].data(); }
ltr_stutter_params ctx_stutter_params(const ltr_ctx* ctx) { return ctx->stutter; }
// The seeded path: the batch builder is the library's (ltr_short_batch.cpp); the two functions of ltr_short.hip are defined here.
// On a fake device a batch "runs" like a plan does below: pair by pair, every offset a kernel follows is followed over the extent
// the kernel reads (checked against the array it points into: a vector's spare capacity hides an overrun from ASan), and the
// pair's score is a checksum of what was read there, stored where the pair's result goes.
int short_batch_run(ltr_ctx* ctx, ShortBatch* B) {
  if (!ctx->fake_device) return LTR_ERR_NO_DEVICE;
  auto bad = [&](const char* what) { set_error(ctx, std::string("fake short_batch_run: ") + what); return LTR_ERR_INVALID; };
  auto in = [](int64_t off, int64_t n, size_t size) { return off >= 0 && n >= 0 && (uint64_t)off + (uint64_t)n <= size; };
  if (B->phap.size() != B->pread.size() || B->pdst.size() != B->pread.size() || B->rv.size() != B->fw.size() || B->art.size() != B->fw.size() * kNumArt) return bad("array sizes");
  // (the prep kernel WRITES wrong / correct at q_off and cum at cum_off, read by read: no two reads may share a slot there, and
  // nothing here reads those arrays -- so: the reads lie back to back, as the builder lays them out)
  int64_t rb = 0, qo = 0, co = 0;
  for (const ShortRead& rd : B->reads) {
    if (rd.seq_off != rb || rd.q_off != qo || rd.cum_off != co || rd.len < 3 || rd.seed < 1 || rd.seed > rd.len - 2) return bad("reads not back to back");
    rb += (int64_t)rd.len + (rd.len - 1 - rd.seed); qo += rd.len; co += (int64_t)rd.len + 1;
  }
  if (rb != (int64_t)B->rbytes.size() || qo != (int64_t)B->qidx.size() || co != B->n_cum) return bad("read arrays longer than the reads");
  for (size_t q = 0; q < B->pread.size(); ++q) {
    if (!in(B->pread[q], 1, B->reads.size()) || !in(B->phap[q], 1, B->fw.size())) return bad("pair index");
    const ShortRead& rd = B->reads[(size_t)B->pread[q]];
    const int len = rd.len, seed = rd.seed, rlen = len - 1 - seed;
    if (seed < 1 || rlen < 1 || std::max(seed, rlen) > B->maxS) return bad("seed");
    if (rd.rev_off != rd.seq_off + len || !in(rd.seq_off, (int64_t)len + rlen, B->rbytes.size())) return bad("read bytes");
    if (!in(rd.q_off, len, B->qidx.size()) || !in(rd.cum_off, (int64_t)len + 1, (size_t)B->n_cum)) return bad("quality offsets");
    uint64_t s = 0;
    for (int j = 0; j < len + rlen; ++j) s = s * 31 + B->rbytes[(size_t)rd.seq_off + j];
    for (int j = 0; j < rlen; ++j) if (B->rbytes[(size_t)rd.rev_off + j] != B->rbytes[(size_t)rd.seq_off + len - 1 - j]) return bad("reversed read half");
    for (int j = 0; j < len; ++j) { const uint8_t k = B->qidx[(size_t)rd.q_off + j]; if (k > 'J' - '!') return bad("quality index"); s = s * 31 + k; }
    const ShortHap* dir[2] = {&B->fw[(size_t)B->phap[q]], &B->rv[(size_t)B->phap[q]]};
    for (const ShortHap* h : dir) {
      const int64_t hs = (int64_t)h->len[0] + h->len[1] + h->len[2];
      if (h->len[0] < 1 || h->len[1] < 0 || h->len[2] < 1 || hs > B->maxHS || h->len[1] > B->maxB || !in(h->seq_off, hs, B->hbytes.size())) return bad("haplotype bytes");
      if (h->num_deletions < 0 || h->num_deletions > kMaxDel || h->num_deletions * B->period > h->len[1]) return bad("num_deletions");
      const int64_t nup = (int64_t)std::max(h->num_deletions, 1) * std::max(h->len[1], 1);
      if (!in(h->up_off, nup, B->upstream.size())) return bad("upstream tables");
      for (int64_t j = 0; j < hs; ++j) s = s * 31 + B->hbytes[(size_t)(h->seq_off + j)];
      for (int64_t j = 0; j < nup; ++j) { const int32_t u = B->upstream[(size_t)(h->up_off + j)]; if (u < 0 || u > h->len[1]) return bad("upstream match length"); s = s * 31 + (uint64_t)u; }
    }
    const int64_t hs = (int64_t)dir[0]->len[0] + dir[0]->len[1] + dir[0]->len[2];
    for (int64_t j = 0; j < hs; ++j) if (B->hbytes[(size_t)(dir[1]->seq_off + j)] != B->hbytes[(size_t)(dir[0]->seq_off + hs - 1 - j)]) return bad("reversed haplotype");
    for (int a = 0; a < kNumArt; ++a) s = s * 31 + (uint64_t)(int64_t)(B->art[(size_t)B->phap[q] * kNumArt + a] * 1000.0);
    *B->pdst[q] = -1.0 - (double)(s % 100000);
  }
  return LTR_OK;
}
int process_reads_short(ltr_ctx* ctx, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap, const ltr_alignment* alns, int32_t n_alns,
                        int32_t init_read_index, const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions) {
  ShortBatch B;                                                    // (as ltr_short.hip has it)
  int rc = short_batch_add(ctx, &B, hap, realign_to_hap, alns, n_alns, init_read_index, realign_read, aln_probs, seed_positions);
  if (rc == LTR_OK) rc = short_batch_run(ctx, &B);
  return rc;
}
}
namespace ltrp {                                                   // (no page-locked memory without a device: RawBuf falls back to malloc)
void* pinned_alloc(size_t) { return nullptr; }
void pinned_free(void*) {}
}
static std::atomic<long> g_batches(0), g_pairs(0);                 // (the stub scorer is called from two threads at once below)
// A context with fake_device set gets plans that "run": the score of a pair is a checksum of its read's and its haplotype's bytes
// (the same however the loci are cut into chunks), so that the whole chunk pipeline of ltr_calc_hap_aln_probs (staging ahead on a
// thread of its own, fetch, fan-out) runs under the sanitizers.
extern "C" int ltr_plan_execute(ltr_plan* p, double*, void*) { return p ? LTR_OK : LTR_ERR_NO_DEVICE; }
extern "C" int ltr_plan_fetch(ltr_plan* p, double* ll, int32_t*) {
  if (!p) return LTR_ERR_NO_DEVICE;
  std::copy(p->ll.begin(), p->ll.end(), ll);
  return LTR_OK;
}
extern "C" int64_t ltr_plan_ll_size(const ltr_plan* p) { return p ? p->ll_size : 0; }
extern "C" int64_t ltr_plan_num_pairs(const ltr_plan* p) { return p ? p->pairs : 0; }
extern "C" void ltr_plan_destroy(ltr_plan* p) { delete p; }
static int touch_batch(const ltr_locus_batch* b);
extern "C" int ltr_plan_create(ltr_ctx* ctx, const ltr_locus_batch* b, ltr_plan** out) {
  *out = nullptr;
  const int rc = touch_batch(b);
  if (!ctx->fake_device) return rc;
  ltr_plan* p = new ltr_plan();
  auto checksum = [](const uint8_t* bytes, const int64_t* off, int64_t i) { uint64_t s = 0; for (int64_t k = off[i]; k < off[i + 1]; ++k) s = s * 31 + bytes[k]; return (long)(s & 0xffff); };
  for (int64_t l = 0; l < b->n_loci; ++l)
    for (int64_t r = b->locus_read_off[l]; r < b->locus_read_off[l + 1]; ++r)
      for (int64_t h = b->locus_hap_off[l]; h < b->locus_hap_off[l + 1]; ++h)
        p->ll.push_back(-1.0 - (double)((checksum(b->read_bytes, b->read_off, r) * 7 + checksum(b->hap_bytes, b->hap_off, h)) % 1000));
  p->pairs = p->ll_size = (int64_t)p->ll.size();
  *out = p;
  return LTR_OK;
}
extern "C" int ltr_align_batch(ltr_ctx*, const ltr_locus_batch* b, double*, int32_t*) { return touch_batch(b); }
static int touch_batch(const ltr_locus_batch* b) {
  // touch every byte the library handed over: ASan checks the extents
  long sum = 0;
  for (int64_t r = 0; r < b->n_reads; ++r)
    for (int64_t k = b->read_off[r]; k < b->read_off[r + 1]; ++k) sum += b->read_bytes[k];
  for (int64_t h = 0; h < b->n_haps; ++h)
    for (int64_t k = b->hap_off[h]; k < b->hap_off[h + 1]; ++k) sum += b->hap_bytes[k];
  g_batches++; g_pairs += (long)(b->n_reads * b->n_haps) + (sum & 1);
  return LTR_ERR_NO_DEVICE;
}

static std::mt19937_64 rng(20250225);
static int ri(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }
static std::string rseq(int n) { std::string s((size_t)n, 'A'); for (auto& c : s) c = "ACGT"[rng() & 3]; return s; }
static std::string rhomo(int n) { std::string s((size_t)n, 'A'); for (auto& c : s) if (rng() % 8 == 0) c = "CGT"[rng() % 3]; return s; }   // a homopolymer run with a few interruptions
static std::string rqual(int n) { std::string s((size_t)n, '5'); for (auto& c : s) c = (char)ri(20, 90); return s; }     // Phred+33, with bytes below '!' (33) and above 'J' (74)

// Loci for ltr_calc_hap_aln_probs: [flank][repeat][flank] blocks of block_len bp with up to max_alleles repeat alleles, n_reads
// reads of up to read_len bases (dup_reads: a later read is a copy of the first every other time, so that reads pool) placed
// start_off around the first block; masks: every few loci carry second_mate (never at read 0), realign_to_hap, realign_pool or copy_read.
// seeded: loci for the seeded stutter path -- the repeat has period 1 and homopolymer alleles of 0 .. 30 bases (every fourth locus
// has an EMPTY one: num_deletions == 0), every read has base qualities, locus 3 has a left flank of one base, locus 4 such a right flank.
struct LocSpec { int block_len[2], max_alleles, n_reads[2], read_len, start_off[2]; bool dup_reads, masks, seeded; };
struct Loc { std::vector<int32_t> bs, be, per, na; std::vector<uint8_t> rep, bytes; std::vector<int64_t> off;
             std::vector<std::string> seqs, quals, types; std::vector<std::vector<int32_t>> nums; std::vector<ltr_alignment> alns;
             ltr_haplotype_blocks hb; std::vector<double> probs; std::vector<int32_t> seeds; std::vector<uint8_t> mate, to_hap, pool, copy; };
struct LocSet {
  std::vector<Loc> L; std::vector<ltr_locus> loci; std::vector<double*> pp; std::vector<int32_t*> sp;
  LocSet(int NL, const LocSpec& s) : L((size_t)NL), loci((size_t)NL), pp((size_t)NL), sp((size_t)NL) {
    for (int l = 0; l < NL; ++l) {
      Loc& X = L[(size_t)l];
      int pos = ri(100, 1000);
      X.off.push_back(0);
      for (int b = 0; b < 3; ++b) {
        const bool is_rep = (b == 1);
        const bool one_base = s.seeded && ((l == 3 && b == 0) || (l == 4 && b == 2)), empty_allele = s.seeded && is_rep && l % 4 == 0;
        const int len = one_base ? 1 : ri(s.block_len[0], s.block_len[1]), nall = is_rep ? ri(empty_allele ? 2 : 1, s.max_alleles) : 1;
        X.bs.push_back(pos); X.be.push_back(pos + len); pos += len;
        X.rep.push_back(is_rep); X.per.push_back(is_rep ? (s.seeded ? 1 : ri(2, 6)) : 0); X.na.push_back(nall);
        for (int k = 0; k < nall; ++k) {
          const std::string a = !s.seeded ? rseq(k == 0 ? len : ri(1, 60)) : (!is_rep ? rseq(len) : rhomo(k == 0 ? len : (k == 1 && empty_allele ? 0 : ri(0, 30))));
          X.bytes.insert(X.bytes.end(), a.begin(), a.end()); X.off.push_back((int64_t)X.bytes.size());
        }
      }
      X.hb = {3, X.bs.data(), X.be.data(), X.rep.data(), X.per.data(), X.na.data(), X.bytes.data(), X.off.data()};
      const int R = ri(s.n_reads[0], s.n_reads[1]);
      for (int r = 0; r < R; ++r) {
        X.seqs.push_back(s.dup_reads && r > 0 && (rng() & 1) ? X.seqs[0] : rseq(ri(1, s.read_len)));
        X.types.push_back("="); X.nums.push_back({(int32_t)X.seqs.back().size()});
        if (s.seeded) X.quals.push_back(rqual((int)X.seqs.back().size()));       // (pooled copies of a read: each its own, so the pool's are medians)
      }
      for (int r = 0; r < R; ++r) {
        const int st = X.bs[0] + ri(s.start_off[0], s.start_off[1]);
        X.alns.push_back({st, st + X.nums[(size_t)r][0] - 1, (const uint8_t*)X.seqs[(size_t)r].data(), (int32_t)X.seqs[(size_t)r].size(), 1,
                          X.types[(size_t)r].data(), X.nums[(size_t)r].data(), s.seeded ? (const uint8_t*)X.quals[(size_t)r].data() : nullptr});
      }
      const int64_t H = ltr_haplotype_num_combs(&X.hb);
      X.probs.assign((size_t)std::max<int64_t>(1, R * H), 0.0); X.seeds.assign((size_t)std::max(1, R), 0);
      loci[(size_t)l] = {&X.hb, X.alns.data(), R, nullptr, nullptr, nullptr, nullptr};
      if (s.masks && R > 0) {
        auto bits = [&](size_t n) { std::vector<uint8_t> m(n); for (auto& x : m) x = rng() & 1; return m; };
        if (l % 3 == 0) { X.mate = bits((size_t)R); X.mate[0] = 0; loci[(size_t)l].second_mate = X.mate.data(); }
        if (l % 4 == 1) { X.to_hap = bits((size_t)H); loci[(size_t)l].realign_to_hap = X.to_hap.data(); }
        if (l % 5 == 2) { X.pool = bits((size_t)R); loci[(size_t)l].realign_pool = X.pool.data(); }      // (at most R pools)
        if (l % 7 == 3) { X.copy = bits((size_t)R); loci[(size_t)l].copy_read = X.copy.data(); }
      }
      pp[(size_t)l] = X.probs.data(); sp[(size_t)l] = X.seeds.data();
    }
  }
  void bad_cigar(int l, int r) {              // an invalid CIGAR operation in read r of locus l (if it has that many reads)
    Loc& X = L[(size_t)l];
    if ((int)X.alns.size() > r) { X.types[(size_t)r] = "Q"; X.alns[(size_t)r].cigar_type = X.types[(size_t)r].data(); }
  }
  const uint8_t* drop_qual(int l, int r) { const uint8_t* q = L[(size_t)l].alns[(size_t)r].qual; L[(size_t)l].alns[(size_t)r].qual = nullptr; return q; }
  void clear_outputs() { for (Loc& X : L) { std::fill(X.probs.begin(), X.probs.end(), 0.0); std::fill(X.seeds.begin(), X.seeds.end(), -7); } }
};
static ltr_ctx* init_ctx(ltr_ctx* ctx, bool fake_device) { std::memset(&ctx->p, 0, sizeof(ctx->p)); ctx->p.indel_flank_len = 5; ctx->fake_device = fake_device; return ctx; }

int main(int argc, char** argv) {
  long checks = 0;
  // ---- trim_alignment: random CIGARs (valid and corrupt) ---------------------------------------
  for (int it = 0; it < 20000; ++it) {
    const int nops = ri(0, 8);
    std::string types; std::vector<int32_t> nums; int qlen = 0, rlen = 0;
    for (int k = 0; k < nops; ++k) {
      const char t = (it % 17 == 0 && k == 1) ? 'Q' : "M=XIDSH"[ri(0, 6)];
      const int n = ri(it % 13 == 0 ? 0 : 1, 40);
      types += t; nums.push_back(n);
      if (t == 'M' || t == '=' || t == 'X') { qlen += n; rlen += n; } else if (t == 'I' || t == 'S') qlen += n; else if (t == 'D') rlen += n;
    }
    if (it % 11 == 0) qlen = std::max(0, qlen + ri(-3, 3));           // sequence / CIGAR length mismatch
    const std::string seq = rseq(qlen);
    const int start = ri(0, 2000);
    ltr_alignment a = {start, start + rlen - 1, (const uint8_t*)seq.data(), (int32_t)seq.size(), (int32_t)nums.size(),
                       types.data(), nums.data(), nullptr};
    int32_t lt = -1, rt = -1;
    const int rs = start + ri(-20, rlen + 20), re = rs + ri(0, 60);
    const int rc = ltr_trim_alignment(&a, rs, re, ri(0, 35), &lt, &rt);
    if (rc == LTR_OK && (lt < 0 || rt < 0 || lt + rt > (int)seq.size() + 1)) { std::printf("trim out of range\n"); return 1; }
    checks++;
  }
  // ---- haplotype enumeration + process_reads host half ----------------------------------------
  for (int it = 0; it < 600; ++it) {
    const int nb = ri(1, 4);
    std::vector<int32_t> bs, be, per, na; std::vector<uint8_t> rep, bytes; std::vector<int64_t> off(1, 0);
    int pos = ri(100, 1000);
    std::vector<std::string> keep;
    for (int b = 0; b < nb; ++b) {
      const bool is_rep = (b % 2 == 1);
      const int len = ri(is_rep ? 0 : 5, 60), nall = is_rep ? ri(1, 5) : 1;
      bs.push_back(pos); be.push_back(pos + len); pos += len;
      rep.push_back(is_rep); per.push_back(is_rep ? (it % 5 == 0 ? 1 : ri(1, 6)) : 0); na.push_back(nall);      // (period 1: the seeded path below)
      for (int k = 0; k < nall; ++k) { const std::string s = rseq(k == 0 ? len : ri(0, 80)); bytes.insert(bytes.end(), s.begin(), s.end()); off.push_back((int64_t)bytes.size()); }
    }
    ltr_haplotype_blocks hb = {nb, bs.data(), be.data(), rep.data(), per.data(), na.data(), bytes.data(), off.data()};
    const int64_t H = ltr_haplotype_num_combs(&hb);
    if (H < 1) { std::printf("num_combs %ld\n", (long)H); return 1; }
    std::vector<uint8_t> buf(400);
    for (int64_t k = -1; k <= H; ++k) {
      const int64_t n = ltr_haplotype_seq(&hb, k, buf.data(), (int64_t)buf.size());
      if (k >= 0 && k < H && n < 0 && n != LTR_ERR_INVALID) { std::printf("haplotype_seq rc %ld\n", (long)n); return 1; }
    }
    // reads over the locus, through ltr_process_reads (host half; the stub scorer says "no device"); every fifth locus down the
    // seeded path on the fake device, every other one of those with base qualities (without: LTR_ERR_INVALID at the first seed)
    ltr_ctx ctx; std::memset(&ctx.p, 0, sizeof(ctx.p)); ctx.p.indel_flank_len = ri(0, 35); ctx.p.use_short_path = (it % 5 == 0); ctx.fake_device = (it % 5 == 0);
    const int R = ri(0, 6);
    std::vector<std::string> seqs, quals, types; std::vector<std::vector<int32_t>> nums; std::vector<ltr_alignment> alns;
    for (int r = 0; r < R; ++r) {
      const int len = ri(1, 300);
      seqs.push_back(rseq(len)); quals.push_back(rqual(len)); types.push_back(std::string(1, '=')); nums.push_back({len});
    }
    for (int r = 0; r < R; ++r) {
      const int st = bs[0] + ri(-150, 50);
      alns.push_back({st, st + nums[(size_t)r][0] - 1, (const uint8_t*)seqs[(size_t)r].data(), (int32_t)seqs[(size_t)r].size(), 1,
                      types[(size_t)r].data(), nums[(size_t)r].data(), it % 10 == 0 ? (const uint8_t*)quals[(size_t)r].data() : nullptr});
    }
    std::vector<double> probs((size_t)std::max<int64_t>(1, R * H), 0.0); std::vector<int32_t> seeds((size_t)std::max(1, R), 0);
    (void)ltr_process_reads(&ctx, &hb, nullptr, alns.data(), R, 0, nullptr, probs.data(), seeds.data());
    if (ctx.err.rfind("fake short_batch_run", 0) == 0) { std::printf("process_reads, seeded path: %s\n", ctx.err.c_str()); return 1; }
    checks++;
  }
  // ---- ltr_calc_hap_aln_probs: threaded per-locus preparation + concatenation --------------------
  for (int it = 0; it < 6; ++it) {
    const int NL = 300 + 40 * it;
    LocSet S(NL, {{5, 40}, 4, {0, 8}, 200, {-100, 40}, true, false});
    if (it == 5) S.bad_cigar(123, 1);
    ltr_ctx ctx;
    const int rc = ltr_calc_hap_aln_probs(init_ctx(&ctx, false), S.loci.data(), NL, S.pp.data(), S.sp.data());
    if (rc != LTR_ERR_NO_DEVICE && rc != LTR_ERR_CIGAR && rc != LTR_ERR_INVALID) { std::printf("calc_hap_aln_probs rc %d\n", rc); return 1; }
    checks++;
  }
  // ---- the whole chunk pipeline on a fake device: five growing chunks, chunk c + 1 staged by the helper thread while the
  // calling thread "plans" chunk c; then the same one chunk after the other: the rows must be the same ----
  {
    const int NL = 2600;
    LocSet S(NL, {{36, 60}, 3, {1, 6}, 150, {-80, 30}, true, false});
    std::vector<std::vector<double>> first;
    for (int mode = 0; mode < 3; ++mode) {
      ltr_ctx ctx; init_ctx(&ctx, true);
      ctx.knobs.chunks = 5; ctx.knobs.chunk_growth = 1.3; ctx.knobs.chunk_growth_set = true;
      ctx.knobs.prep_ahead = mode == 0 ? 0 : (mode == 1 ? 3 : -1);          // helper thread on 16 threads / on 3 / off
      for (Loc& X : S.L) std::fill(X.probs.begin(), X.probs.end(), 0.0);
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_OK) { std::printf("chunked calc_hap_aln_probs on the fake device: rc %d (%s)\n", rc, ctx.err.c_str()); return 1; }
      if (mode == 0) for (const Loc& X : S.L) first.push_back(X.probs);
      else for (int l = 0; l < NL; ++l) if (first[(size_t)l] != S.L[(size_t)l].probs) { std::printf("chunk pipeline: mode %d differs at locus %d\n", mode, l); return 1; }
      checks++;
    }
    // a bad record in the fourth chunk: the call's error, whatever thread found it
    {
      S.bad_cigar(2000, 0);
      ltr_ctx ctx; init_ctx(&ctx, true);
      ctx.knobs.chunks = 5; ctx.knobs.chunk_growth = 1.3; ctx.knobs.chunk_growth_set = true;
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_ERR_CIGAR) { std::printf("bad record in a late chunk: rc %d\n", rc); return 1; }
      checks++;
    }
  }
  // ---- the same pipeline with mate pairs and the three masks of the realignment call: the helper thread on the whole budget / on
  // 3 threads / off, then one chunk -- identical rows and seeds (cells and seeds a mask leaves alone keep what they held) ----
  {
    const int NL = 2600;
    LocSet S(NL, {{36, 60}, 3, {1, 6}, 150, {-80, 30}, true, true});
    std::vector<std::vector<double>> rows; std::vector<std::vector<int32_t>> seeds;
    for (int mode = 0; mode < 4; ++mode) {
      ltr_ctx ctx; init_ctx(&ctx, true);
      ctx.knobs.chunks = mode == 3 ? 1 : 5; ctx.knobs.chunk_growth = 1.3; ctx.knobs.chunk_growth_set = true;
      ctx.knobs.prep_ahead = mode == 1 ? 3 : (mode == 2 ? -1 : 0);
      S.clear_outputs();
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_OK) { std::printf("masked calc_hap_aln_probs on the fake device: rc %d (%s)\n", rc, ctx.err.c_str()); return 1; }
      if (mode == 0) for (const Loc& X : S.L) { rows.push_back(X.probs); seeds.push_back(X.seeds); }
      else for (int l = 0; l < NL; ++l)
        if (rows[(size_t)l] != S.L[(size_t)l].probs || seeds[(size_t)l] != S.L[(size_t)l].seeds) { std::printf("masked chunk pipeline: mode %d differs at locus %d\n", mode, l); return 1; }
      checks++;
    }
    long written = 0, kept = 0;                                          // (the masks did mask, and did not mask everything)
    for (const Loc& X : S.L) for (size_t r = 0; r < X.alns.size(); ++r) (X.seeds[r] == -7 ? kept : written)++;
    if (!written || !kept) { std::printf("masked chunk pipeline: %ld reads written, %ld kept\n", written, kept); return 1; }
  }
  // ---- the same pipeline down the seeded stutter path (period-1 loci under use_short_path): every locus prepared by the library's
  // own batch builder on whatever thread has it, the batches strung together in locus order (short_batch_merge shifts their
  // offsets), the fake device following every offset.  Identical rows and seeds under the four modes; a read without base
  // qualities and a bad CIGAR operation are the call's error ----
  {
    const int NL = 2600;
    LocSet S(NL, {{20, 45}, 4, {1, 6}, 150, {-60, 30}, true, true, true});
    std::vector<std::vector<double>> rows; std::vector<std::vector<int32_t>> seeds;
    auto seeded_ctx = [](ltr_ctx* ctx, int mode) {
      init_ctx(ctx, true); ctx->p.use_short_path = 1;
      ctx->knobs.chunks = mode == 3 ? 1 : 5; ctx->knobs.chunk_growth = 1.3; ctx->knobs.chunk_growth_set = true;
      ctx->knobs.prep_ahead = mode == 1 ? 3 : (mode == 2 ? -1 : 0);
    };
    for (int mode = 0; mode < 4; ++mode) {
      ltr_ctx ctx; seeded_ctx(&ctx, mode);
      S.clear_outputs();
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_OK) { std::printf("seeded calc_hap_aln_probs on the fake device: rc %d (%s)\n", rc, ctx.err.c_str()); return 1; }
      if (mode == 0) for (const Loc& X : S.L) { rows.push_back(X.probs); seeds.push_back(X.seeds); }
      else for (int l = 0; l < NL; ++l)
        if (rows[(size_t)l] != S.L[(size_t)l].probs || seeds[(size_t)l] != S.L[(size_t)l].seeds) { std::printf("seeded chunk pipeline: mode %d differs at locus %d\n", mode, l); return 1; }
      checks++;
    }
    long seeded = 0, unseeded = 0, kept = 0, scored = 0;                 // (kept: reads a copy_read mask leaves alone)
    for (const Loc& X : S.L) {
      for (size_t r = 0; r < X.alns.size(); ++r) (X.seeds[r] >= 0 ? seeded : (X.seeds[r] == -1 ? unseeded : kept))++;
      for (const double v : X.probs) scored += v < 0.0;
    }
    std::printf("seeded path: %ld seeded reads, %ld unseeded, %ld left alone by a mask; %ld cells scored\n", seeded, unseeded, kept, scored);
    if (seeded <= 0 || unseeded <= 0 || scored <= 0 || 4 * seeded < seeded + unseeded + kept) { std::printf("seeded path: too few seeded or unseeded reads\n"); return 1; }
    // (the four modes string the same batches together in the same order; what the merge itself must keep: eight loci scored from one
    // merged batch get the scores each gets from a batch of its own)
    {
      ltr_ctx ctx; seeded_ctx(&ctx, 0);
      for (int l0 = 0; l0 + 8 <= 800; l0 += 8) {
        ltr::ShortBatch one[8], all;
        std::vector<std::vector<double>> alone;
        int rc = LTR_OK;
        for (int k = 0; k < 8 && rc == LTR_OK; ++k) {
          Loc& X = S.L[(size_t)(l0 + k)];
          std::fill(X.probs.begin(), X.probs.end(), 0.0);
          rc = ltr::short_batch_add(&ctx, &one[k], &X.hb, nullptr, X.alns.data(), (int32_t)X.alns.size(), 0, nullptr, X.probs.data(), X.seeds.data());
          if (rc == LTR_OK) rc = ltr::short_batch_run(&ctx, &one[k]);
          alone.push_back(X.probs);
          std::fill(X.probs.begin(), X.probs.end(), 0.0);
        }
        for (int k = 0; k < 8 && rc == LTR_OK; ++k) rc = ltr::short_batch_merge(&ctx, &all, &one[k]);
        if (rc == LTR_OK) rc = ltr::short_batch_run(&ctx, &all);
        if (rc != LTR_OK) { std::printf("seeded path, merged batch: rc %d (%s)\n", rc, ctx.err.c_str()); return 1; }
        for (int k = 0; k < 8; ++k) if (S.L[(size_t)(l0 + k)].probs != alone[(size_t)k]) { std::printf("seeded path: locus %d scores differently from a merged batch\n", l0 + k); return 1; }
        checks++;
      }
    }
    {
      const uint8_t* q = S.drop_qual(1500, 0);
      ltr_ctx ctx; seeded_ctx(&ctx, 0);
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_ERR_INVALID) { std::printf("seeded path, a read without base qualities: rc %d\n", rc); return 1; }
      S.L[1500].alns[0].qual = q;
      checks++;
    }
    {
      S.bad_cigar(2000, 0);                                              // (locus 2000 has no realign_pool mask: pool 0 is realigned)
      ltr_ctx ctx; seeded_ctx(&ctx, 0);
      const int rc = ltr_calc_hap_aln_probs(&ctx, S.loci.data(), NL, S.pp.data(), S.sp.data());
      if (rc != LTR_ERR_CIGAR) { std::printf("seeded path, a bad CIGAR operation: rc %d\n", rc); return 1; }
      checks++;
    }
  }
  // ---- two callers at once, own contexts: one gets the worker pool, the other finds it busy and falls back to
  // short-lived threads (ltr_internal.h) ----
  {
    const LocSpec spec = {{5, 40}, 3, {1, 6}, 150, {-80, 30}, false, false};
    LocSet A(700, spec), B(800, spec);
    int rca = 0, rcb = 0;
    std::thread ta([&]() { ltr_ctx c; init_ctx(&c, false); for (int k = 0; k < 3; ++k) rca = ltr_calc_hap_aln_probs(&c, A.loci.data(), 700, A.pp.data(), A.sp.data()); });
    std::thread tb([&]() { ltr_ctx c; init_ctx(&c, false); for (int k = 0; k < 3; ++k) rcb = ltr_calc_hap_aln_probs(&c, B.loci.data(), 800, B.pp.data(), B.sp.data()); });
    ta.join(); tb.join();
    if (rca != LTR_ERR_NO_DEVICE || rcb != LTR_ERR_NO_DEVICE) { std::printf("concurrent calc_hap_aln_probs rc %d %d\n", rca, rcb); return 1; }
    checks++;
  }
  // ---- on-disk formats: region reader (valid, malformed, truncated lines), VCF writer (plain + BGZF) ----
  {
    const std::string dir = "/tmp/ltr_harness_" + std::to_string((long)getpid());
    (void)mkdir(dir.c_str(), 0700);
    for (int it = 0; it < 300; ++it) {
      const std::string bed = dir + "/r.bed";
      FILE* f = std::fopen(bed.c_str(), "w");
      const int nl = ri(0, 12);
      for (int l = 0; l < nl; ++l) {
        const int st = ri(it % 7 == 0 ? 0 : 1, 5000);
        std::string line = "chr" + std::to_string(ri(1, 3)) + "\t" + std::to_string(st) + "\t" + std::to_string(st + ri(it % 5 == 0 ? -2 : 1, 80)) + "\t" + rseq(ri(1, 6));
        if (it % 3 == 0) line += ",AC";
        if (it % 4 == 0) line += "\tname" + std::to_string(l);
        if (it % 11 == 0 && l == 1) line = line.substr(0, (size_t)ri(0, (int)line.size()));     // truncated line
        std::fprintf(f, "%s\n", line.c_str());
      }
      std::fclose(f);
      ltr_region_set* rs = nullptr; char err[64];                  // (a short error buffer: messages are cut, not overrun)
      const int rc = ltr_read_regions(bed.c_str(), (uint32_t)ri(1, 20), it % 2 ? "chr1" : nullptr, &rs, err, (int)sizeof(err));
      if (rc == LTR_OK) {
        ltr_region_set_order(rs);
        for (int64_t i = -1; i <= ltr_region_set_size(rs); ++i) { (void)ltr_region_chrom(rs, i); (void)ltr_region_period(rs, i); (void)ltr_region_period_str(rs, i); }
        ltr_region_set_free(rs);
      } else if (rc != LTR_ERR_INVALID || std::strlen(err) >= sizeof(err)) { std::printf("read_regions rc %d\n", rc); return 1; }
      checks++;
    }
    for (int it = 0; it < 6; ++it) {
      ltr_vcf_writer* w = nullptr;
      const std::string path = dir + (it % 2 ? "/o.vcf.gz" : "/o.vcf");
      if (ltr_vcf_writer_open(path.c_str(), &w) != LTR_OK) { std::printf("vcf_writer_open\n"); return 1; }
      (void)ltr_vcf_writer_header(w, "##fileformat=VCFv4.1\n");
      int pos = 100;
      for (int k = 0; k < 4000; ++k) {
        pos += ri(0, 90);
        const std::string rec = "chr" + std::to_string(1 + k / 1500) + "\t" + std::to_string(pos + ri(-25, 25)) + "\t" + rseq(ri(0, 300));
        if (ltr_vcf_writer_add_record(w, ("chr" + std::to_string(1 + k / 1500)).c_str(), pos + ri(-25, 25), rec.c_str()) != LTR_OK) { std::printf("add_record\n"); return 1; }
      }
      if (ltr_vcf_writer_close(w) != LTR_OK) { std::printf("vcf_writer_close\n"); return 1; }
      checks++;
    }
    (void)std::remove((dir + "/r.bed").c_str()); (void)std::remove((dir + "/o.vcf").c_str()); (void)std::remove((dir + "/o.vcf.gz").c_str());
    (void)rmdir(dir.c_str());
  }
  // ---- BAM reader on a real file (argv[1]): every chromosome, random regions, a truncated and a corrupted copy ----
  if (argc > 1) {
    const char* paths[1] = {argv[1]};
    ltr_bam* b = nullptr; char err[256];
    if (ltr_bam_open(paths, 1, 1, &b, err, (int)sizeof(err)) != LTR_OK) { std::printf("bam_open: %s\n", err); return 1; }
    long n_rec = 0, n_bases = 0;
    ltr_bam_record rec;
    for (int32_t t = 0; t < ltr_bam_num_refs(b); ++t) {
      if (ltr_bam_set_region(b, ltr_bam_ref_name(b, t), 0, (int32_t)std::min<int64_t>(ltr_bam_ref_len(b, t), 0x7fffffff)) != LTR_OK) { std::printf("set_region\n"); return 1; }
      int rc;
      while ((rc = ltr_bam_next(b, &rec)) == 1) {
        n_rec++; n_bases += (long)std::strlen(rec.bases) + (long)std::strlen(rec.quals) + rec.n_cigar;
        int64_t iv; double dv; char cv;
        (void)ltr_bam_aux_int(&rec, "NM", &iv); (void)ltr_bam_aux_float(&rec, "rq", &dv); (void)ltr_bam_aux_char(&rec, "XX", &cv); (void)ltr_bam_aux_string(&rec, "RG");
        if (n_rec % 40 == 0 && ltr_bam_set_region(b, ltr_bam_ref_name(b, t), rec.pos + ri(-500, 500), rec.pos + ri(0, 30000)) != LTR_OK) { std::printf("set_region (inner)\n"); return 1; }
      }
      if (rc < 0) { std::printf("bam_next rc %d\n", rc); return 1; }
    }
    ltr_bam_close(b);
    if (n_rec == 0 || n_bases == 0) { std::printf("no BAM records read\n"); return 1; }
    // damaged copies: any status is fine, any memory error is not
    std::vector<uint8_t> raw; { FILE* f = std::fopen(argv[1], "rb"); uint8_t tmp[65536]; size_t n; while ((n = std::fread(tmp, 1, sizeof(tmp), f)) > 0) raw.insert(raw.end(), tmp, tmp + n); std::fclose(f); }
    std::vector<uint8_t> bai; { FILE* f = std::fopen((std::string(argv[1]) + ".bai").c_str(), "rb"); uint8_t tmp[65536]; size_t n; while ((n = std::fread(tmp, 1, sizeof(tmp), f)) > 0) bai.insert(bai.end(), tmp, tmp + n); std::fclose(f); }
    const std::string dir = "/tmp/ltr_harness_bam_" + std::to_string((long)getpid());
    (void)mkdir(dir.c_str(), 0700);
    for (int it = 0; it < 12; ++it) {
      std::vector<uint8_t> d = raw, x = bai;
      if (it % 3 == 0) d.resize((size_t)ri(100, (int)d.size() - 1));
      else if (it % 3 == 1) for (int k = 0; k < 30; ++k) d[(size_t)ri(2000, (int)d.size() - 1)] ^= (uint8_t)ri(1, 255);
      else for (int k = 0; k < 6; ++k) x[(size_t)ri(8, (int)x.size() - 1)] ^= (uint8_t)ri(1, 255);
      const std::string p = dir + "/d.bam";
      { FILE* f = std::fopen(p.c_str(), "wb"); std::fwrite(d.data(), 1, d.size(), f); std::fclose(f); }
      { FILE* f = std::fopen((p + ".bai").c_str(), "wb"); std::fwrite(x.data(), 1, x.size(), f); std::fclose(f); }
      const char* pp[1] = {p.c_str()};
      ltr_bam* q = nullptr;
      if (ltr_bam_open(pp, 1, 1, &q, err, (int)sizeof(err)) == LTR_OK) {
        for (int32_t t = 0; t < std::min(ltr_bam_num_refs(q), 3); ++t)
          if (ltr_bam_set_region(q, ltr_bam_ref_name(q, t), 0, 0x7fffffff) == LTR_OK) { int guard = 0; while (ltr_bam_next(q, &rec) == 1 && ++guard < 100000) {} }
        ltr_bam_close(q);
      }
      checks++;
    }
    (void)std::remove((dir + "/d.bam").c_str()); (void)std::remove((dir + "/d.bam.bai").c_str()); (void)rmdir(dir.c_str());
    checks++;
  }
  // ---- pooling + scatter ------------------------------------------------------------------------
  for (int it = 0; it < 2000; ++it) {
    const int R = ri(0, 40), H = ri(1, 9);
    std::vector<std::string> pool; for (int k = 0; k < 6; ++k) pool.push_back(rseq(ri(0, 30)));
    std::vector<const uint8_t*> ptr; std::vector<int32_t> len, idx((size_t)std::max(1, R));
    for (int r = 0; r < R; ++r) { const std::string& s = pool[(size_t)ri(0, 5)]; ptr.push_back((const uint8_t*)s.data()); len.push_back((int32_t)s.size()); }
    const int P = ltr_pool_reads(ptr.data(), len.data(), R, idx.data());
    if (P < 0 || P > R) { std::printf("pool_reads %d\n", P); return 1; }
    std::vector<double> pp((size_t)std::max(1, P * H), -1.0), out((size_t)std::max(1, R * H), -5.0);
    std::vector<int32_t> ps((size_t)std::max(1, P), 7), seeds((size_t)std::max(1, R), -1);
    std::vector<uint8_t> mh((size_t)H), cr((size_t)std::max(1, R)), sm((size_t)std::max(1, R));
    for (auto& x : mh) x = rng() & 1; for (auto& x : cr) x = rng() & 1; for (auto& x : sm) x = (rng() % 5 == 0);
    if (R > 0) sm[0] = 0;
    (void)ltr_scatter_pool_probs(pp.data(), ps.data(), idx.data(), R, H, it % 3 ? mh.data() : nullptr, it % 2 ? cr.data() : nullptr,
                                 it % 4 ? nullptr : sm.data(), out.data(), seeds.data());
    checks++;
  }
  // ---- genotype fields --------------------------------------------------------------------------
  for (int it = 0; it < 3000; ++it) {
    const int S = ri(0, 4), H = ri(1, 8), V = ri(1, H), hap = it & 1;
    std::vector<double> post((size_t)std::max(1, S * H * H)), stl((size_t)std::max(1, S), -30.0);
    for (auto& x : post) x = -(double)(rng() % 100000) / 1000.0 - ((rng() % 50 == 0) ? 8.9e307 : 0.0);
    std::vector<int32_t> h2a((size_t)H), best((size_t)std::max(1, 2 * S));
    for (auto& x : h2a) x = ri(0, V - 1);
    for (auto& x : best) x = ri(0, H - 1);
    if (it % 37 == 0) best[0] = H;                                     // invalid on purpose
    const int ngl = hap ? V : V * (V + 1) / 2, npgl = hap ? V : V * V;
    std::vector<int32_t> gts((size_t)std::max(1, 2 * S)), pls((size_t)std::max(1, S * ngl));
    std::vector<double> a((size_t)std::max(1, S)), b2(a), c(a), d(a), gl((size_t)std::max(1, S * ngl)), gd(a), pg((size_t)std::max(1, S * npgl));
    ltr_genotype_fields f = {gts.data(), a.data(), b2.data(), c.data(), d.data(), it % 3 ? gl.data() : nullptr, it % 2 ? gd.data() : nullptr,
                             it % 5 ? pls.data() : nullptr, it % 7 ? pg.data() : nullptr};
    (void)ltr_extract_genotypes(S, H, V, h2a.data(), hap, post.data(), stl.data(), best.data(), &f);
    checks++;
  }
  // ---- the launch schedule of a plan (ltrp::describe_batch, class_stats, build_schedule): random batches, every schedule ----
  for (int it = 0; it < 300; ++it) {
    const int n_loci = ri(0, 12);
    std::vector<int64_t> lro(1, 0), lho(1, 0), ro(1, 0), ho(1, 0);
    std::string rb, hb;
    for (int l = 0; l < n_loci; ++l) {
      const int base = (it % 7 == 0) ? ri(1, 3000) : ri(1, 700), nr = ri(0, 6), nh = ri(0, 4);
      for (int r = 0; r < nr; ++r) { std::string s = rseq(std::max(1, base + ri(-30, 30))); if (ri(0, 20) == 0) s[0] = 'N'; rb += s; ro.push_back((int64_t)rb.size()); }
      for (int h = 0; h < nh; ++h) { hb += rseq(ri(0, 9) == 0 ? ri(0, 60) : base + 60 + ri(-20, 20)); ho.push_back((int64_t)hb.size()); }
      lro.push_back((int64_t)ro.size() - 1); lho.push_back((int64_t)ho.size() - 1);
    }
    ltr_locus_batch b = {};
    b.n_loci = n_loci; b.locus_read_off = lro.data(); b.locus_hap_off = lho.data();
    b.n_reads = (int64_t)ro.size() - 1; b.read_bytes = (const uint8_t*)rb.data(); b.read_off = ro.data();
    b.n_haps = (int64_t)ho.size() - 1; b.hap_bytes = (const uint8_t*)hb.data(); b.hap_off = ho.data();
    ltr_align_params prm = {-1.0f, -0.458675f, -1.0f, it % 4 == 0 ? -0.5f : -0.458675f, -0.00005800168f, -10.448214f, -10.448214f, 5, 0};   // (every fourth: an asymmetric model)
    const int nk = ltr_debug_num_classes();
    std::vector<int32_t> grids((size_t)nk + 3);
    for (auto& g : grids) g = ri(1, 40);
    const int32_t knobs[7] = {ri(0, 1), ri(-1, 1), ri(0, 1), ri(0, 20), ri(0, 20), ri(0, 1), ri(0, 9)};
    const int mode = (it % 3 == 0) ? ri(-1, 8) : -1;
    std::vector<int64_t> out((size_t)8 + kNumExact + nk + 1);
    std::vector<int32_t> xg(kNumExact), launch((size_t)2 * nk * 8), members((size_t)2 * nk + 128), entry(256 * 6);
    std::vector<double> cells((size_t)2 * nk);
    const int rc = ltr_debug_plan_schedule(&prm, mode, ri(1, 4), &b, grids.data(), knobs, out.data(), xg.data(), 2 * nk, launch.data(), cells.data(),
                                           (int)members.size(), members.data(), 256, entry.data());
    if (rc != LTR_OK && rc != LTR_ERR_INVALID) { std::printf("plan_schedule rc %d\n", rc); return 1; }
    if (rc == LTR_OK && (out[0] > nk || out[1] > nk || out[2] > 256 || out[5] < 1)) { std::printf("plan_schedule out of range\n"); return 1; }
    checks++;
  }
  std::printf("host sanitizer harness: %ld cases, %ld batches reached the scorer (%ld pairs)\n", checks, g_batches.load(), g_pairs.load());
  return 0;
}
