// ltr_internal.h -- shared between the HIP side (ltr_ctx.hip and the units around it, ltr_short.hip, ltr_nw.hip) and the host mirror (ltr_host.cpp, ltr_hap_aln.cpp).
#ifndef LTR_INTERNAL_H_
#define LTR_INTERNAL_H_

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <pthread.h>
#include <sched.h>
#include <cstdio>
#include <cstdlib>

#include "../../include/ltr_gpu.h"

namespace ltr {

constexpr int kRefFlankLen = 35;        // REF_FLANK_LEN, reference HapAligner.cpp:245
constexpr double kImpossible = -1000000000.0;

// Window of the haplotype the DP sees: hap.substr(35-F, size-2*(35-F)) with
// std::string::substr's clamping and size_t wrap (reference HapAligner.cpp:246).
inline int64_t hap_window(int64_t hap_len, int flank, int64_t* pos_out) {
  const int64_t pos = kRefFlankLen - flank;
  int64_t cnt = hap_len - 2 * pos;
  const int64_t rest = hap_len - pos;
  if (cnt < 0 || cnt > rest) cnt = rest;
  *pos_out = pos;
  return cnt;
}

// ---- host-thread budget (round 6) -------------------------------------------------------------------------------------
// The reference is one thread per process and N processes per node (README.md:78-82).  This library's host loops (pooling,
// trimming, planning: ltr_calc_hap_aln_probs, seq_stutter_genotyper.cpp:514-563) run on worker threads, and eight ranks on a
// 64-core host must not start 8 x 32 of them.  The budget of a PROCESS (the worker pools are per process):
//   min(CPUs of the affinity mask, cgroup CPU quota rounded up, hardware threads) / ranks on this host, clamped to 1 .. 16.
// Ranks on this host: the launcher's LOCAL_WORLD_SIZE (torch.distributed.run sets it) unless the caller names the number
// (ltr_host_threads_rule) or the budget itself (ltr_ctx_set_host_threads, the only writer of the setting).  A call reads the budget
// ONCE (ltr_calc_hap_aln_probs: HapAlnCall::budget) and hands that value to its loops, so a setting changed meanwhile by another
// thread cannot make two decisions of one call disagree.
constexpr int kMaxHostThreads = 16;
constexpr int kPrepAheadMinThreads = 12;      // the chunk pipeline's helper thread pays from here on (profiles/r05/prep_ahead_ab.log: level at ~12)

inline int detect_host_cpus() {
  int n = (int)std::thread::hardware_concurrency();
  if (n <= 0) n = 1;
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int a = CPU_COUNT(&set); if (a > 0) n = std::min(n, a); }
  auto quota_cpus = [](const char* path_quota, const char* path_period) -> int {
    // cgroup v2: one file "max 100000" / "400000 100000"; cgroup v1: quota and period in files of their own (-1: no quota)
    long long q = -1, per = 100000;
    if (FILE* f = std::fopen(path_quota, "r")) {
      char word[64] = {0};
      if (std::fscanf(f, "%63s", word) == 1 && word[0] != 'm') q = std::atoll(word);
      if (!path_period) { long long p2 = 0; if (std::fscanf(f, "%lld", &p2) == 1 && p2 > 0) per = p2; }
      std::fclose(f);
    } else return 0;
    if (path_period) if (FILE* f = std::fopen(path_period, "r")) { long long p2 = 0; if (std::fscanf(f, "%lld", &p2) == 1 && p2 > 0) per = p2; std::fclose(f); }
    if (q <= 0) return 0;
    return (int)std::min<long long>((q + per - 1) / per, 1 << 20);
  };
  int q = quota_cpus("/sys/fs/cgroup/cpu.max", nullptr);
  if (q <= 0) q = quota_cpus("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us");
  if (q > 0) n = std::min(n, q);
  return std::max(n, 1);
}
// local_world_size <= 0: LOCAL_WORLD_SIZE of the environment (1 when unset)
inline int host_threads_rule(int local_world_size) {
  static const int cpus = detect_host_cpus();
  int lw = local_world_size;
  if (lw <= 0) { const char* e = std::getenv("LOCAL_WORLD_SIZE"); lw = e ? std::atoi(e) : 1; }
  if (lw <= 0) lw = 1;
  return std::max(1, std::min(cpus / lw, kMaxHostThreads));
}
inline std::atomic<int>& host_thread_setting() { static std::atomic<int> v(0); return v; }    // 0 = the rule
inline int host_thread_budget() {
  const int v = host_thread_setting().load(std::memory_order_relaxed);
  if (v > 0) return std::min(v, kMaxHostThreads);
  static const int rule = host_threads_rule(0);
  return rule;
}
inline int host_thread_budget_or(int n) { return n > 0 ? std::min(n, kMaxHostThreads) : host_thread_budget(); }   // (test hooks: a budget named by the caller)

// Host worker threads, started once per process and parked on a condition variable between jobs
// (every parallel_for of a plan used to start and join its own 15 threads: ~0.5 ms each, ten times per
// plan).  One job at a time; a caller that finds the pool busy (another context on another thread), a
// nested call from a worker, or a process forked while the pool existed falls back to short-lived threads.
// (Two pools: the second one serves the thread of ltr_calc_hap_aln_probs that prepares the next chunk of loci while the calling
// thread plans and launches the current one.)
class WorkerPool {
 public:
  static constexpr int kMaxWorkers = 15;
  static WorkerPool* get(int which = 0) {
    static std::once_flag once;
    std::call_once(once, []() {
      instance(0) = new WorkerPool(); instance(1) = new WorkerPool();
      (void)pthread_atfork(nullptr, nullptr, []() { instance(0) = nullptr; instance(1) = nullptr; });
    });
    return instance(which);                  // (leaked on purpose: parked workers outlive static destructors; null in a forked child)
  }
  static bool& on_worker() { static thread_local bool w = false; return w; }
  // job() on `extra` workers and on the caller; returns when all of them are back.  False: not run at all.
  template <class Job>
  bool run(int extra, Job&& job) {
    if (on_worker()) return false;
    std::unique_lock<std::mutex> busy(busy_mu_, std::try_to_lock);
    if (!busy.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      while ((int)threads_ < std::min(extra, kMaxWorkers)) {
        try { std::thread([this]() { worker(); }).detach(); } catch (...) { break; }
        ++threads_;
      }
      extra = std::min<int>(extra, (int)threads_);
      if (extra <= 0) return false;
      fn_ = [&job]() { job(); };
      tickets_ = extra; pending_ = extra; ++generation_;
    }
    cv_work_.notify_all();
    job();
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [this]() { return pending_ == 0; });
    fn_ = nullptr;
    return true;
  }

 private:
  static WorkerPool*& instance(int which) { static WorkerPool* p[2] = {nullptr, nullptr}; return p[which & 1]; }
  void worker() {
    on_worker() = true;
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_work_.wait(lk, [&]() { return generation_ != seen && tickets_ > 0; });
      seen = generation_;
      --tickets_;
      std::function<void()> fn = fn_;
      lk.unlock();
      fn();                                   // (the job catches its own exceptions)
      lk.lock();
      if (--pending_ == 0) cv_done_.notify_all();
    }
  }
  std::mutex busy_mu_, mu_;
  std::condition_variable cv_work_, cv_done_;
  std::function<void()> fn_;
  int threads_ = 0, tickets_ = 0, pending_ = 0;
  uint64_t generation_ = 0;
};

// f(i) for i in [0, n) on up to `threads` host threads (chunks of `grain` from a shared counter); serial when the range is too
// short to pay for the hand-over.  The cap is the caller's: a call that must see ONE budget from its first loop to its last
// (ltr_calc_hap_aln_probs) reads host_thread_budget() once and hands that value to every loop.  (which_pool: see WorkerPool)
template <class F>
inline void parallel_for_on(int threads, int64_t n, int64_t min_per_thread, F&& f, int64_t grain = 64, int which_pool = 0) {
  const int64_t nt = std::min<int64_t>(std::max(threads, 1), n / std::max<int64_t>(min_per_thread, 1));
  if (nt <= 1) { for (int64_t i = 0; i < n; ++i) f(i); return; }
  std::atomic<int64_t> next(0);
  // an exception on a worker thread would end the process (std::terminate): the first one is kept
  // and re-thrown on the calling thread after the join, where the entry points turn it into a status
  std::exception_ptr first_error;
  std::atomic<bool> failed(false);
  auto work = [&]() {
    try {
      for (;;) {
        const int64_t i0 = next.fetch_add(grain);
        if (i0 >= n || failed.load(std::memory_order_relaxed)) break;
        for (int64_t i = i0; i < std::min(i0 + grain, n); ++i) f(i);
      }
    } catch (...) {
      if (!failed.exchange(true)) first_error = std::current_exception();
    }
  };
  WorkerPool* pool = WorkerPool::get(which_pool);
  if (!pool || !pool->run((int)nt - 1, work)) {
    std::vector<std::thread> th;
    try {
      for (int64_t k = 1; k < nt; ++k) th.emplace_back(work);
    } catch (...) {                                            // could not start every thread: the ones running finish the range
    }
    work();
    for (std::thread& t : th) t.join();
  }
  if (failed.load()) std::rethrow_exception(first_error);
}
// ... on up to min(host_thread_budget(), max_threads) threads: the budget as it stands when the loop starts
template <class F>
inline void parallel_for(int64_t n, int64_t min_per_thread, F&& f, int64_t grain = 64, int which_pool = 0, int max_threads = kMaxHostThreads) {
  parallel_for_on(std::min(host_thread_budget(), max_threads), n, min_per_thread, std::forward<F>(f), grain, which_pool);
}

// Entry points never let an exception cross the C-ABI: LTR_GUARD(ctx, body) maps bad_alloc to
// LTR_ERR_NOMEM and anything else to LTR_ERR_INVALID.
#define LTR_GUARD_BEGIN try {
#define LTR_GUARD_END(ctx)                                                                                   \
  } catch (const std::bad_alloc&) { ltr::set_error(ctx, "out of host memory"); return LTR_ERR_NOMEM; }       \
  catch (const std::exception& e_) { ltr::set_error(ctx, std::string("internal error: ") + e_.what()); return LTR_ERR_INVALID; } \
  catch (...) { ltr::set_error(ctx, "internal error"); return LTR_ERR_INVALID; }

enum { kTimerHapBuild = 0, kTimerHapAln = 1, kTimerPosterior = 2, kTimerNwKernel = 3, kTimerShortKernel = 4 };   // (3, 4: kernel_ms only)
void add_time(ltr_ctx* ctx, int which, double seconds, double kernel_ms = 0.0);

// Wall-clock scope of one entry point; nested entry points (ltr_process_reads -> ltr_align_batch) count once.
struct TimedCall {
  ltr_ctx* ctx; int which; bool outer;
  std::chrono::steady_clock::time_point t0;
  static int& depth() { static thread_local int d = 0; return d; }
  TimedCall(ltr_ctx* c, int w) : ctx(c), which(w), outer(depth()++ == 0), t0(std::chrono::steady_clock::now()) {}
  ~TimedCall() {
    --depth();
    if (outer) add_time(ctx, which, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
};

// ltr_ctx_set_debug(ctx, "trace", 1) on any context: phase prints to stderr (the flag and the clock live in ltr_ctx.hip)
extern std::atomic<int> g_trace __attribute__((visibility("hidden")));
double dbg_ms() __attribute__((visibility("hidden")));
#define LTR_DBG(...) do { if (ltr::g_trace.load(std::memory_order_relaxed)) { std::fprintf(stderr, "[ltr %10.2f ms] ", ltr::dbg_ms()); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::fflush(stderr); } } while (0)

// Measurement switches of a context (ltr_ctx_set_debug): A/B runs of tests/manual/*.py and profiles/collect.sh.
// 0 / unset = the library's own rule.  Scheduling only: results never depend on them.
struct DebugKnobs {
  int fan_lanes = 0;            // streams the certificate launches of a plan are dealt over (1 .. 4; rule: 2)
  int64_t fan_pairs = 0;        // plans with at least this many pairs stay on one stream
  int64_t chunks = 0;           // ltr_calc_hap_aln_probs: number of chunks (rule: 2 from 1500 loci up)
  int chunk_streams = 0;        // ... streams the chunks' plans alternate between (rule: 2)
  double chunk_growth = 0.0;    // ... weights 1, g, g^2, .. (g > 0); 1, 2, 3, .. (0); 1, 2, .., k, k, .., 2, 1 (g < 0); rule: 3
  bool chunk_growth_set = false;
  int fold_rounds = 0;          // automatic mode: fold launch classes below this many rounds of resident waves (rule: ltrp::kFoldRounds)
  int short_lane_kernel = 0;    // short path: the lane-per-pair kernel even where the wavefront-per-pair kernel applies (A/B)
  int plan_kernel = 0;          // A/B: 1 = a launch per class / the multi-width launches as before round 5; 0 (and -1, kept for old scripts) = the rule: the plan kernel for every automatic-mode plan
  int wave_clock = 0;           // 1: the plan kernel records every wavefront's first / last wall clock (ltr_plan_debug_wave_clocks), and so does the family launch (ltr_debug_family_wave_clocks)
  int chain = 0;                // 1 = the plan kernel's one-wave classes of strip widths 11 .. 20 by the chained walk (ltr_dp_chain.hpp; measured slower: off)
  int chain_min_w = 0, chain_max_w = 0;   // ... the chained walk for these strip widths only (0: 11 .. 20)
  int plan_share = 0;           // A/B: 1 = every wavefront of the plan kernel starts at the top of its table (default: spread over the entries in proportion to their work)
  int wg_first_pass = 0;        // first pass of the workgroup classes: 0 = what the context has learnt (rule), 1 = always the certificate kernels, 2 = always the threshold kernels (exact in one pass)
  int wgt_keep_waves = 0;       // A/B: 1 = the threshold first pass keeps the four waves of the wide four-wave classes (rule: eight waves, strips half as wide)
  int short_split = 0;          // 1: the seeded stutter path records events between its launches (ltr_ctx_short_kernel_split)
  int compact_plan = 0;         // A/B: -1 = no compact plans (every plan through the separate allocations, copies and fills of the large ones)
  int no_multi = 0;             // A/B: 1 = a launch per class (no multi-width launches), -1 = multi-width launches whatever the plan's size (rule: 512 .. 4096 pairs per CU)
  int pack_rule = 0;            // A/B: 3 = the per-length floor on the lanes per pair of the packed classes (rule until round 4), 2 = no floor at all
  int prep_ahead = 0;           // ltr_calc_hap_aln_probs: -1 = chunk c + 1 is pooled, trimmed and laid out only after chunk c's launches are queued (as before round 5); n > 0: the helper thread on, with n threads of its own; rule: on from a host-thread budget of kPrepAheadMinThreads, with the whole budget
  int trace = 0;                // ltr_calc_hap_aln_probs prints a timestamped phase profile to stderr
  int64_t ll_chunk_loci = 0;    // ltr_ll_genotype: loci per upload chunk (rule: as many as fit 8 MB of staging)
  int families = 0;             // haplotype families (ltr_dp_family.hpp): -1 = never, 0 = by rule (where modelled cheaper), 1 = whenever one can be formed from reads of 641 .. 1280 columns, 2 = ... of 321 .. 1280
  int family_min_rows = 0;      // ... fewest shared rows (0: ltrp::kFamMinRows)
  int family_spine = 0;         // ... run along a spine (ltr_dp_family.hpp, spine_walk): -1 = never (plain families), 0 = by rule (plans of ltrp::kSpinePerCu families per CU and more), 1 = in any plan
  int grid_cap = 0;             // tests: n > 0 = every DP launch of ltr_plan_execute and every class launch of ltr_haplotype_align_to_ref on at most n workgroups (many items per wavefront on any device); read when a plan is built
  int64_t poa_group_cap_bytes = 0;    // ltr_poa_consensus: scratch of one group at most (rule: 512 MB); a group over it is not aligned (status 1) -- the one switch results depend on
  int64_t poa_call_budget_bytes = 0;  // ... scratch of one launch set at most (rule: 16 GB)
};
DebugKnobs ctx_debug(const ltr_ctx* ctx);
// the class launches of an ltr_haplotype_align_to_ref call as made, for ltr_debug_last_launches (ltr_plan.h: LaunchNote); kind < 0 begins a call
void ctx_note_nw_launch(ltr_ctx* ctx, int kind, int cls, int grid, int takers, int64_t items);

void set_error(ltr_ctx* ctx, const std::string& msg);
ltr_align_params ctx_params(const ltr_ctx* ctx);
ltr_stutter_params ctx_stutter_params(const ltr_ctx* ctx);
int ctx_device(const ltr_ctx* ctx);
void* ctx_stream(const ltr_ctx* ctx);      // hipStream_t
// (device memory of the context's pool and its recycled events: through a DevLease, ltr_lease.h)
void* ctx_big_scratch(ltr_ctx* ctx, size_t bytes);   // one grow-only device block kept by the context (NW trace); NULL = out of memory; one user at a time
std::unique_lock<std::mutex> ctx_call_lock(ltr_ctx* ctx);   // held for a whole ltr_calc_hap_aln_probs / haplotype-alignment call: they stage in the two arrays below / in ctx_big_scratch
uint8_t* ctx_host_bytes(ltr_ctx* ctx, int which, size_t bytes);   // one of four grow-only staging arrays kept by the context (uninitialised)
void* ctx_side_stream(const ltr_ctx* ctx, int k);
void ctx_note_short_split(ltr_ctx* ctx, const double ms4[4]);   // ltr_short.hip -> the context: device time of the seeded path's launches, summed over calls   // k % 8 == 0: the context's stream, else one of its seven side streams

// HapAligner::process_reads with short_ == 1 (ltr_short.hip)
int process_reads_short(ltr_ctx* ctx, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap,
                        const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                        const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions);

// The same in two halves, for many loci in one launch (ltr_calc_hap_aln_probs): add() prepares a
// locus on the host (and writes its seeds / all-zero rows at once), run() scores everything queued.
// aln_probs passed to add() must stay valid until run().  (new / add / merge / free: ltr_short_batch.cpp, host code; run:
// ltr_short.hip; the struct: ltr_short.h)
struct ShortBatch;
ShortBatch* short_batch_new();
void short_batch_free(ShortBatch* b);
int short_batch_add(ltr_ctx* ctx, ShortBatch* b, const ltr_haplotype_blocks* hap, const uint8_t* realign_to_hap,
                    const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                    const uint8_t* realign_read, double* aln_probs, int32_t* seed_positions);
int short_batch_merge(ltr_ctx* ctx, ShortBatch* dst, ShortBatch* src);   // dst += src; src is left empty
int short_batch_run(ltr_ctx* ctx, ShortBatch* b);

// Haplotype::next() order (reference Haplotype.cpp:123-196): allele index per block for
// every combination, combination-major.
int haplotype_counts(const ltr_haplotype_blocks* hap, std::vector<int32_t>* counts, int64_t* ncombs);

// Per-locus primitives of ltr_host.cpp that ltr_process_reads and the many-locus call (ltr_hap_aln.cpp) share.
int64_t allele_slot(const ltr_haplotype_blocks* hap, int block, int allele);
int trim_alignment_into(const ltr_alignment* aln, int32_t repeat_start, int32_t repeat_end, int32_t padding, int32_t* rem /* n_cigar ints */,
                        int32_t* ltrim_out, int32_t* rtrim_out);
const char* trim_error_text(int rc);
constexpr const char* kBadAlignmentRecord = "alignment with a negative length or a null sequence / CIGAR pointer";
inline bool alignment_record_ok(const ltr_alignment& a) {
  return a.seq_len >= 0 && (a.seq_len == 0 || a.seq) && a.n_cigar >= 0 && (a.n_cigar == 0 || (a.cigar_type && a.cigar_num));
}
// What stands in for a read whose trim is empty: the last 5 bp of the first block's reference allele + the first 5 bp of the last
// block's (HapAligner.cpp:820-823).  Its length, -1 when the first block is shorter than 5 bp; its bytes to dst.
constexpr const char* kShortLeftFlank = "left flank shorter than 5 bp (std::string::substr would throw in the reference)";
int32_t empty_trim_len(const ltr_haplotype_blocks* hap);
void write_empty_trim(const ltr_haplotype_blocks* hap, uint8_t* dst);
// The haplotype strings of a locus in Haplotype::next() order: their number and total length (a status on a malformed block
// list), and the strings themselves written to bytes + at one after the other, off[h] = where string h starts; returns where the
// last one ends.  counts: scratch of haplotype_counts.
int haplotype_sizes(const ltr_haplotype_blocks* hap, std::vector<int32_t>* counts, int64_t* n_haps, int64_t* n_bytes);
int64_t write_haplotypes(const ltr_haplotype_blocks* hap, int64_t n_haps, std::vector<int32_t>* counts, uint8_t* bytes, int64_t at, int64_t* off);
// Mate pairs share one row sum (seq_stutter_genotyper.cpp:546-559) in rows [n_reads x n_haps]; read 0 as a second mate: LTR_ERR_INVALID
int sum_mate_rows(double* rows, int32_t n_reads, int64_t n_haps, const uint8_t* second_mate, const uint8_t* copy_read, const uint8_t* realign_to_hap);
// ltr_vcf_record_from_fields into a string (ltr_vcf.cpp): the length of the text or a negative status.  sample_haploid: null, or
// for a diploid-form locus (v->haploid == 0) the ploidy of each of its samples [n_samples] (ltr_gpu_ploidy.h): a haploid one fills
// its ten-field column with one allele and "." where a single copy has no value.
int64_t vcf_record_string(const ltr_vcf_locus* v, const ltr_locus_fields* f, const ltr_vcf_options* opt, std::string* text, int32_t* pos,
                          const uint8_t* sample_haploid = nullptr);

// A block list that owns its arrays (view points into them; not copyable once filled).
struct OwnedHapBlocks {
  std::vector<int32_t> bstart, bend, period, nall;
  std::vector<uint8_t> is_rep, bytes;
  std::vector<int64_t> off;
  ltr_haplotype_blocks view = {};
  OwnedHapBlocks() = default;
  OwnedHapBlocks(const OwnedHapBlocks&) = delete;
  OwnedHapBlocks& operator=(const OwnedHapBlocks&) = delete;
};
// HapBlock::remove_alleles (HapBlock.h:151-160, RepeatBlock.h:60-69) for every block of a list: removed[b] = allele indices
// of block b to drop (b beyond removed.size(): none).  Allele 0 or an index outside the block: LTR_ERR_INVALID.  (ltr_vcf.cpp)
int prune_hap_blocks(const ltr_haplotype_blocks* old, const std::vector<std::vector<int32_t>>& removed, OwnedHapBlocks* out);
// The haplotype matching of add_and_remove_alleles (seq_stutter_genotyper.cpp:322-360) as ltr_remap_haplotypes does it, on
// Haplotype::next() tables computed once: allele_mapping [H old] = new index or -1; realign [H new] (may be null).  (ltr_vcf.cpp)
int remap_haplotypes(const ltr_haplotype_blocks* old_hap, const ltr_haplotype_blocks* new_hap, std::vector<int32_t>* allele_mapping,
                     std::vector<uint8_t>* realign);

}  // namespace ltr

// Test hooks of ltr_hap_aln.cpp's chunk rule (tests/test_abi_and_host.py; not part of the ABI of include/ltr_gpu.h): see there.
extern "C" int ltr_debug_chunk_plan(int64_t n_loci, double est_cells, const double* knobs, int budget, int64_t* bounds, int bounds_cap, int32_t* out);

#endif
