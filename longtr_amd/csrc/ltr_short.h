// ltr_short.h -- what the two halves of the seeded path share: the host batch builder (ltr_short_batch.cpp, plain C++) and
// the kernels with the stages that launch them (ltr_short.hip).  No HIP header, no HIP type: streams are void* (ltr_internal.h).
#ifndef LTR_SHORT_H_
#define LTR_SHORT_H_

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ltr {

constexpr double kImpS = -1000000000.0;        // IMPOSSIBLE, HapAligner.cpp:20
constexpr int kMaxIns = 6, kMaxDel = 6;        // MAX_STUTTER_REPEAT_INS / -DEL, RepeatStutterInfo.h:10-11
constexpr int kNumArt = kMaxIns + kMaxDel + 1;

struct ShortHap {            // one haplotype combination, one direction
  int64_t seq_off;           // into hap_bytes: the three blocks back to back
  int32_t len[3];            // block lengths (block 1 = repeat)
  int32_t up_off;            // into upstream: num_deletions (or 1) arrays of len[1] ints
  int32_t num_deletions;     // StutterAlignerClass::num_deletions_
  int32_t pad;
};
struct ShortRead {
  int64_t seq_off;           // read bytes (full sequence), then the reversed right part at rev_off
  int64_t rev_off;
  int64_t q_off;             // into wrong/correct: [0,seed) left part, [seed+1,len) right part REVERSED (HapAligner.cpp:889-890)
  int64_t cum_off;           // into cum: seed + 1 running sums of the left part's log_correct (left_prob before every base, then the
                             // total, HapAligner.cpp:36-44), then len - seed of the reversed right part's
  int32_t len, seed;
};
// (ShortArgs, what the kernels take by value, points at arrays of these two: ltr_short.hip)

// Host-side accumulator of the seeded path: loci are prepared one by one (short_batch_add), each on whatever host thread has
// it, strung together (short_batch_merge) and scored in ONE set of launches (short_batch_run): a wavefront per (pair, side) for
// the flank rows, a workgroup per (pair, side) for the stutter block's row -- one locus has ~100 pairs, a launch wants thousands.
struct ShortBatch {
  std::vector<ShortRead> reads; std::vector<ShortHap> fw, rv;
  std::vector<uint8_t> rbytes, hbytes; std::vector<int32_t> upstream;
  std::vector<double> art;
  std::vector<uint8_t> qidx;               // per base: index into BaseQuality's tables, in the order the kernels read wrong / correct
  int64_t n_cum = 0;
  std::vector<int32_t> pread, phap;
  std::vector<double*> pdst;               // where every pair's result goes on the host
  int period = 0, maxS = 1, maxHS = 1, maxB = 1;
  size_t n_ilog() const { return (size_t)maxHS + (size_t)maxB + 16; }   // entries of int_log: what a walk over the longest haplotype / block looks up
};

// S, HS, LP: ShortArgs.  A pure function of the batch and the knobs.
struct ShortGeom { int S, HS, LP, grid, chunk_cap; int64_t per_block; size_t lds_bytes; bool wave_kernel; };
ShortGeom short_geometry(const ShortBatch& B, int n_pairs, bool lane_knob);

// The host's libm tables of one call, into vectors the caller owns: int_log[B.n_ilog()] (mathops.cpp:14-22), qtab[128]
// (BaseQuality's log_error_ / log_correct_ by index, base_quality.h:29-43), pout[q] = q for every pair.
void short_host_tables(const ShortBatch& B, std::vector<double>* int_log, std::vector<double>* qtab, std::vector<int64_t>* pout);

}  // namespace ltr

// Test hook of short_geometry (tests/test_short_geometry_cases.py; not part of the ABI of include/ltr_gpu.h): the rule for a batch
// with these maxima.  out: S, HS, LP, lds_bytes, chunk_cap, wave_kernel, grid, per_block.
extern "C" int ltr_debug_short_geometry(int32_t max_side, int32_t max_block, int32_t max_hap, int32_t n_pairs, int32_t lane_knob, int64_t out[8]);

#endif
