// ltr_prep.h -- what ltr_prep.cpp (candidate haplotypes from exact alleles) shares with ltr_cluster.cpp (the clustering step of
// gen_candidate_seqs, HaplotypeGenerator.cpp:376-472): the result object, and ltr_build_haplotype cut in two at :372.
#ifndef LTR_PREP_H_
#define LTR_PREP_H_

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ltr_gpu.h"

struct ltr_hap_result {
  std::vector<int32_t> bstart, bend, period, nall;
  std::vector<uint8_t> is_rep, bytes, inexact;
  std::vector<int64_t> off;
  ltr_haplotype_blocks view;
  std::string failure;
  int32_t unplaced = 0, needs_clustering = 0;
  std::vector<int32_t> cluster_threshold;                       // per sample: accepted T, -1 none, 0 not needed (ltr_build_haplotypes_clustered / _consensus only)
  std::vector<int32_t> consensus_rounds, medoid_kept;           // per sample: refinement rounds taken; final clusters that kept the medoid (ltr_build_haplotypes_consensus only)
};

namespace ltr {
#pragma GCC visibility push(hidden)

// The state of gen_candidate_seqs at :373 (candidates from exact alleles, reference first) inside add_haplotype_block (:530-578).
struct HapDraft {
  std::string failure;                                          // not empty: the construction failed before the candidates
  int32_t rstart = 0, rend = 0, min_aln_start = 0, max_aln_stop = 0, ideal_min_length = 0, pad = 0, period = 0;
  std::vector<std::string> seqs;
  std::vector<std::vector<std::string>> per_sample;             // extracted sequences per sample
  std::vector<int32_t> ignored;                                 // per sample: reads whose sequence is no candidate (:376-391)
  int32_t unplaced = 0, needs_clustering = 0;
};
// ltr_build_haplotype up to :372; a status other than LTR_OK is the call's status
int hap_draft(const ltr_read_set* rs, int32_t n_samples, int32_t region_start, int32_t region_stop, int32_t period, const uint8_t* chrom_seq,
              int64_t chrom_seq_start, int64_t chrom_seq_len, int64_t chrom_len, int32_t indel_flank_len, HapDraft* d);
// ... and from :475 on: sort (the inexact flag travels with its sequence), trim, fuse.  seqs / inexact: the candidates, reference first.
int hap_finish(const HapDraft& d, std::vector<std::string> seqs, std::vector<uint8_t> inexact, const uint8_t* chrom_seq, int64_t chrom_seq_start,
               int64_t chrom_seq_len, int64_t chrom_len, ltr_hap_result** out);
bool by_len_seq(const std::string& x, const std::string& y);    // orderByLengthAndSequence

#pragma GCC visibility pop
}  // namespace ltr

#endif
