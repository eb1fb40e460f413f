// ltr_plan_fields.h -- what ltr_plan_genotype.hip (the passes) and ltr_plan_fields.hip (the VCF fields of every locus of a
// genotyped plan) share: the result object and the fields stage.
#pragma once

#include <memory>
#include <vector>

#include "ltr_posterior_common.h"

// a locus that lost alleles
struct LtrPruned {
  ltr::OwnedHapBlocks blocks;                    // HapBlock::remove_alleles of every block
  std::vector<int32_t> new_to_old, allele_mapping;
  std::vector<std::vector<int32_t>> removed;     // per block
  int32_t aff_blocks = 0, aff_alleles = 0, Hn = 0;
  int64_t post_off = 0;                          // its [S x Hn x Hn] block in post2
};

struct ltr_genotype_result {
  int64_t n_loci = 0;
  std::vector<int32_t> S, H, n_blocks;           // per locus
  std::vector<uint8_t> haploid;                  // per locus: its ploidy, resolved once at the top of the call (LocusPloidy); every stage reads this.
                                                 // With a ploidy per sample: 1 exactly when every sample of the locus is haploid (0 for a mixed locus)
  std::vector<uint8_t> sample_haploid;           // per unit: the sample's ploidy, resolved in the same place (SamplePloidy): priors, fields and records follow it
  bool mixed(int64_t l) const {                  // a locus with a haploid sample that is not all haploid: the diploid shape, some rows haploid
    if (haploid[(size_t)l]) return false;
    for (int64_t u = unit_off[(size_t)l]; u < unit_off[(size_t)l + 1]; ++u) if (sample_haploid[(size_t)u]) return true;
    return false;
  }
  std::vector<int64_t> unit_off, post1_off;      // [n_loci + 1]
  std::unique_ptr<double[]> post1, post2, read_ll;      // first-pass blocks (plan's H), second-pass blocks of the pruned loci
  std::vector<double> stl;                       // [units] final
  std::vector<int32_t> gts;                      // [2 units] final
  std::vector<int32_t> identity;                 // 0 .. max H - 1: new_to_old / allele_mapping of a locus that lost nothing
  std::vector<std::unique_ptr<LtrPruned>> pruned;   // per locus, null: nothing removed
  std::vector<const ltr_haplotype_blocks*> haps; // the caller's block lists
  std::vector<int64_t> read_ll_off;              // [n_loci + 1] (want_read_ll)
  // ---- ltr_plan_genotype_fields only ----
  bool has_fields = false;
  ltr_ctx* ctx = nullptr;                        // (for ltr_last_error of ltr_genotype_result_vcf_records)
  std::vector<int32_t> f_block, f_V;             // per locus: the block the fields are for, its alleles
  std::vector<int64_t> f_gl_off, f_pgl_off, f_read_off;   // [n_loci + 1]: gls / pls, phased_gls, reads
  std::unique_ptr<int32_t[]> f_i32;              // best_gts [2 nu], n_aligned, n_snp, n_s1, n_s2 [nu each], read_allele [reads]
  std::unique_ptr<double[]> f_f64;               // log_phased, log_unphased, hap_log_phased, hap_log_unphased, gl_diffs [nu each]
  std::unique_ptr<double[]> f_gls, f_pgls;       // when asked for
  std::unique_ptr<int32_t[]> f_pls;
};

// the device outputs of a posterior pass (null: the pass did not run)
struct DevPass { double* post = nullptr; double* stl = nullptr; int* gts = nullptr; };

#pragma GCC visibility push(hidden)
// The fields stage of ltr_plan_genotype_fields (ltr_plan_fields.hip): layout, tables, the kernel on the passes' buffers where they
// lie, copies into res.  src: where the scores lie (the plan's buffer, or the per-read block of ltr_ll_genotype); pass[0] /
// pass[1]: the first / second pass; d_map: the column maps of the pruned loci (null: none).
int ltr_plan_fields_stage(ltr_ctx* ctx, const LlSource& src, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result* res,
                          const DevReads& rd, const int32_t* d_map, const DevPass pass[2], DevLease& lease);
// ... of a batch without a single sample: the per-locus sizes, nothing to compute
void ltr_plan_fields_empty(const ltr_genotype_batch* gb, ltr_genotype_result* res);
#pragma GCC visibility pop
