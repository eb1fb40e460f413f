// ltr_plan_fields.h -- what ltr_plan_genotype.hip (the passes) and ltr_plan_fields.hip (the VCF fields of every locus of a
// genotyped plan) share: the result object and the launch of the fields kernel.
#pragma once

#include <memory>
#include <vector>

#include "ltr_ctx.h"

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
  int32_t haploid = 0;
  std::vector<int32_t> f_block, f_V;             // per locus: the block the fields are for, its alleles
  std::vector<int64_t> f_gl_off, f_pgl_off, f_read_off;   // [n_loci + 1]: gls / pls, phased_gls, reads
  std::unique_ptr<int32_t[]> f_i32;              // best_gts [2 nu], n_aligned, n_snp, n_s1, n_s2 [nu each], read_allele [reads]
  std::unique_ptr<double[]> f_f64;               // log_phased, log_unphased, hap_log_phased, hap_log_unphased, gl_diffs [nu each]
  std::unique_ptr<double[]> f_gls, f_pgls;       // when asked for
  std::unique_ptr<int32_t[]> f_pls;
};

namespace ltrf {

// one locus of the fields kernel
struct FieldLocus {
  int64_t ll_off, map_off;       // the locus block in the LL buffer ([P x H]); new_to_old in the map buffer, -1: identity
  int64_t tab_off;               // in the table buffer: hap_to_allele [Hn], allele_first [V + 1], haps_by_allele [Hn] (allele, then haplotype, ascending)
  int64_t gl_off, pgl_off;       // sample 0 of the locus in gls / pls and in phased_gls
  int32_t r0, r1, H, Hn, V, haploid, n_gl, n_pgl;
  double hom_gl, het_gl, hom_pgl, het_pgl;   // prior + configuration term of a homozygous / heterozygous cell (genotyper.cpp:204-241; host libm)
};
// one (locus, sample)
struct FieldUnit {
  int64_t post_off;              // its [Hn x Hn] block in the posterior buffer of its pass
  int64_t cell_off;              // its [V x V] genotype posteriors in the workspace; -1: they fit LDS
  int32_t locus, sample, out;    // out: slot in the per-unit outputs
  int32_t src, pass;             // slot in the total / best-pair buffers of pass 0 (first) or 1 (second)
};
struct FieldArgs {
  const FieldUnit* units; const FieldLocus* loci; const int32_t* tab;
  const double* ll; const int32_t* pool_index; const double* lp1; const double* lp2; const int32_t* label; const int32_t* map;
  const double* post[2]; const double* stl[2]; const int* gts[2];
  int32_t* best_gts; int32_t* counts;            // [2 nu]; n_aligned, n_snp, n_s1, n_s2: [4][nu]
  double* scalars;                               // log_phased, log_unphased, hap_log_phased, hap_log_unphased, gl_diffs: [5][nu]
  int64_t nu;
  double* gls; int32_t* pls; double* pgls;       // pls, pgls: null = not wanted
  double* cells; int32_t* read_allele;
};

constexpr int kFieldSmallH = 8;        // like the posterior passes: up to 8 haplotypes run in workgroups of one wavefront, the others of four
constexpr int kFieldCellCap = 2048;    // largest V x V table kept in LDS (16 KB)

// units [0, n_small) in workgroups of 64 threads, [n_small, n_small + n_large) of 256; cell_cap_*: doubles of LDS for the V x V table
void launch_fields(hipStream_t st, const FieldArgs& a, size_t n_small, int cell_cap_small, size_t n_large, int cell_cap_large);

}  // namespace ltrf
