/*
 * ltr_gpu_ploidy.h -- ploidy per (locus, sample): haploid and diploid samples in one locus.
 *
 * The reference decides ploidy per chromosome (--haploid-chrs, genotyper_bam_processor.cpp:248 -> :294); ltr_gpu.h's *_ploidy
 * entry points take it per locus.  On chrX a cohort of men and women has no correct value for either: the calls below take one
 * flag per (locus, sample).  They are defined in libltr_gpu.so next to the calls they extend and add to the interface of
 * ltr_gpu.h without changing it (its declarations, its structs and LTR_ABI_VERSION stay what they are).
 *
 *   sample_haploid   one byte per (locus, sample) in unit order -- locus-major, the samples of a locus in label order,
 *                    sum of pb->n_samples[] entries.  != 0 = that sample has one copy at that locus.  NULL = the call without it
 *                    (ltr_plan_posteriors / ltr_plan_genotype[_fields] / ltr_ll_genotype: pb->haploid for every locus).
 *                    With the array given pb->haploid is read only for a locus without a sample.
 *
 * What follows the sample: the priors of unit (locus, sample) in both passes (genotyper.cpp:21-33, seq_stutter_genotyper.cpp:405-408),
 * its GL / PL terms, its genotype index mapping and its strand rule in the fields (genotyper.cpp:132-256, seq_stutter_genotyper.cpp:
 * 965-967).  Samples of a locus meet only in pruning: the called alleles are the union over samples of the best pairs, and a
 * haploid sample's pair (a, a) calls a.
 *
 * A locus whose samples all have one ploidy is the per-locus case: the same path and the same bytes as *_ploidy with that
 * locus_haploid -- scores, genotypes, packed fields, widths and records.  ltr_genotype_result_haploid(r, l) is 1 exactly when
 * every sample of l is haploid, so it is 0 for a MIXED locus, which has the diploid shape everywhere:
 *   ltr_locus_fields   n_gl = V(V+1)/2, n_pgl = V*V.  A haploid sample's gls / pls row holds its V values in entries 0..V-1 and
 *                      0 after them; its phased_gls row is all 0.0 and is never printed.
 *   records            FORMAT GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF (+ the optional fields).  A haploid sample writes one
 *                      allele index in GT and one difference in GB; Q, DP, DFLANKINDEL, GLDIFF, ALLREADS, MALLREADS as in the
 *                      six-field haploid form; "." in PQ, DSNP, PDP, PSNP and PHASEDGL; V values in GL / PL; and it counts one
 *                      allele towards AN / AC.  Header lines are the same.
 * Errors are those of the calls they extend.
 */
#ifndef LTR_GPU_PLOIDY_H_
#define LTR_GPU_PLOIDY_H_

#include "ltr_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ltr_plan_posteriors with the priors of every unit following its sample */
int ltr_plan_posteriors_sample_ploidy(ltr_plan* plan, const ltr_posterior_batch* pb, const uint8_t* sample_haploid,
                                      double* post, double* sample_total_ll, int32_t* gts);
/* ltr_plan_genotype (fr == NULL) / ltr_plan_genotype_fields (fr given) */
int ltr_plan_genotype_sample_ploidy(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr,
                                    const uint8_t* sample_haploid, ltr_genotype_result** out);
/* ltr_ll_genotype */
int ltr_ll_genotype_sample_ploidy(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr,
                                  const uint8_t* sample_haploid, ltr_genotype_result** out);
/* the ploidy sample s of locus l was genotyped with, whichever entry point made the result: 0 / 1, negative for a bad index */
int32_t ltr_genotype_result_sample_haploid(const ltr_genotype_result* r, int64_t l, int32_t s);

#ifdef __cplusplus
}
#endif
#endif /* LTR_GPU_PLOIDY_H_ */
