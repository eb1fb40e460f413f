/*
 * ltr_snp.h -- phasing priors of reads from the heterozygous SNPs of a phased SNP VCF (host code, no GPU, no HIP).
 *
 * A restatement of the SNP half of SNPBamProcessor::process_reads (src/snp_bam_processor.cpp:35-124): create_snp_trees
 * (src/snp_tree.cpp:25-113) without a pedigree tracker, and calc_het_snp_factors for reads without mates
 * (src/snp_phasing_quality.cpp:4-120) with BaseQuality's tables (src/base_quality.h:29-75).  It lives in a library of its own
 * (libltr_snp.so, built from longtr_amd/snp/ltr_snp.cpp) so that libltr_gpu.so, its headers and its ABI version are exactly
 * what they were.  These reference units include htslib, so the restatement cannot be pinned to the compiled reference; only
 * the two base-quality tables can (ltr_snp_debug_quality_tables).  tests/snp_phasing_util.py restates the same lines a second
 * time, independently.
 *
 * The library reads no file.  The text of a window comes from the tabix-indexed reader of include/ltr_gpu.h: the "#CHROM" line
 * of the VCF's header and the record lines of one tabix query, each ending in '\n' (a last line may go without).
 *
 * ltr_snp_set_create, per record line (CHROM POS ID REF ALT QUAL FILTER INFO FORMAT sample...):
 *   - Samples are the columns after FORMAT of the #CHROM line, in order; a set holds one SNP list per COLUMN.  The index of a
 *     name follows std::map insertion (vcf_reader.cpp:108-111): for a name that occurs twice the LAST column wins.
 *   - Every record is parsed before it is judged, as the reference builds a Variant before it asks is_biallelic_snp: a record
 *     with fewer than 8 columns or an unreadable POS, with sample columns in the header and no GT key in FORMAT, with fewer
 *     sample columns than the header, with an allele that is neither '.' nor a number, or with an allele index that names no
 *     allele of the record (above 1 in a biallelic record) returns LTR_SNP_ERR_INVALID and names POS.  A header without sample
 *     columns asks nothing of FORMAT.
 *   - A record counts (n_valid_snps, the reference's locus_count) only if it is a biallelic SNP: exactly one ALT, REF and ALT
 *     one byte each, neither of them '*' or '.'.  bcf_is_snp of an unpinned htslib cannot be compiled here, so two rules are
 *     OURS: a '*' allele (the spanning deletion) is no SNP, and a symbolic ALT ("<X>", "<*>", more than one byte) is no SNP.
 *   - It must not lie in a skip region: POS >= skip_start - padding && POS <= skip_stop + padding, with POS as written in the
 *     file (1-based) against the 0-based starts the region file gives, as snp_tree.cpp:9-15 does.  The driver passes the
 *     region's own start / stop and padding 15 (snp_bam_processor.h:54).
 *   - Per sample column: the GT subfield is found by the position of GT in FORMAT (a sample field that ends before it is a
 *     missing call).  The alleles are cut at '/' and '|'.  A call with an allele '.' is missing; a call that is not exactly
 *     two alleles is skipped (the reference reads past its arrays there or ends the run); a call is phased iff the separator
 *     before its second allele is '|' (vcf_reader.cpp:55-70).  A phased call of two different alleles adds
 *     SNP(POS - 1, allele[gt_a][0], allele[gt_b][0]) to the column (snp_tree.cpp:61-72).
 *   - Per column the SNPs are kept sorted by position, STABLE in file order.  std::sort leaves ties open; they are fixed here
 *     because the order of the sums below decides their last bit.
 *
 * ltr_snp_phasing_priors, per read (calc_het_snp_factors, snp_phasing_quality.cpp:110-120):
 *   - the SNPs considered are those of the column with pos <= snp.pos <= end_pos - 1, ascending (:67);
 *   - extract_bases_and_qualities (:4-61), branch for branch, with cur = pos, i = 0 (index into the bases):
 *       M = X  snp.pos < cur + len: take base and quality at snp.pos - cur + i; else cur += len, i += len, next op
 *       D      snp.pos < cur + len: take '-'; else cur += len, next op
 *       I      i += len, next op
 *       S      snp.pos < cur: take '-'; else i += len, next op
 *       H      next op
 *       other  LTR_SNP_ERR_CIGAR -- only when met while SNPs are left, as the loop ends with the last SNP
 *     an index outside the bases (the reference's .at()) or a CIGAR that ends with SNPs left (its assert): LTR_SNP_ERR_INVALID;
 *   - for every base that is not '-': equal to base_one: log_p1 += correct(q), log_p2 += error(q); equal to base_two:
 *     log_p1 += error(q), log_p2 += correct(q); neither: both += error(q).  The sums start at 0.0 and run in SNP order (:73-91);
 *   - the tables: q is a `char` as the reference's compiler has it (signed: a byte above 127 is below '!'); q < '!' is index 0,
 *     q > 'J' is index 'J' - '!', else q - '!'.  log_correct[0] = -100, log_error[0] = 0, else
 *     log(1 - pow(10, i / -10.0)) and log(pow(10, i / -10.0 / 5.0)).
 */
#ifndef LTR_SNP_H_
#define LTR_SNP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LTR_SNP_OK           0
#define LTR_SNP_ERR_INVALID -1     /* = LTR_ERR_INVALID of ltr_gpu.h */
#define LTR_SNP_ERR_NOMEM   -4     /* = LTR_ERR_NOMEM */
#define LTR_SNP_ERR_CIGAR   -5     /* = LTR_ERR_CIGAR */

#define LTR_SNP_SKIP_PADDING 15    /* SKIP_PADDING, snp_bam_processor.h:54 */
#define LTR_SNP_N_QUALITIES  42    /* 'J' - '!' + 1 entries in each table */

typedef struct ltr_snp_set ltr_snp_set;

/* header_line: the "#CHROM ..." line.  record_lines[len]: the record lines of one window (len may be 0).  skip_start /
 * skip_stop[n_skip]: the regions whose padded span holds no SNP.  Errors: a status, a text in err (NUL-terminated, at most
 * err_cap bytes; err may be NULL) and *out left NULL. */
int ltr_snp_set_create(const char* header_line, const char* record_lines, int64_t len, const int32_t* skip_start,
                       const int32_t* skip_stop, int32_t n_skip, int32_t skip_padding, ltr_snp_set** out, char* err, int err_cap);
void        ltr_snp_set_free(ltr_snp_set* s);
int32_t     ltr_snp_set_n_samples(const ltr_snp_set* s);                            /* sample columns of the header */
const char* ltr_snp_set_sample_name(const ltr_snp_set* s, int32_t column);          /* "" when out of range */
int32_t     ltr_snp_set_sample_index(const ltr_snp_set* s, const char* name);       /* the column of a name (the last of several), -1 = absent */
int32_t     ltr_snp_set_n_valid_snps(const ltr_snp_set* s);                         /* locus_count: records that passed the record filter */
int32_t     ltr_snp_set_n_snps(const ltr_snp_set* s, int32_t column);               /* phased het SNPs of a column, -1 when out of range */
/* The SNPs of a column in their order: at most cap of them into pos (0-based) / base_one / base_two; returns how many were written. */
int32_t     ltr_snp_set_snps(const ltr_snp_set* s, int32_t column, int32_t* pos, char* base_one, char* base_two, int32_t cap);

/* The fields of an ltr_raw_alignment the walk reads. */
typedef struct ltr_snp_read {
  int32_t        pos, end_pos;   /* 0-based, end_pos exclusive */
  int32_t        length;
  const char*    bases;          /* [length] */
  const char*    quals;          /* [length] Phred + 33 */
  int32_t        n_cigar;
  const char*    cigar_type;     /* [n_cigar] */
  const int32_t* cigar_num;      /* [n_cigar] */
} ltr_snp_read;

/* log_p1 / log_p2[n_reads] of the reads of ONE sample against column vcf_sample.  vcf_sample < 0 (the sample is not in the
 * VCF) writes zeros (snp_bam_processor.cpp:74-81).  counts[3] (may be NULL) is ADDED to, as the reference adds to its match
 * and mismatch counters over the samples of a run: bases equal to base_one, equal to base_two, equal to neither.  On an
 * error nothing is added, log_p1 / log_p2 are undefined and err names the read. */
int ltr_snp_phasing_priors(const ltr_snp_set* s, int32_t vcf_sample, const ltr_snp_read* reads, int32_t n_reads, double* log_p1,
                           double* log_p2, int32_t* counts, char* err, int err_cap);

/* Test hook: the two tables, LTR_SNP_N_QUALITIES doubles each. */
void ltr_snp_debug_quality_tables(double* log_correct, double* log_error);

#ifdef __cplusplus
}
#endif
#endif /* LTR_SNP_H_ */
