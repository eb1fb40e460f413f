/*
 * ltr_filter.h -- the reference's read filter for one region (host code, no GPU, no HIP).
 *
 * A restatement of BamProcessor::read_and_filter_reads (src/bam_processor.cpp:188-487) for reads that are NOT flagged
 * paired, which is what long-read BAMs hold.  It lives in a library of its own (libltr_filter.so, built from
 * longtr_amd/filter/ltr_filter.cpp) so that libltr_gpu.so, its header and its ABI version are exactly what they were:
 * nothing here touches a kernel or a struct of include/ltr_gpu.h.  It cannot be pinned to the compiled reference, because
 * bam_processor.cpp includes htslib; tests/read_filter_util.py restates the same lines a second time, independently.
 *
 * Input: the records of ONE region in the order the reader delivers them file by file -- ltr_bam_open(...,
 * merge_by_position = 0), the ORDER_ALNS_BY_FILE the reference asserts at :193 -- fetched with
 * ltr_bam_set_region(chrom, max(0, start - 1000), stop + 1000) (:586-587, MAX_MATE_DIST).
 *
 * Per record, in the reference's order:
 *   1. pos > stop || end_pos < start: LTR_FILTER_OUTSIDE (:208-215, the rule for a read without a mate).
 *   -  BAM flag 0x1: LTR_FILTER_PAIRED_UNSUPPORTED, dropped and counted.  The mate-pair branches of the reference
 *      (:96-150, :324-417) serve its short-read ancestor and are not restated; such a record takes no further part
 *      (it neither changes the file label nor enters the maps below).
 *   2. more than max_total_reads reads held: too_many_reads is set and the scan ends (:217-220); the records not reached
 *      are LTR_FILTER_NOT_SCANNED.  The reference counts paired_str_alns there, which reads without mates never enter,
 *      so for them its stop cannot fire; here the count is that of the reads held so far (potential_strs), the
 *      single-end reads the limit is meant to bound.
 *   3. unmapped (0x4), pos == 0, no CIGAR or length 0: LTR_FILTER_SKIPPED, silently (:222).
 *   4. pos < stop && end_pos >= start, base_qual_trim > ' ', CIGAR starts or ends with H: LTR_FILTER_HARD_CLIPPED (:228-235).
 *   -  the file label "<k>_" changes here, k = 1, 2, ... at every change of file among the records that get this far (:247-254).
 *   5. not (pos < stop && end_pos >= start): LTR_FILTER_OUTSIDE (:257, :385-417: such a read is only remembered as a
 *      possible mate, which has no effect for reads without mates).
 *   6. the first failing test of :265-284: HAS_N_BASES, LOW_BASE_QUALS (mean of qual - '!' < min_mean_qual,
 *      base_quality.h:77-84), LOW_MAPQ (mapq < min_mapq), NOT_SPANNING (require_spanning == 1 and not
 *      pos <= start && end_pos >= stop, :175-186).
 *   7. a passing read's PF flag (:289-318) is set unless min_flank > 0 and (pos > start - min_flank || end_pos < stop +
 *      min_flank); it is ltr_raw_alignment.use_for_hap_generation.
 * Bookkeeping (:321-383, :420-437): key = file label + name (a trailing "/x" cut, :163-170).  A passing read enters the
 * map potential_strs, which keeps the FIRST read of a key (a later one: LTR_FILTER_DUPLICATE_NAME); a failing read enters
 * potential_mates (cleared at a change of file), from where a later passing read of that key erases it.  At the end a held
 * read with an XA tag is LTR_FILTER_NO_UNIQUE_MAPPING, the rest pass.
 * Output order (:452-483): the passing reads in std::map order of the key STRING ("10_" < "2_"), handed out from the BACK,
 * grouped by sample in order of first appearance in that walk.  The sample is the SM of the read's RG tag in its file's
 * header (get_read_group :153-161) or, with --bam-samps, the sample given for the file.
 */
#ifndef LTR_FILTER_H_
#define LTR_FILTER_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LTR_FILTER_OK           0
#define LTR_FILTER_ERR_INVALID -1     /* = LTR_ERR_INVALID of ltr_gpu.h */

enum {
  LTR_FILTER_PASS = 0, LTR_FILTER_OUTSIDE = 1, LTR_FILTER_NOT_SCANNED = 2, LTR_FILTER_SKIPPED = 3, LTR_FILTER_HARD_CLIPPED = 4,
  LTR_FILTER_HAS_N_BASES = 5, LTR_FILTER_LOW_BASE_QUALS = 6, LTR_FILTER_LOW_MAPQ = 7, LTR_FILTER_NOT_SPANNING = 8,
  LTR_FILTER_NO_UNIQUE_MAPPING = 9, LTR_FILTER_DUPLICATE_NAME = 10, LTR_FILTER_PAIRED_UNSUPPORTED = 11
};
/* the counters the reference logs at :440-450, + the paired records dropped */
enum {
  LTR_FILTER_N_OVERLAPPED = 0, LTR_FILTER_N_HARD_CLIPPED = 1, LTR_FILTER_N_HAS_N = 2, LTR_FILTER_N_LOW_MAPQ = 3, LTR_FILTER_N_LOW_QUAL = 4,
  LTR_FILTER_N_NOT_SPANNING = 5, LTR_FILTER_N_NOT_UNIQUE = 6, LTR_FILTER_N_PASSED = 7, LTR_FILTER_N_PAIRED = 8, LTR_FILTER_N_COUNTERS = 9
};

/* bam_processor.h:82-101 */
typedef struct ltr_filter_options {
  int32_t min_mapq;          /* MIN_MAPQ 20 */
  double  min_mean_qual;     /* MIN_SUM_QUAL_LOG_PROB 30 */
  int32_t require_spanning;  /* REQUIRE_SPANNING 1 */
  int32_t min_flank;         /* MIN_FLANK 5 */
  int32_t max_total_reads;   /* MAX_TOTAL_READS 1000000 */
  int32_t base_qual_trim;    /* BASE_QUAL_TRIM '5' (a character code) */
} ltr_filter_options;
void ltr_filter_default_options(ltr_filter_options* opt);

/* The fields of an ltr_bam_record the filter reads, and the two tags. */
typedef struct ltr_filter_record {
  const char* name;
  int32_t     file_index;
  int32_t     pos, end_pos;
  int32_t     mapq, flag;
  int32_t     length;
  const char* bases;        /* [length] */
  const char* quals;        /* [length] Phred + 33 */
  int32_t     n_cigar;
  const char* cigar_type;   /* [n_cigar] */
  const char* rg;           /* the RG tag, NULL when absent */
  int32_t     has_xa;       /* HasTag("XA") */
} ltr_filter_record;

/* Which sample a read belongs to.  use_rgs != 0: the read-group table of the header(s), as ltr_bam_read_group_* gives it
 * (id, sample, file of each @RG line).  use_rgs == 0 (--bam-samps): file_sample[file_index]. */
typedef struct ltr_filter_samples {
  int32_t            use_rgs;
  int32_t            n_rg;
  const char* const* rg_id;
  const char* const* rg_sample;
  const int32_t*     rg_file;
  int32_t            n_files;
  const char* const* file_sample;
} ltr_filter_samples;

typedef struct ltr_filter_result ltr_filter_result;
/* opt NULL = the defaults.  Errors: LTR_FILTER_ERR_INVALID and a text in err (NUL-terminated, at most err_cap bytes; err
 * may be NULL), *out left NULL; where the reference would end the process (a passing read without an RG tag, or with one
 * no header names, while RG mapping is in force, :155-159) the text is its message. */
int ltr_filter_reads(const ltr_filter_record* recs, int32_t n_recs, int32_t region_start, int32_t region_stop,
                     const ltr_filter_options* opt, const ltr_filter_samples* samples, ltr_filter_result** out, char* err, int err_cap);
void           ltr_filter_result_free(ltr_filter_result* r);
int32_t        ltr_filter_result_n_records(const ltr_filter_result* r);
const uint8_t* ltr_filter_result_verdicts(const ltr_filter_result* r);       /* [n_records] LTR_FILTER_* */
int32_t        ltr_filter_result_n_passing(const ltr_filter_result* r);
const int32_t* ltr_filter_result_pass_record(const ltr_filter_result* r);    /* [n_passing] record index, in output order */
const int32_t* ltr_filter_result_pass_sample(const ltr_filter_result* r);    /* [n_passing] index into the sample names */
const uint8_t* ltr_filter_result_pass_pf(const ltr_filter_result* r);        /* [n_passing] use_for_hap_generation */
int32_t        ltr_filter_result_n_samples(const ltr_filter_result* r);
const char*    ltr_filter_result_sample_name(const ltr_filter_result* r, int32_t i);
const int32_t* ltr_filter_result_counters(const ltr_filter_result* r);       /* [LTR_FILTER_N_COUNTERS] */
int32_t        ltr_filter_result_too_many_reads(const ltr_filter_result* r);
const char*    ltr_filter_verdict_name(int32_t verdict);                     /* "PASS", "HAS_N_BASES", ...; "" when unknown */

#ifdef __cplusplus
}
#endif
#endif /* LTR_FILTER_H_ */
