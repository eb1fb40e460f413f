/*
 * ltr_gpu.h -- C-ABI of the MI355X (gfx950) read-vs-haplotype alignment library.
 *
 * This is the drop-in boundary for ONE path of gymrek-lab/LongTR: the batch
 * driver HapAligner::process_reads and the pair-HMM DP it runs for every
 * (pooled read, candidate haplotype) pair, plus the two thin consumers either
 * side of it.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 *   reference call site    src/seq_stutter_genotyper.cpp:517-523
 *   reference callee       src/SeqAlignment/HapAligner.h:137-138 (process_reads)
 *                          src/SeqAlignment/HapAligner.cpp:236-343 (align_seq_to_hap)
 *
 * Plain pointers and sizes only; no C++/torch types.  The library never
 * exits the process (the reference does, src/error.cpp:6-10): every function
 * returns an ltr_status and ltr_last_error() holds the text.
 *
 * Threads.  The reference is single-threaded and its HapAligner is not re-entrant (it advances the Haplotype's
 * iterator, HapAligner.cpp:852-853).  Here any number of host threads may use ONE context: plan creation is
 * serialised inside the library (the context's work arrays); ltr_calc_hap_aln_probs and ltr_haplotype_align_to_ref,
 * which stage in buffers the context keeps, run one at a time per context (a second caller waits); executes of
 * DIFFERENT plans may be queued side by side; ONE plan is driven by one thread at a time.  ltr_ctx_set_params /
 * ltr_ctx_set_pair_packing / ltr_ctx_set_debug while another thread is inside a call on the same context is the
 * caller's race.  Threads that should score at the same time take a context each.
 *
 * There is NO CPU fallback behind these entry points: if no HIP device (or no
 * gfx950 code object) is available the compute calls fail with
 * LTR_ERR_NO_DEVICE.
 */
#ifndef LTR_GPU_H_
#define LTR_GPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
#define LTR_OK              0
#define LTR_ERR_INVALID    -1   /* bad argument / malformed batch                       */
#define LTR_ERR_NO_DEVICE  -2   /* no usable HIP device: the product path has no CPU fallback */
#define LTR_ERR_HIP        -3   /* a HIP runtime call failed                            */
#define LTR_ERR_NOMEM      -4
#define LTR_ERR_CIGAR      -5   /* CIGAR op outside MIDNSHP=X handled by trim_alignment
                                   (reference: printErrorAndDie, HapAligner.cpp:375)     */
#define LTR_ERR_UNSUPPORTED -6  /* e.g. a short-path locus that is not [flank][repeat][flank] */

/* ---- sentinels the reference writes as values (reproduced, never errors) -- */
#define LTR_IMPOSSIBLE     (-1000000000.0) /* HapAligner.cpp:20, haplotype <= 60 bp (:241-244)   */
#define LTR_ABORT_SCORE    (-700.0)        /* |n-m| > 600 (:249-252) and row abort (:300-306)    */

typedef struct ltr_ctx  ltr_ctx;    /* one per GPU; owns device memory, streams, model tables */
typedef struct ltr_plan ltr_plan;   /* one packed + uploaded batch, resident in HBM            */

/*
 * Alignment model.  Replaces class AlignmentModel (HapAligner.h:12-37) and the
 * two ints HapAligner carries (HapAligner.h:50-51).  The seven transitions stay
 * FLOAT on purpose: the reference stores them as float and promotes to double
 * inside the recurrence, and bit-exact parity depends on reproducing that.
 * Order = --alignment-params order (hipstr_main.cpp:419-439).
 */
typedef struct ltr_align_params {
  float   log_ins_to_ins;      /* a */
  float   log_ins_to_match;    /* b */
  float   log_del_to_del;      /* c */
  float   log_del_to_match;    /* d */
  float   log_match_to_match;  /* e */
  float   log_match_to_ins;    /* f */
  float   log_match_to_del;    /* g */
  int32_t indel_flank_len;     /* INDEL_FLANK_LEN, CLI default 5 (hipstr_main.cpp:324-326) */
  int32_t use_short_path;      /* SWITCH_OLD_ALIGN_LEN used as a bool (HapAligner.cpp:552) */
} ltr_align_params;

/* Fills the defaults of HapAligner.h:118 and indel_flank_len=5, use_short_path=0. */
void ltr_default_params(ltr_align_params* p);

/*
 * A batch of loci, flattened.  One locus = the inputs of one
 * HapAligner::process_reads call: P pooled, TRIMMED reads (the output of
 * HapAligner::trim_alignment, :346-465) and H candidate haplotype strings in
 * Haplotype::next() order (Haplotype.cpp:151-196), each the FULL haplotype
 * (35-bp flanks included; the library cuts hap[30:len-30] itself like :245-246).
 *
 * Output layout: for locus l the P_l x H_l log-likelihood matrix is row-major
 * at out_ll + ll_off[l], ll_off[l] = sum_{k<l} P_k*H_k  -- i.e. exactly
 * aln_probs[(pool)*H + hap] of HapAligner.cpp:550 per locus, loci back to back.
 */
typedef struct ltr_locus_batch {
  int64_t        n_loci;
  const int64_t* locus_read_off;  /* [n_loci+1] first read index of each locus            */
  const int64_t* locus_hap_off;   /* [n_loci+1] first haplotype index of each locus       */
  int64_t        n_reads;         /* = locus_read_off[n_loci]                             */
  const uint8_t* read_bytes;      /* concatenated trimmed read sequences                  */
  const int64_t* read_off;        /* [n_reads+1] byte offsets into read_bytes             */
  int64_t        n_haps;          /* = locus_hap_off[n_loci]                              */
  const uint8_t* hap_bytes;       /* concatenated full haplotype sequences                */
  const int64_t* hap_off;         /* [n_haps+1] byte offsets into hap_bytes               */
  const uint8_t* realign_read;    /* optional [n_reads]; 0 => row left untouched
                                     (HapAligner.cpp:557-560). NULL = all 1.              */
  const uint8_t* realign_hap;     /* optional [n_haps]; 0 => column left untouched
                                     (HapAligner.cpp:841-845). NULL = all 1.              */
} ltr_locus_batch;

/* ---- context ------------------------------------------------------------- */
/* device_ordinal: HIP device index (one process per GPU: pass LOCAL_RANK). */
int  ltr_ctx_create(int device_ordinal, ltr_ctx** ctx);
void ltr_ctx_destroy(ltr_ctx* ctx);
/* Replaces the alignment_model_params_ argument of the HapAligner constructor
 * (HapAligner.h:94-120).  Rebuilds the device-side boundary tables. */
int  ltr_ctx_set_params(ltr_ctx* ctx, const ltr_align_params* p);
const char* ltr_last_error(const ltr_ctx* ctx);
/* "gfx950" etc. of the device the context is bound to; number of CUs; shader clock in MHz. */
int  ltr_ctx_device_info(const ltr_ctx* ctx, char* arch, int arch_len, int* n_cu, int* clock_mhz);

/* ---- one-shot: host buffers in, host buffers out -------------------------- */
/*
 * Replaces the compute of HapAligner::process_reads (HapAligner.cpp:545-581,
 * long path) for a whole batch of loci.  out_ll: sum_l P_l*H_l doubles (cells
 * whose row/column mask is 0 are NOT written, like the reference).  out_seed:
 * n_reads ints, seed_positions[] of :562-563 (= trimmed length - 1 ... see
 * note in DESIGN.md; written only for realigned reads).  May be NULL.
 */
int ltr_align_batch(ltr_ctx* ctx, const ltr_locus_batch* batch,
                    double* out_ll, int32_t* out_seed);

/* ---- resident plan: pack + upload once, execute many times ---------------- */
int     ltr_plan_create(ltr_ctx* ctx, const ltr_locus_batch* batch, ltr_plan** plan);
void    ltr_plan_destroy(ltr_plan* plan);
int64_t ltr_plan_num_pairs(const ltr_plan* plan);   /* pairs with both masks set            */
int64_t ltr_plan_ll_size(const ltr_plan* plan);     /* number of doubles in the LL buffer   */
double  ltr_plan_cells(const ltr_plan* plan);       /* nominal DP cells, n*m per non-shortcut pair
                                                       (BASELINE.md definition)             */
double  ltr_plan_input_bytes(const ltr_plan* plan); /* algorithmic HBM bytes of one execute:
                                                       sum m + sum n + 8*P*H per locus      */
/*
 * Launch the alignment kernels for the whole plan on `stream` (a hipStream_t
 * passed as void*; NULL = the context's own stream).  Asynchronous.  d_out_ll:
 * device pointer to ltr_plan_ll_size() doubles, or NULL to use the plan's own
 * device buffer.  Inputs are already resident in HBM.
 */
int ltr_plan_execute(ltr_plan* plan, double* d_out_ll, void* stream);
/* Waits for the last execute and copies results to host (either may be NULL). */
int ltr_plan_fetch(ltr_plan* plan, double* out_ll, int32_t* out_seed);
/* Device time of the DP kernels of the last execute, measured with HIP events
 * recorded on the launch stream; n_launches = kernel launches it took. */
int ltr_plan_last_kernel_ms(ltr_plan* plan, float* ms, int* n_launches);
/* The DP runs as one launch per strip-width class (k = 0 .. ltr_num_kernels()-1, read
 * columns per lane = *strip_width; 0 = chosen per pair).  Per class: pairs, nominal cells, and the device time of
 * its launch in the last execute (HIP events on the launch stream). */
int ltr_num_kernels(void);
/* Lanes that share one pair in class k: 64 (one pair per wavefront), 2 .. 32 (packed classes: 64 / lanes
 * short reads per wavefront, each on a segment of the lanes with wider strips), 256 / 512 (a workgroup per pair). */
int ltr_kernel_lanes_per_pair(int k);
/* Kernel family of class k: 0 one pair per wavefront, 1 several pairs per wavefront (packed), 2 one pair per workgroup
 * (certificate kernels); 3 exact (redo) kernels -- the classes at the end of the list: pairs a certificate
 * could not clear, by read length, plus the byte-compare kernel for pairs with bytes outside ACGT.  For
 * them ltr_plan_kernel_stats reports the pairs they scored in the last execute (cells: only of the
 * pairs that start out in their lists). */
int ltr_kernel_family(int k);
/* Per-launch HIP events cost a few microseconds each: off by default, switch on before the
 * executes whose ltr_plan_kernel_stats times you want. */
int ltr_plan_set_timing(ltr_plan* plan, int on);
int ltr_plan_kernel_stats(ltr_plan* plan, int k, int* strip_width, int64_t* n_pairs, double* cells, float* ms);
/* Launches that score several classes: the several-pairs-per-wavefront kernels run ONE launch per strip width over up to five
 * ranges of pairs (32, 16, 8, 4, 2 lanes per pair), and in automatic mode the one-pair-per-wavefront classes of strip widths
 * 11 .. 20 are ONE persistent launch that walks them widest first.  ltr_plan_kernel_stats reports such a launch under its first
 * class that has pairs, the others report zero.  Returns the number of ranges of class k's launch (0: k is not such a class)
 * and fills lanes_per_pair / strip_width / n_pairs (room for ltr_num_kernels() each) in launch order.  (In automatic mode the
 * packed launches of strip widths 13 .. 20 are one persistent launch as well; and every plan of the automatic mode, whatever its
 * size and indel model, runs EVERY one-wave class and packed width as one launch, the plan kernel -- csrc/ltr_dp_plan.hpp -- which
 * also scores the pairs whose certificate fails itself: its ranges are the one-wave classes, then the packed widths.)
 * ltr_plan_set_timing: on = 1 times every launch as it is launched; on = 2 launches the multi-width launch class by class
 * (the single-class kernels: the same bodies) so that every class has a time of its own. */
int ltr_plan_kernel_ranges(ltr_plan* plan, int k, int32_t* lanes_per_pair, int32_t* strip_width, int64_t* n_pairs);
/* The class the plan kernel's launch is reported under by ltr_plan_kernel_stats / _ranges (-1: this plan runs a launch per class). */
int ltr_plan_kernel_class(const ltr_plan* plan);
/* Haplotype families (csrc/ltr_dp_family.hpp): in automatic mode, under a symmetric indel model, the pairs of one pooled read of
 * 641 .. 1280 columns against several haplotypes of its locus are scored by a launch of their own, listed under a class of its own
 * (family 2 in ltr_kernel_family), that runs the rows the haplotype windows share once per read; a member it cannot prove
 * bit-identical to the unshared DP is scored again by the exact body.  ltr_ctx_set_debug "families" (-1 never, 0 by rule, 1 whenever
 * one can be formed) and "family_min_rows" (fewest shared rows; 0: the rule's 64) act on the plans created afterwards.
 * out5 = families, member pairs of the plan; of its last execute: families whose stem certificate failed (all members to the exact
 * body), members the acceptance rule sent there, members whose tail certificate failed. */
int ltr_plan_family_stats(ltr_plan* plan, int64_t* out5);
/* Families run along a SPINE (csrc/ltr_dp_family.hpp, spine_walk): where members fork from each other beyond the family's fork row,
 * the stream follows one member's window to its end and the others leave it at the row where they leave that member, so the rows
 * longer alleles share are scored once as well.  ltr_ctx_set_debug "family_spine": -1 never (plain families), 0 by rule (plans that form
 * at least 24 families per CU), 1 in any plan.
 * out2 = families of the plan that run along a spine, modelled wavefront steps that saves against plain families. */
int ltr_plan_family_spine_stats(const ltr_plan* plan, int64_t* out2);
/* Measurement aid: with ltr_ctx_set_debug(ctx, "wave_clock", 1) set when the plan was created, the plan kernel records the wall
 * clock (100 MHz) at which every one of its wavefronts started and left, and what it spent in the exact body: out = {first, last,
 * pairs scored with the exact body, ticks spent there} per wavefront of the last execute, then 4096 words: a count and
 * (n << 32 | m) of the pairs that took the exact body, then 256 words: per entry of the plan kernel's table (ltr_plan_debug_entries) the
 * ticks all wavefronts together spent in it.  cap (64-bit words) must hold 4 x wavefronts + 4096 + 256.
 * Returns the number of wavefronts written (0: not recorded), negative on error.
 * (Under the same knob the family launch records its wavefronts' first and last clock in a buffer of its own: the hook
 * ltr_debug_family_wave_clocks, csrc/ltr_plan.h.) */
int ltr_plan_debug_wave_clocks(ltr_plan* plan, uint64_t* out, int64_t cap);
/* The plan kernel's table, in walk order: kind (0 one pair per wavefront, 1 packed strip width, 2 pairs that start with the exact
 * body, 3 = 0 by the chained walk), strip width, pairs, nominal cells of every entry.  Returns the number of entries. */
int ltr_plan_debug_entries(const ltr_plan* plan, int32_t* kind, int32_t* strip_width, int64_t* n_pairs, double* cells, int cap);

/* ---- planning units (host only, no GPU needed): which kernel scores a pair, in what order ------------------
 * ltr_plan_create = validate -> one launch class + launch-order key per pair -> counting sort by class, longest
 * first inside a class -> upload.  The rule and the sort are plain host functions (csrc/ltr_plan_rules.cpp, ltr_plan_sort.cpp); these entry
 * points expose them to the CPU tests.  They decide scheduling only: every kernel returns the reference's bits
 * (HapAligner.cpp:236-343).
 *   ltr_debug_class_info   family (ltr_kernel_family), strip width, waves per pair, lanes per pair of class k
 *   ltr_debug_classify     the class / order key / exact list of ONE pair of a batch with `pairs_in_batch` pairs
 *                          (`long_pairs_in_batch` of them with reads over 1281 bases) on a GPU of n_cu CUs under
 *                          ltr_ctx_set_pair_packing mode `mode`; window_len = haplotype window (0 when
 *                          hap_full_len <= 60), generic = bytes outside ACGT
 *   ltr_debug_sort_by_class  order[i] = pair at sorted position i; class_first[k] .. class_first[k+1] = class k;
 *                          fold: 0 = none; 1 = under-filled classes are folded into the next wider one (automatic mode, a
 *                          launch per class); 2 = the same where the widths 11.. / 13.. share a multi-width launch (nothing is
 *                          folded inside those); 3 = under the plan kernel (one launch for every one-wave and packed class:
 *                          only the workgroup families fold) */
int ltr_debug_num_classes(void);
int ltr_debug_class_info(int k, int* family, int* strip_width, int* waves_per_pair, int* lanes_per_pair);
int ltr_debug_classify(const ltr_align_params* p, int mode, int n_cu, int64_t pairs_in_batch, int64_t long_pairs_in_batch,
                       int32_t window_len, int32_t read_len, int32_t hap_full_len, int generic,
                       int* launch_class, int* order_key, int* exact_list);
int ltr_debug_sort_by_class(const int16_t* launch_class, const int16_t* order_key, int64_t n_pairs, int fold, int n_cu,
                            int32_t* order, int32_t* class_first);
/* The modelled launch time (wave-cycles: steps x (strip width + per-step overhead) x the share of the wavefront the pair holds) the
 * launch-order key is the logarithm of, for n pairs at once: what a host shards a catalogue by (longtr_amd/shard.py). */
int ltr_debug_pair_costs(const ltr_align_params* p, int mode, int n_cu, int64_t pairs_in_batch, int64_t long_pairs_in_batch, int64_t n,
                         const int32_t* window_len, const int32_t* read_len, const int32_t* hap_full_len, double* cost);
/* The exact kernels' row test as a table: entry k + H (H = half the returned length) = the smallest double x with
 * fl(x + (double)((float)|k| * log_del_to_del)) >= -600, +inf where no negative cell value can pass (the reference's abort test,
 * HapAligner.cpp:297-306, only compares the row maximum with -600).  Returns the table's length (cap must be >= 2110). */
int ltr_debug_threshold_table(float log_del_to_del, double* out, int64_t cap);
/* The seeded path's host-side seed choice = HapAligner::calc_seed_base + calc_best_seed_position (HapAligner.cpp:467-542):
 * index of the seed base in the read, -1 none, -2 a CIGAR op the reference dies on (forward declarations: types below). */
struct ltr_alignment;
struct ltr_haplotype_blocks;
int ltr_debug_calc_seed_base(const struct ltr_alignment* aln, const struct ltr_haplotype_blocks* hap);
/* The host-thread budget (see "host threads" below) as the CPU tests see it: the number of distinct threads a parallel loop of
 * n_items really ran on under a budget of n_threads (0: the rule) in worker pool which_pool (0 / 1), and whether
 * ltr_calc_hap_aln_probs stages its next chunk on a helper thread under that budget (1 / 0). */
int ltr_debug_parallel_threads(int n_threads, int64_t n_items, int which_pool);
int ltr_debug_prep_ahead_rule(int n_threads);

/* ---- host-side mirror of the reference objects (flattened) ---------------- */
/*
 * One haplotype = an ordered list of blocks (Haplotype.h:12-16); block b has
 * n_alleles[b] alternative sequences (HapBlock.h:19-21; allele 0 = reference)
 * and reference coordinates [start,end).  is_repeat marks RepeatBlock
 * (RepeatBlock.h:15).  Sequences of all alleles of all blocks are concatenated
 * in (block, allele) order.
 */
typedef struct ltr_haplotype_blocks {
  int32_t        n_blocks;
  const int32_t* block_start;     /* [n_blocks] HapBlock::start()                */
  const int32_t* block_end;       /* [n_blocks] HapBlock::end()                  */
  const uint8_t* is_repeat;       /* [n_blocks] get_repeat_info() != NULL        */
  const int32_t* period;          /* [n_blocks] repeat period (0 for flanks)     */
  const int32_t* n_alleles;       /* [n_blocks] HapBlock::num_options()          */
  const uint8_t* allele_bytes;    /* concatenated allele sequences               */
  const int64_t* allele_off;      /* [sum n_alleles + 1]                         */
} ltr_haplotype_blocks;

/* class Alignment (AlignmentData.h:28-140): the fields the path reads. */
typedef struct ltr_alignment {
  int32_t        start;           /* get_start()  */
  int32_t        stop;            /* get_stop()   */
  const uint8_t* seq;             /* get_sequence() */
  int32_t        seq_len;
  int32_t        n_cigar;
  const char*    cigar_type;      /* [n_cigar] CigarElement::get_type() */
  const int32_t* cigar_num;       /* [n_cigar] CigarElement::get_num()  */
  const uint8_t* qual;            /* get_base_qualities(), Phred+33, seq_len bytes; only the short
                                     (stutter) path reads it -- may be NULL on the long path */
} ltr_alignment;

/* Stutter model of the short path.  Replaces StutterModel (stutter_model.h:35-62); the CLI always
 * installs (0.95, 0.05, 0.05, 0.95, 0.01, 0.01) (hipstr_main.cpp:140,362-363). */
typedef struct ltr_stutter_params {
  double in_geom, in_up, in_down;      /* in-frame geometric parameter, P(up), P(down)     */
  double out_geom, out_up, out_down;   /* out-of-frame                                      */
} ltr_stutter_params;
void ltr_default_stutter_params(ltr_stutter_params* p);
int  ltr_ctx_set_stutter_params(ltr_ctx* ctx, const ltr_stutter_params* p);
/* Scheduling knob, results never depend on it.  Reads of up to 641 bases can share a wavefront
 * with other pairs (segments of 32 .. 2 lanes each): better throughput, longer latency per pair.  Reads longer
 * than 1281 bases are scored by a whole workgroup (4 or 8 wavefronts, boundary columns handed
 * over through LDS) while there are fewer than 10 such pairs per CU, else as several column
 * blocks on one wavefront each; reads of 3586 .. 5121 bases by four-wave workgroups with wide strips up to 80
 * long pairs per CU, for as many whole rounds of workgroups as the batch fills.
 *   -1 (default) automatic: several pairs per wavefront from 32 pairs per CU up, the fewer lanes per pair the more
 *                pairs of that length the batch holds; launch classes that cannot fill the GPU a few times over
 *                are folded into the next wider class; from 16 pairs per CU up the launches of a plan are dealt
 *                over four streams of the context
 *    0 / 1       packed kernels never / 32 lanes per pair whenever the read fits (one class per strip width, one stream)
 *    2           workgroup kernels wherever they exist: reads over 1025 bases, and the one-wave variant for every
 *                read of up to 1025 bases (inputs streamed through LDS; A/B and tests -- slower than the default)
 *    3           no workgroup kernels at all (long reads walk their column blocks on one wavefront)
 *    4           no certificate kernels: every pair goes straight to the exact kernels (the reference's
 *                cell-by-cell row maximum) -- verification, and the rate of the exact kernels by themselves
 *    5 .. 8      packed kernels with 16 / 8 / 4 / 2 lanes per pair whenever the read fits that many lanes of up
 *                to 20 columns (else the next wider segment; beyond 641 bases one pair per wavefront)
 * Workgroup kernels exist for symmetric indel models (ins->match == del->match, match->ins ==
 * match->del: the defaults); a plan that uses them must be re-created if ltr_ctx_set_params switches
 * to an asymmetric model (ltr_plan_execute reports LTR_ERR_INVALID otherwise); so must a plan with
 * haplotype families or, under ltr_ctx_set_debug "chain", with entries of the chained walk. */
int  ltr_ctx_set_pair_packing(ltr_ctx* ctx, int mode);
/* Measurement switches (A/B runs, profile collection); results never depend on them; value 0 = the library's rule.
 *   "fan_lanes"      streams the certificate launches of a plan are dealt over (1 .. 4; rule: 2) -- profiles/collect.sh
 *                    sets 1 so that every launch's own duration is what rocprofv3 and the per-launch HIP events see
 *   "fan_pairs"      plans with at least this many pairs stay on one stream
 *   "chunks", "chunk_streams", "chunk_growth"   ltr_calc_hap_aln_probs: chunk count / streams / size progression
 *   "trace"          1: ltr_calc_hap_aln_probs prints a timestamped phase profile to stderr
 *   "wg_first_pass"  first pass of the workgroup-per-pair classes (long reads): 1 = always the certificate kernels, 2 = always the
 *                    threshold kernels; rule: what the context has learnt, see ltr_ctx_wg_first_pass
 *   "poa_group_cap_bytes", "poa_call_budget_bytes"   ltr_poa_consensus: its memory rule, lowered (see there; the cap decides which
 *                    groups are aligned, so this one switch does change results)
 *   "grid_cap"       n > 0: every DP launch of ltr_plan_execute (of plans created from now on) and every class launch of
 *                    ltr_haplotype_align_to_ref on at most n workgroups, and whatever is sized by a grid with it -- the tests'
 *                    way to many items per persistent wavefront on a device of any size (tests/test_gpu_grid_cap.py)
 *   "reset"          every switch back to the library's rule */
int  ltr_ctx_set_debug(ltr_ctx* ctx, const char* key, double value);
/* Which kernels score the workgroup-per-pair classes (reads beyond 1281 bases, symmetric models) FIRST in the next
 * ltr_plan_execute: 0 = the certificate kernels (11 operations a cell; a pair whose certificate fails -- it would abort in the
 * reference, HapAligner.cpp:297-306, or comes close -- is scored again by an exact kernel), 1 = the threshold kernels (13
 * operations a cell, exact in one pass).  The context LEARNS it from the reads: every execute leaves the number of pairs its
 * first pass could not finish; more than half of them failing switches to the threshold kernels, fewer than a quarter aborting
 * switches back; ltr_ctx_set_params forgets it.  HiFi reads finish (0); ONT reads under the default model abort (1: every pair
 * of BASELINE config 5).  Scores never depend on it.  last_unfinished / last_scored (optional): the counts of the last execute
 * that has been read.  The query waits for the statistics of the executes queued so far (ltr_plan_execute never waits: it reads
 * what has arrived).  Returns 0 / 1, or a negative error. */
int  ltr_ctx_wg_first_pass(ltr_ctx* ctx, int64_t* last_unfinished, int64_t* last_scored);

/*
 * HapAligner::process_reads (HapAligner.h:137-138, .cpp:545-581) for one locus:
 * trims every alignment on the host exactly like trim_alignment (:346-465,
 * incl. the 10-bp substitute for an empty trim, :820-823), enumerates the
 * haplotypes in Haplotype::next() order and scores all pairs on the GPU.
 * aln_probs[(init_read_index+i)*H + k] and seed_positions[init_read_index+i]
 * are written for realign_read[i] != 0 and realign_to_hap[k] != 0 only.
 */
int ltr_process_reads(ltr_ctx* ctx, const ltr_haplotype_blocks* hap,
                      const uint8_t* realign_to_hap,
                      const ltr_alignment* alns, int32_t n_alns, int32_t init_read_index,
                      const uint8_t* realign_read,
                      double* aln_probs, int32_t* seed_positions);

/* Number of haplotype combinations (Haplotype::num_combs) and the k-th
 * haplotype string in Haplotype::next() order; used by callers that need to
 * flatten several loci into one ltr_locus_batch themselves. */
int64_t ltr_haplotype_num_combs(const ltr_haplotype_blocks* hap);
/* Writes haplotype `index` into out (capacity cap); returns its length or <0. */
int64_t ltr_haplotype_seq(const ltr_haplotype_blocks* hap, int64_t index, uint8_t* out, int64_t cap);
/* HapAligner::trim_alignment (:346-465): returns ltrim/rtrim (bases cut left/right). */
int ltr_trim_alignment(const ltr_alignment* aln, int32_t repeat_start, int32_t repeat_end,
                       int32_t indel_flank_len, int32_t* ltrim, int32_t* rtrim);
/* ReadPooler::add_alignment over a whole read list (read_pooler.cpp:3-20):
 * pool_index[i] = pool of read i (pools numbered by first occurrence);
 * returns the number of pools or <0. */
int32_t ltr_pool_reads(const uint8_t* const* seqs, const int32_t* seq_lens, int32_t n_reads,
                       int32_t* pool_index);
/* SeqStutterGenotyper::calc_hap_aln_probs scatter (seq_stutter_genotyper.cpp:526-559):
 * pool rows -> read rows (masked), then mate-pair row sums. */
int ltr_scatter_pool_probs(const double* log_pool_aln_probs, const int32_t* pool_seed_positions,
                           const int32_t* pool_index, int32_t n_reads, int32_t n_alleles,
                           const uint8_t* realign_to_hap, const uint8_t* copy_read,
                           const uint8_t* second_mate,
                           double* log_aln_probs, int32_t* seed_positions);

/*
 * SeqStutterGenotyper::calc_hap_aln_probs (seq_stutter_genotyper.cpp:514-563) for MANY loci in one
 * GPU pass -- the throughput form of the drop-in.  Per locus: the R reads as the genotyper holds
 * them (alns_, after left_align_reads) and the haplotype blocks.  The library pools the reads
 * (ReadPooler), trims each pool (HapAligner::trim_alignment), scores every pool x haplotype pair of
 * every locus together, and fans the rows back out to reads (+ mate-pair sums).
 * log_aln_probs[l]: R_l x H_l doubles, seed_positions[l]: R_l ints (caller-owned, like
 * log_aln_probs_ / seed_positions_ of genotyper.h:37, seq_stutter_genotyper.h).
 */
typedef struct ltr_locus {
  const ltr_haplotype_blocks* hap;
  const ltr_alignment*        alns;
  int32_t                     n_alns;
  const uint8_t*              second_mate;   /* optional [n_alns], second_mate_ (seq_stutter_genotyper.cpp:491-497) */
  /* The three masks of calc_hap_aln_probs(realign_to_haplotype, realign_pool, copy_read) -- the form
   * add_and_remove_alleles calls after new candidate haplotypes were added (seq_stutter_genotyper.cpp:390-391):
   * only flagged haplotype columns / pools are scored and only flagged reads' rows are rewritten; mate rows
   * are summed over the flagged columns only (:546-559).  Each optional, NULL = all set (the call at :634). */
  const uint8_t*              realign_to_hap; /* [H]      */
  const uint8_t*              realign_pool;   /* [P] pools in order of first occurrence (ReadPooler) */
  const uint8_t*              copy_read;      /* [n_alns] */
} ltr_locus;
int ltr_calc_hap_aln_probs(ltr_ctx* ctx, const ltr_locus* loci, int64_t n_loci,
                           double* const* log_aln_probs, int32_t* const* seed_positions);

/* ---- consumer: genotype posteriors ---------------------------------------- */
/*
 * Genotyper::calc_log_sample_posteriors + get_optimal_haplotypes
 * (genotyper.cpp:21-100) on the GPU.  log_aln_probs [R x H] is clamped to
 * >= -600 IN PLACE like genotyper.cpp:57-58.  log_sample_posteriors [S x H x H],
 * sample_total_ll [S], gts [S x 2] (argmax, first maximum in row-major order).
 * Returns total LL through *total_ll.
 */
int ltr_posteriors(ltr_ctx* ctx, int32_t n_samples, int32_t n_reads, int32_t n_alleles,
                   double* log_aln_probs, const double* log_p1, const double* log_p2,
                   const int32_t* sample_label, int32_t haploid,
                   double* log_sample_posteriors, double* sample_total_ll,
                   int32_t* gts, double* total_ll);

/*
 * The same consumer for EVERY locus of a resident plan, reading the log-likelihood buffer of
 * the last ltr_plan_execute in place on the device (what SeqStutterGenotyper::genotype does per
 * locus: calc_hap_aln_probs -> calc_log_sample_posteriors, seq_stutter_genotyper.cpp:632-634).
 * Reads map to pool rows through pool_index (the scatter of seq_stutter_genotyper.cpp:526-538
 * without materialising the per-read matrix).  Outputs, loci then samples in order:
 * log_sample_posteriors [sum_l S_l*H_l*H_l], sample_total_ll [sum_l S_l], gts [2*sum_l S_l].
 */
typedef struct ltr_posterior_batch {
  int64_t        n_loci;          /* must equal the plan's */
  const int64_t* locus_read_off;  /* [n_loci+1] first READ (not pool) of each locus            */
  int64_t        n_reads;
  const int32_t* pool_index;      /* [n_reads] pool row of the read inside its locus          */
  const double*  log_p1;          /* [n_reads] phasing log-likelihoods (snp_bam_processor.h:17-18) */
  const double*  log_p2;
  const int32_t* sample_label;    /* [n_reads] sample index inside the locus                  */
  const int32_t* n_samples;       /* [n_loci]                                                 */
  int32_t        haploid;
} ltr_posterior_batch;
int ltr_plan_posteriors(ltr_plan* plan, const ltr_posterior_batch* pb,
                        double* log_sample_posteriors, double* sample_total_ll, int32_t* gts);
/*
 * Per-locus ploidy.  The reference decides ploidy per CHROMOSOME: genotyper_bam_processor.cpp:248 sets `haploid` for a locus whose
 * chromosome is in --haploid-chrs and hands it to the locus's SeqStutterGenotyper (:294), from where it reaches the priors
 * (genotyper.cpp:21-33), extract_genotypes_and_likelihoods (:132-256) and the FORMAT layout of write_vcf_record.  A resident
 * plan, a shard or an LL batch cuts across chromosomes, so every batched consumer has a *_ploidy form that takes
 *   locus_haploid  [n_loci], != 0 = the locus is on a haploid chromosome; NULL = pb->haploid for every locus.
 *                  When given, pb->haploid is not read.
 * Loci are independent: locus l of a mixed call carries the bits of the uniform call with haploid = (locus_haploid[l] != 0).
 * ltr_plan_posteriors is this call with locus_haploid = NULL.
 */
int ltr_plan_posteriors_ploidy(ltr_plan* plan, const ltr_posterior_batch* pb, const uint8_t* locus_haploid,
                               double* log_sample_posteriors, double* sample_total_ll, int32_t* gts);

/* ---- consumer, next step: genotype fields ------------------------------------ */
/*
 * Genotyper::extract_genotypes_and_likelihoods (genotyper.cpp:132-256) with calc_PLs (:102-107)
 * and calc_gl_diff (:109-130): from the normalised posterior matrix (ltr_posteriors /
 * ltr_plan_posteriors) to the per-sample values the VCF writer prints
 * (seq_stutter_genotyper.cpp:1255-1300: GT, Q = exp(log_unphased), PQ = exp(log_phased), GLDIFF,
 * GL, PL, PHASEDGL).  Host code: libm exp/log and the FP32 fastlog/fastexp of fast_log_sum_exp
 * (mathops.cpp:87-96), evaluated in the reference's order.
 *   n_alleles      number of haplotypes H (Genotyper::num_alleles_)
 *   n_variants     number of alleles V of the variant being reported
 *   hap_to_allele  [H] haplotype -> allele of that variant
 *   best_haplotypes[S x 2] get_optimal_haplotypes (the `gts` output of ltr_posteriors)
 * Every output pointer is optional (NULL = not wanted); gl_diffs, gls, pls and phased_gls are the
 * calc_gls / calc_pls / calc_phased_gls branches (:204-255).
 *   gls, pls    [S x n_gl], n_gl = haploid ? V : V(V+1)/2, order (i1, i2 <= i1) as VCF GL
 *   phased_gls  [S x (haploid ? V : V*V)]
 */
typedef struct ltr_genotype_fields {
  int32_t* best_gts;                      /* [S x 2] */
  double*  log_phased_posteriors;         /* [S] */
  double*  log_unphased_posteriors;       /* [S] */
  double*  hap_log_phased_posteriors;     /* [S] */
  double*  hap_log_unphased_posteriors;   /* [S] */
  double*  gls;
  double*  gl_diffs;                      /* [S] */
  int32_t* pls;
  double*  phased_gls;
} ltr_genotype_fields;
int ltr_extract_genotypes(int32_t n_samples, int32_t n_alleles, int32_t n_variants,
                          const int32_t* hap_to_allele, int32_t haploid,
                          const double* log_sample_posteriors, const double* sample_total_ll,
                          const int32_t* best_haplotypes, const ltr_genotype_fields* out);

/* ---- upstream of the path: raw reads -> prepared reads -> candidate haplotypes (host) ---- */
/* A BAM record as the locus driver hands it over (BamAlignment, bam_io.h): only what the path reads. */
typedef struct ltr_raw_alignment {
  int32_t        pos;             /* Position(), 0-based */
  int32_t        end_pos;         /* GetEndPosition(): first reference base after the alignment */
  const uint8_t* bases;           /* QueryBases() */
  const uint8_t* quals;           /* Qualities(), Phred+33; may be NULL */
  int32_t        length;
  int32_t        n_cigar;
  const char*    cigar_type;      /* CigarData(): M = X I D S H */
  const int32_t* cigar_num;
  int32_t        sample;          /* index of the read's sample (read group) */
  int32_t        haplotype_tag;   /* HP tag: 1 / 2, 0 = none (genotyper_bam_processor.cpp:145-150) */
  uint8_t        reverse;         /* IsReverseStrand() */
  uint8_t        use_for_hap_generation;   /* the read's "PF" flag for this region (bam_processor.cpp:28-35) */
} ltr_raw_alignment;
typedef struct ltr_read_set ltr_read_set;       /* the locus' prepared reads (left_alns), owned by the library */
/*
 * GenotyperBamProcessor::left_align_reads (genotyper_bam_processor.cpp:38-168) for one locus: reads that do not
 * span the region are dropped (:56), the rest are cut to region -+ 200 bp (BamAlignment::TrimAlignment,
 * bam_io.cpp:267-372), reads with the repeat deleted become "deleted" placeholders (:62-71), M/=/X runs are
 * re-derived against the reference (:80-135), soft-clipped reads are dropped (:137-140), HP tags are counted.
 * chrom_seq is a window of the chromosome that starts at coordinate chrom_seq_start.
 */
int ltr_left_align_reads(const ltr_raw_alignment* raw, int32_t n_raw, int32_t n_samples, int32_t region_start, int32_t region_stop,
                         const uint8_t* chrom_seq, int64_t chrom_seq_start, int64_t chrom_seq_len, ltr_read_set** out);
/*
 * SNPBamProcessor::process_phased_reads (snp_bam_processor.cpp:141-226, --phased-bam) for unpaired reads: the phasing priors
 * log_p1 / log_p2 that Genotyper::calc_log_sample_posteriors weighs a read's two haplotypes with, from the reads' HP tags.
 * haplotype[r] = 1 / 2 (the tag) or -1 (no tag, get_haplotype :126-134); read groups are visited in order 0 .. n_samples-1
 * with the reference's running totals: once a group has more than 20 % untagged reads or at most one read of either
 * haplotype (counted over the groups so far), no read of that and any later group is phased.  phased_reads may be NULL.
 */
int ltr_phasing_priors(int32_t n_reads, const int32_t* sample_of_read, const int32_t* haplotype, int32_t n_samples,
                       double* log_p1, double* log_p2, int32_t* phased_reads);
int32_t              ltr_read_set_size(const ltr_read_set* rs);
const ltr_alignment* ltr_read_set_alignments(const ltr_read_set* rs);          /* what ltr_calc_hap_aln_probs takes */
const char* const*   ltr_read_set_alignment_strings(const ltr_read_set* rs);   /* Alignment::get_alignment(): bases, '-' for deleted reference bases */
const uint8_t*       ltr_read_set_deleted(const ltr_read_set* rs);             /* Alignment::get_deleted() */
const int32_t*       ltr_read_set_source(const ltr_read_set* rs);              /* index of the raw read */
const int32_t*       ltr_read_set_sample(const ltr_read_set* rs);
const int32_t*       ltr_read_set_n_p1s(const ltr_read_set* rs);               /* [n_samples] reads tagged HP:1 / HP:2 */
const int32_t*       ltr_read_set_n_p2s(const ltr_read_set* rs);
int32_t              ltr_read_set_fail_count(const ltr_read_set* rs);          /* align_fail_count */
void                 ltr_read_set_free(ltr_read_set* rs);
/* HaplotypeGenerator::extract_sequence (HaplotypeGenerator.cpp:84-165) for read i: the read's bases between two
 * reference coordinates.  Returns their number (>= 0; out may be NULL), -1 if the read does not span, < -1 on error. */
int64_t ltr_extract_sequence(const ltr_read_set* rs, int32_t i, int32_t region_start, int32_t region_end, uint8_t* out, int64_t cap);
/*
 * SeqStutterGenotyper::build_haplotype (seq_stutter_genotyper.cpp:416-482) for one region with alleles taken from
 * the reads: HaplotypeGenerator::add_haplotype_block (:530-578: region padded by indel_flank_len, candidate
 * alleles by the exact-sequence rules of gen_candidate_seqs :295-373, sorted and trimmed :474-480, :14-82) and
 * fuse_haplotype_blocks (:580-607) -> [flank <= 35 bp][repeat block][flank <= 35 bp].  The partial-order-alignment
 * clustering of reads without a candidate (:376-472, spoa) is NOT performed here (ltr_build_haplotypes_clustered below
 * does it with medoids for the consensus, ltr_build_haplotypes_consensus with a partial-order-alignment consensus); the result says how many reads / samples the reference would have clustered.  ctx may be NULL (it only receives the hap-build time).
 * A failed construction (the reference's failure_msg_) is not an error status: blocks() is NULL, failure() the text.
 */
typedef struct ltr_hap_result ltr_hap_result;
int ltr_build_haplotype(ltr_ctx* ctx, const ltr_read_set* rs, int32_t n_samples, int32_t region_start, int32_t region_stop, int32_t period,
                        const uint8_t* chrom_seq, int64_t chrom_seq_start, int64_t chrom_seq_len, int64_t chrom_len,
                        int32_t indel_flank_len, ltr_hap_result** out);
/*
 * The same with the alleles of a --ref-vcf panel (ltr_vcf_read_alleles): HaplotypeGenerator::add_vcf_haplotype_block
 * (HaplotypeGenerator.cpp:497-525) and fuse_haplotype_blocks (:580-607).  The repeat block is [pos, pos+len(REF)) with the
 * panel's alleles uppercased in panel order (no indel-flank padding, sorting or trimming); the flanks are those of
 * ltr_build_haplotype, bounded by all reads of rs.  Failures are texts, as there: the reference's "Haplotype blocks are too
 * near to the chromosome ends", and -- where the reference asserts or would misbehave -- a REF that differs from the
 * reference bases and a symbolic allele (<...>, '*').  The one exception is an ALT "<DEL>": ltr_vcf_record writes it for a
 * block allele with no bases, and it is read back as that empty allele.  unplaced_reads / samples_needing_clustering are 0.
 */
int ltr_build_vcf_haplotype(ltr_ctx* ctx, const ltr_read_set* rs, int32_t pos, const char* alleles, const int64_t* allele_off,
                            int32_t n_alleles, int32_t period, const uint8_t* chrom_seq, int64_t chrom_seq_start,
                            int64_t chrom_seq_len, int64_t chrom_len, ltr_hap_result** out);
const ltr_haplotype_blocks* ltr_hap_result_blocks(const ltr_hap_result* r);
const char* ltr_hap_result_failure(const ltr_hap_result* r);
int32_t     ltr_hap_result_unplaced_reads(const ltr_hap_result* r);
int32_t     ltr_hap_result_samples_needing_clustering(const ltr_hap_result* r);
void        ltr_hap_result_free(ltr_hap_result* r);

/* ---- reads without an exact allele: clustered into inexact candidate alleles (GPU distances, host clustering) -------- */
/*
 * The distance of HaplotypeGenerator::needleman_wunsch (HaplotypeGenerator.cpp:201-234: unit costs, bytes compared for
 * equality as at :223 -- 'N' equals 'N', nothing is case-folded) for ALL pairs of every group of sequences, capped:
 *   dist + dist_off[g]   U_g x U_g int32, row-major, symmetric, zero diagonal; entry = min(levenshtein(a, b), cap)
 * with 1 <= cap <= 32767.  Empty sequences are legal (d("", x) = len(x)).  Only i < j is computed and the result mirrored; a pair
 * with |n - m| >= cap (and a pair with an empty side) is written by the host and never launched; a group of at most one
 * sequence launches nothing.  A sequence belongs to at most one group, and the bytes of a group are remapped to at most 32
 * codes: a group with more distinct bytes is LTR_ERR_INVALID.  Every error is LTR_ERR_INVALID + ltr_last_error naming the
 * group; then nothing is launched and dist is untouched.  The kernel is the bit-vector block algorithm (Myers 1999 / Hyyro),
 * ltr_editdist.hip; the cap is applied to the result only.  No CPU fallback: without a context LTR_ERR_NO_DEVICE.
 */
typedef struct ltr_seq_groups {
  int64_t        n_groups;
  const int64_t* group_seq_off;   /* [n_groups+1] first sequence of each group */
  int64_t        n_seqs;
  const uint8_t* seq_bytes;       /* concatenated */
  const int64_t* seq_off;         /* [n_seqs+1] */
} ltr_seq_groups;
int ltr_edit_distances(ltr_ctx* ctx, const ltr_seq_groups* sg, int32_t cap, int32_t* dist, const int64_t* dist_off);
/*
 * The clustering of gen_candidate_seqs (:399-470) for ONE sample, as a function of its U unique unplaced sequences (any order,
 * no duplicates), how many reads carry each, their distance matrix capped at 701 (ltr_edit_distances; host code, no GPU) and
 * the candidate alleles present so far:
 *   order        the lexicographically first sequence first (the first std::map key, :400-402), the rest by
 *                orderByLengthAndSequence (:403)
 *   ladder       T in {20,50,80,100,150,200,300,400,500,600,700} (:405); the first T that passes the coverage rule ends it
 *   greedy_clustering (:237-268)  sequence against the centroids in creation order, the smallest score < T (first on ties),
 *                a 16th centroid fails the threshold
 *   score < T    decided from the matrix: needleman_wunsch(a, b, score, T) has score < T <=> d(a, b) < T for T <= 700.  ONE
 *                EXCEPTION, reproduced by argument position in the greedy step and in merge_clusters: with an empty second
 *                argument (the centroid) and a non-empty first, the reference's inner loop never runs and it answers T + 1
 *   refinement (:418-440)  DEVIATION: where the reference takes the partial-order-alignment consensus (poa, :427) the cluster's
 *                MEDOID stands in -- the member x minimising sum_y count[y] * dist[x][y] over the members, ties to the earlier in
 *                length-then-sequence order; clusters in std::map order of their centroid, new centroids sorted from the
 *                second on (:437), merge_clusters (:271-293) with j from 1, (centroid i, centroid j) argument order; until
 *                no merge happens
 *   acceptance (:446-469)  a cluster counts when its reads are > min((int)(0.10 * ignored), 10); T passes when the counted
 *                reads are >= (int)(0.80 * ignored); the counted centroids that are no candidate yet are the new alleles
 * Result: threshold (accepted T or -1: then no clusters), the clusters in std::map order of their centroid -- centroids and
 * members as indices into the caller's sequences --, counted[c], new_allele[c].  Free with ltr_cluster_result_free.
 */
typedef struct ltr_cluster_result ltr_cluster_result;
int ltr_cluster_sequences(const uint8_t* seq_bytes, const int64_t* seq_off, const int32_t* counts, int32_t n_seqs, const int32_t* dist,
                          const uint8_t* cand_bytes, const int64_t* cand_off, int32_t n_cands, ltr_cluster_result** out);
int32_t        ltr_cluster_result_threshold(const ltr_cluster_result* r);
int32_t        ltr_cluster_result_n_clusters(const ltr_cluster_result* r);
const int32_t* ltr_cluster_result_centroids(const ltr_cluster_result* r);       /* [n_clusters] */
const uint8_t* ltr_cluster_result_new_allele(const ltr_cluster_result* r);      /* [n_clusters] */
const uint8_t* ltr_cluster_result_counted(const ltr_cluster_result* r);         /* [n_clusters] */
const int32_t* ltr_cluster_result_members(const ltr_cluster_result* r, int32_t cluster, int32_t* n);
void           ltr_cluster_result_free(ltr_cluster_result* r);
/*
 * ltr_build_haplotype for many loci WITH the clustering step (:376-472), in three phases: A (worker pool) everything
 * ltr_build_haplotype does up to :372, and per sample with ignored > 0.25 * reads (:392) its unique unplaced sequences; B ONE
 * ltr_edit_distances launch set over all those groups, cap 701; C (worker pool) per locus the samples in order (:398), each
 * through ltr_cluster_sequences against the candidates so far (:457-458), then the sort (:475, the inexact flag travels with
 * its sequence), trim and fuse as in ltr_build_haplotype.  The cluster centres are medoids (see above), flagged inexact
 * (INEXACT_ALLELE=1).  A failed construction stays a text in the result; an error status leaves every out[l] NULL.
 * unplaced_reads / samples_needing_clustering keep their meaning (what was found before clustering).  A locus where no sample
 * needs clustering comes out byte-identical to ltr_build_haplotype.
 *   ltr_hap_result_inexact            [alleles of the repeat block] 1 = a cluster centre (NULL for a failed construction)
 *   ltr_hap_result_cluster_threshold  the sample's accepted T, -1 none passed, 0 clustering not needed
 */
typedef struct ltr_hap_build_locus {
  const ltr_read_set* rs; int32_t n_samples, region_start, region_stop, period;
  const uint8_t* chrom_seq; int64_t chrom_seq_start, chrom_seq_len, chrom_len;
} ltr_hap_build_locus;
int ltr_build_haplotypes_clustered(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len,
                                   ltr_hap_result** out /* [n_loci] */);
const uint8_t* ltr_hap_result_inexact(const ltr_hap_result* r);
int32_t        ltr_hap_result_cluster_threshold(const ltr_hap_result* r, int32_t sample);

/* ---- the consensus of a cluster: partial-order alignment on the GPU -------- */
/*
 * HaplotypeGenerator::poa (HaplotypeGenerator.cpp:167-199, called at :427) for every group of sequences: the consensus of the
 * group's members.  This is partial-order alignment by the PUBLISHED method (Lee, Grasso & Sharlow 2002; heaviest-bundle
 * consensus) with the scoring :169 hands to spoa (global, linear gap, match +1, mismatch -1, gap -1) and every tie rule fixed
 * (restated as code in tests/poa_util.py); it is NOT spoa's bytes, and parity with spoa is not claimed.
 *   members     in the group's order, each weighing 1 (:174-176); bytes compared for equality; empty members are dropped; none
 *               left: the consensus is empty; one left: it is that member, nothing is launched; of more than 30 (:171) the members
 *               at floor(k * n / 30), k = 0 .. 29, are taken in that order (the reference draws 30 at random, :182-192)
 *   result      group g's consensus is out_bytes[out_off[g] .. out_off[g+1]); status[g] = 0, or 1: the group is over the memory
 *               cap below, it was not aligned and its consensus is empty
 * A sequence may lie in several groups; there is no limit on the distinct bytes of a group.  out_cap must be at least
 * ltr_poa_consensus_capacity(sg) (the bytes of all groups; < 0 for a malformed sg).  Errors as ltr_edit_distances: LTR_ERR_INVALID +
 * ltr_last_error naming the group, then nothing is launched and the outputs are untouched.  No CPU fallback: without a context
 * LTR_ERR_NO_DEVICE, whatever the other arguments are, and nothing is launched.
 * Memory rule (ltr_poa.hip: one wavefront per group, all groups of a call in as few launch sets as the budget allows).  A group
 * of B bases in all and a longest member of L keeps 50 bytes a base of graph arrays (in LDS up to 16 KB, else in its scratch)
 * and, for the traceback, the score rows of ONE alignment: (nodes + 1) x (L + 1) cells of 2 bytes while B + L <= 32767 and 4
 * beyond.  Nodes are known only as the graph grows (at most B; in practice two or three per column).
 *   per-group cap    512 MB: 30 x 5000-base reads (BASELINE config 5) at some 12 000 nodes are 12 001 x 5 401 x 4 = 259 MB; the cap
 *                    is reached at 24 000 nodes for such reads, or by 8 x 16 000-base members.  The wavefront tests it before
 *                    every alignment; a group over it reports status 1.
 *   per-call budget  16 GB a launch set (a group's block is min(cap, what B and L allow at most)); further groups go to further sets.
 * ltr_ctx_set_debug "poa_group_cap_bytes" / "poa_call_budget_bytes" lower both (0: the rule); the cap is the one switch that
 * changes a result (which groups report status 1), the budget never does.
 */
int     ltr_poa_consensus(ltr_ctx* ctx, const ltr_seq_groups* sg, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off /* [n_groups+1] */,
                          uint8_t* status /* [n_groups]: 0 consensus, 1 over the cap: empty */);
int64_t ltr_poa_consensus_capacity(const ltr_seq_groups* sg);
/*
 * ltr_build_haplotypes_clustered with the consensus where the reference calls poa (HaplotypeGenerator.cpp:427): the centre of a
 * cluster is ltr_poa_consensus of its members in the cluster's order, not its medoid.  A consensus is none of the input
 * sequences, so the refinement loop (:418-440) needs distances the first matrix does not hold, and runs as rounds over all
 * (locus, sample) groups of the call at once:
 *   1  phases A and B as in ltr_build_haplotypes_clustered; the capped matrix serves greedy_clustering at every threshold
 *   2  host, per group that starts a threshold: the ladder step (:405) and greedy_clustering (:237-268; a 16th centroid: next T)
 *   3  ONE ltr_poa_consensus call over every cluster of every group in refinement whose ordered member list has not been aligned
 *      before in this call (the reference aligns unchanged clusters again; the method is deterministic, the answer is the same)
 *   4  ONE ltr_edit_distances call, cap 701, over each group's new centres: equal ones folded into one cluster (:428-434), sorted
 *      from the second on (:437)
 *   5  host: merge_clusters (:271-293; j from 1, (centre i, centre j) argument order, the empty-second-argument exception); a
 *      group that merged goes back to 3, the others to the acceptance (:446-469), and to the next threshold at 2 if they fail it
 * The is-it-a-candidate-already test (:457-458) is made on the consensus string against the exact and inexact candidates so far,
 * the samples of a locus in order.  New alleles are the consensus strings, flagged inexact; sort, trim and fuse are unchanged.  A
 * cluster over the memory cap of ltr_poa_consensus keeps its medoid and is counted.  A locus where no sample needs clustering
 * comes out byte-identical to ltr_build_haplotype.  Results, errors and ownership as ltr_build_haplotypes_clustered, and
 *   ltr_hap_result_consensus_rounds   refinement rounds (:422) the sample took, over all thresholds it tried (0: not clustered)
 *   ltr_hap_result_medoid_kept        how many of the sample's final clusters kept the medoid because of the cap
 */
int     ltr_build_haplotypes_consensus(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len,
                                       ltr_hap_result** out /* [n_loci] */);
int32_t ltr_hap_result_consensus_rounds(const ltr_hap_result* r, int32_t sample);
int32_t ltr_hap_result_medoid_kept(const ltr_hap_result* r, int32_t sample);

/* ---- neighbour of the path: haplotype -> reference-haplotype alignment (GPU) -------- */
/*
 * Haplotype::aln_haps_to_ref (src/SeqAlignment/Haplotype.cpp:58-86) for every haplotype of every locus in one
 * launch: NeedlemanWunsch::Align(reference haplotype, haplotype, use_ref_end_penalty = true)
 * (NeedlemanWunsch.cpp:380-420), Haplotype::adjust_indels (Haplotype.cpp:8-56) and the M / I / D strings
 * hap_aln_info_ holds.  Haplotypes need three blocks (adjust_indels asserts it).  aln_info receives the
 * strings back to back; haplotype k of locus l (Haplotype::next() order, the reference haplotype first) is
 * [info_off[h], info_off[h+1]) with h = (haplotypes of the loci before l) + k; info_off has sum_l H_l + 1
 * entries; cap >= ltr_haplotype_aln_info_capacity().  In the reference only the traced short path reads
 * these strings (HapAligner.cpp:969); the long-read path does not need this call at all.
 */
int64_t ltr_haplotype_aln_info_capacity(const ltr_haplotype_blocks* const* haps, int64_t n_loci);
int ltr_haplotype_align_to_ref(ltr_ctx* ctx, const ltr_haplotype_blocks* const* haps, int64_t n_loci,
                               char* aln_info, int64_t cap, int64_t* info_off);

/* ---- consumer, last steps: allele pruning and the VCF record (host) -------------- */
/* SeqStutterGenotyper::haps_to_alleles (seq_stutter_genotyper.cpp:240-248): allele of `block` in every haplotype. */
int ltr_haps_to_alleles(const ltr_haplotype_blocks* hap, int32_t block, int32_t* hap_to_allele);
/*
 * SeqStutterGenotyper::get_unused_alleles(check_spanned = false, check_called = true) (:250-308) for one block:
 * non-reference alleles that no called sample with an aligned read carries in its optimal haplotype pair
 * (best_haplotypes [S x 2] = the gts of ltr_posteriors; sample_filtered[s] != 0 <=> call_sample_[s] not empty).
 * Writes the allele indices to `unused` and returns their number (genotype() then calls remove_alleles, :636-645).
 */
int32_t ltr_unused_alleles(int32_t n_samples, const int32_t* best_haplotypes, const uint8_t* sample_has_aligned_read,
                           const uint8_t* sample_filtered, int32_t n_haplotypes, const int32_t* hap_to_allele,
                           int32_t n_block_alleles, int32_t* unused);
/*
 * The bookkeeping of add_and_remove_alleles (:317-409) around the re-alignment.  The caller rebuilds its block
 * list (HapBlock::remove_alleles / add_alternate); haplotypes of the old and the new list are matched by
 * sequence: allele_mapping[old haplotype] = new index or -1, realign_to_hap[new haplotype] = 1 for sequences that
 * did not exist before (the mask of the three-argument calc_hap_aln_probs, ltr_locus.realign_to_hap);
 * ltr_remap_aln_probs moves the surviving columns of log_aln_probs_ (everything else -100000, :367).
 */
int ltr_remap_haplotypes(const ltr_haplotype_blocks* old_hap, const ltr_haplotype_blocks* new_hap,
                         int32_t* allele_mapping, uint8_t* realign_to_hap);
int ltr_remap_aln_probs(const double* old_ll, int32_t n_reads, int32_t h_old, const int32_t* allele_mapping, int32_t h_new, double* new_ll);
/* HapBlock::remove_alleles (HapBlock.h:151-160, RepeatBlock.h:60-69) for `block` of a block list, the other blocks copied:
 * the rebuilt list remove_alleles (:411-414, :332-335) makes from the indices ltr_unused_alleles returned.  Allele 0 is never
 * removed (the assert of HapBlock.h:153): LTR_ERR_INVALID, as for an index outside the block.  Free with ltr_hap_result_free. */
int ltr_prune_hap_blocks(const ltr_haplotype_blocks* old_hap, int32_t block, const int32_t* unused, int32_t n_unused, ltr_hap_result** out);

/* ---- consumer, whole chain: posteriors -> prune uncalled alleles -> posteriors again, every locus of a plan (GPU) ---- */
/*
 * SeqStutterGenotyper::genotype after the alignment (seq_stutter_genotyper.cpp:632-645) for EVERY locus of an executed plan:
 *   1. calc_log_sample_posteriors + get_optimal_haplotypes (:635, genotyper.cpp:21-100), as ltr_plan_posteriors, bit for bit;
 *   2. prune != 0 (discovery mode, :636-645): get_unused_alleles(false, true) (:250-308) per locus -- aligned_read[s] from the
 *      plan's seed positions through pool_index (:262-266); blocks with one option skipped (:274); allele 0 never removed
 *      (:298); sample_filtered[s] != 0 <=> call_sample_[s] not empty (:289);
 *   3. remove_alleles -> add_and_remove_alleles (:317-409) for the loci where something is unused (:641): the new block list
 *      (HapBlock::remove_alleles), its haplotypes in Haplotype::next() order of the NEW list, matched to the old ones by
 *      sequence like ltr_remap_haplotypes (:322-360), the surviving columns of log_aln_probs_ (:364-377; a new haplotype
 *      without an old one reads -100000, :367);
 *   4. calc_log_sample_posteriors over the smaller set (:405-408): priors of the new H (genotyper.cpp:21-33), bit-identical
 *      to ltr_posteriors on the re-mapped matrix.
 * Pruning happens ONCE, not to a fixed point (:640-645); a locus with nothing unused keeps its first posteriors (:641);
 * prune == 0 is the --ref-vcf mode (:636): the first posteriors are final.  The posterior arithmetic and the column gather
 * run on the device (ltr_plan_genotype.hip); the host sees the first pass's best pairs only.
 * The plan must have been executed.  An error (LTR_ERR_INVALID + ltr_last_error) launches nothing and leaves *out NULL.
 */
typedef struct ltr_genotype_batch {
  const ltr_posterior_batch*         pb;      /* reads -> pool rows, priors, sample labels, S_l, haploid: as ltr_plan_posteriors */
  const ltr_haplotype_blocks* const* haps;    /* [n_loci] block list of each locus; its number of combinations must equal the plan's H_l.
                                                 prune == 0: not read at all (may be NULL; ltr_genotype_result_blocks hands back what was given) */
  const uint8_t*                     sample_filtered;   /* optional [sum_l S_l], loci then samples in order */
  int32_t                            prune;   /* 1 = discovery mode (:636-645); 0 = first posteriors are final */
  int32_t                            want_read_ll;      /* != 0: also gather the per-read matrices (ltr_genotype_result_read_ll) */
} ltr_genotype_batch;
typedef struct ltr_genotype_result ltr_genotype_result;      /* owned by the library */
int  ltr_plan_genotype(ltr_plan* plan, const ltr_genotype_batch* gb, ltr_genotype_result** out);
void ltr_genotype_result_free(ltr_genotype_result* r);
/* Per locus l (NULL / a negative status for a bad index); pointers stay valid until ltr_genotype_result_free.  H = the plan's
 * number of haplotypes of the locus, H' = after pruning, S = its samples, R = its reads.
 *   n_haps          H'
 *   new_to_old      [H'] column of the plan's LL matrix each final haplotype reads (-1: none, see 3.)
 *   allele_mapping  [H]  old haplotype -> new index or -1, the array of :349-359
 *   removed         indices of the removed alleles of `block` through *alleles (NULL when none); returns their number
 *   num_aff_blocks, num_aff_alleles   the counters of get_unused_alleles (:253-306)
 *   blocks          the block list the final haplotypes enumerate: the pruned copy, or -- for a locus that lost no allele --
 *                   the caller's own gb->haps[l] (not copied: valid as long as the caller keeps it; the ONLY accessor that
 *                   hands out or reads caller memory after the call has returned); ready for ltr_vcf_record
 *   log_sample_posteriors [S x H' x H'], sample_total_ll [S], gts [S x 2] in the NEW indices
 *   read_ll         [R x H'] log_aln_probs_ per READ (not per pool), clamped at -600 as genotyper.cpp:57-58 leaves it: what
 *                   ltr_vcf_locus.log_aln_probs wants (NULL unless want_read_ll) */
/* the ploidy locus l was genotyped with, whichever entry point made the result: 0 / 1, negative for a bad index */
int32_t        ltr_genotype_result_haploid(const ltr_genotype_result* r, int64_t l);
int64_t        ltr_genotype_result_n_loci(const ltr_genotype_result* r);
int32_t        ltr_genotype_result_n_haps(const ltr_genotype_result* r, int64_t l);
const int32_t* ltr_genotype_result_new_to_old(const ltr_genotype_result* r, int64_t l);
const int32_t* ltr_genotype_result_allele_mapping(const ltr_genotype_result* r, int64_t l);
int32_t        ltr_genotype_result_removed(const ltr_genotype_result* r, int64_t l, int32_t block, const int32_t** alleles);
int32_t        ltr_genotype_result_num_aff_blocks(const ltr_genotype_result* r, int64_t l);
int32_t        ltr_genotype_result_num_aff_alleles(const ltr_genotype_result* r, int64_t l);
const ltr_haplotype_blocks* ltr_genotype_result_blocks(const ltr_genotype_result* r, int64_t l);
const double*  ltr_genotype_result_log_sample_posteriors(const ltr_genotype_result* r, int64_t l);
const double*  ltr_genotype_result_sample_total_ll(const ltr_genotype_result* r, int64_t l);
const int32_t* ltr_genotype_result_gts(const ltr_genotype_result* r, int64_t l);
const double*  ltr_genotype_result_read_ll(const ltr_genotype_result* r, int64_t l);

/*
 * The numbers SeqStutterGenotyper::write_vcf_record (:894-1366) derives from the posteriors and the per-read matrix before it
 * prints, for one repeat block of one locus: views, owned by whoever handed them out.  S samples, R reads, V alleles of the block.
 *   best_gts .. phased_gls   Genotyper::extract_genotypes_and_likelihoods (genotyper.cpp:132-256), as ltr_genotype_fields;
 *                            gl_diffs = calc_gl_diff (:109-130), pls = calc_PLs (:102-107); n_gl = haploid ? V : V(V+1)/2,
 *                            n_pgl = haploid ? V : V*V; gls / pls / phased_gls NULL unless asked for
 *   n_aligned, n_snp, n_s1, n_s2   reads of the sample, those with |log_p1 - log_p2| > 1e-10, and their sides (:1006-1012)
 *   read_allele              [R] allele of the block in the read's more likely strand haplotype (:965-967, :1038-1040)
 */
typedef struct ltr_locus_fields {
  int32_t S, R, V, block, n_gl, n_pgl;
  const int32_t* best_gts;          /* [S x 2] */
  const double  *log_phased, *log_unphased, *hap_log_phased, *hap_log_unphased, *gl_diffs;   /* [S] */
  const double  *gls; const int32_t* pls; const double* phased_gls;                          /* NULL unless asked */
  const int32_t *n_aligned, *n_snp, *n_s1, *n_s2;                                            /* [S] */
  const int32_t* read_allele;       /* [R] */
} ltr_locus_fields;

/* ltr_plan_genotype and, on the blocks where they lie on the device, the fields of every locus (ltr_plan_fields.hip):
 * the same passes and the same bits in every accessor above, then one kernel, one (locus, sample) per workgroup.
 * gb->haps is required (hap_to_allele of the FINAL block list, :240-248, is taken from it on the host).
 * The context of the plan must outlive the result.
 * A sample for which the passes found no optimal haplotype pair (gts = -1: NaN scores) has best_gts = -1 and 0 in every other
 * number of its own; ltr_genotype_result_vcf_records refuses such a locus (LTR_ERR_INVALID, the locus named). */
typedef struct ltr_fields_request {
  const int32_t* block;        /* [n_loci] block each record is for; NULL = the first is_repeat block of the final list */
  int32_t want_gls, want_pls, want_phased_gls;
  int32_t want_posteriors;     /* 0: the S x H' x H' blocks are NOT downloaded (ltr_genotype_result_log_sample_posteriors returns NULL) */
} ltr_fields_request;
int ltr_plan_genotype_fields(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result** out);
/* ltr_plan_genotype (fr == NULL) / ltr_plan_genotype_fields (fr given) with the ploidy of every locus (genotyper_bam_processor.cpp:248,
 * :294; see ltr_plan_posteriors_ploidy): the priors of both passes (genotyper.cpp:21-33, seq_stutter_genotyper.cpp:405-408), n_gl /
 * n_pgl, the GL / PHASEDGL terms and the strand rule of the fields (genotyper.cpp:132-256) follow the locus's own ploidy; the packed
 * gls / pls / phased_gls of a locus have its own widths.  Those two entry points are this call with locus_haploid = NULL; errors
 * are theirs, whether or not locus_haploid is given. */
int  ltr_plan_genotype_ploidy(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr /* NULL = as ltr_plan_genotype */,
                              const uint8_t* locus_haploid, ltr_genotype_result** out);
/* The same consumer WITHOUT a plan: ltr_plan_genotype (fr == NULL) or ltr_plan_genotype_fields (fr given) on per-read matrices in
 * caller memory -- what ltr_calc_hap_aln_probs returns, the state of SeqStutterGenotyper at seq_stutter_genotyper.cpp:634, also
 * after the seeded stutter path, with mate rows summed (:546-559) or re-scored under realign_* masks.  Every read is its own row:
 *   gb            as for ltr_plan_genotype[_fields], except that gb->pb->pool_index is not read (may be NULL); gb->haps[l] must
 *                 enumerate n_haps[l] combinations (checked whenever the block lists are read: prune != 0 or fr given)
 *   aligned_read  of get_unused_alleles (:262-266): seed_positions[l][read] >= 0
 * The matrices are never written (ltr_posteriors clamps its input in place; here the clamp at -600 happens on the device copy).
 * They are gathered into pinned staging by the worker pool under the host-thread budget and uploaded in chunks on the context's
 * stream, chunk k + 1 being gathered while chunk k is copied; the block stays on the device for the whole call.
 * The result is the same object: every accessor above and below works on it; new_to_old indexes the caller's columns, read_ll
 * (want_read_ll) is the caller's matrix clamped and re-mapped; the same bits as the plan path on the same scores.
 * Errors as ltr_plan_genotype: LTR_ERR_INVALID + ltr_last_error (the locus named), nothing launched, *out left NULL.
 * The context must outlive the result. */
typedef struct ltr_ll_batch {
  const double*  const* log_aln_probs;   /* [n_loci] R_l x H_l per READ, host memory, never written (NULL allowed for a locus without reads) */
  const int32_t* const* seed_positions;  /* [n_loci] R_l; NULL, or a NULL entry = every read aligned */
  const int32_t*        n_haps;          /* [n_loci] H_l */
} ltr_ll_batch;
int ltr_ll_genotype(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb,
                    const ltr_fields_request* fr /* NULL = as ltr_plan_genotype */, ltr_genotype_result** out);
/* ... with the ploidy of every locus (genotyper_bam_processor.cpp:248, :294), as ltr_plan_genotype_ploidy: locus_haploid [n_loci],
 * NULL = gb->pb->haploid for every locus (that is ltr_ll_genotype). */
int ltr_ll_genotype_ploidy(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr,
                           const uint8_t* locus_haploid, ltr_genotype_result** out);
/* views into the result (LTR_ERR_INVALID for a result of ltr_plan_genotype, which has none) */
int ltr_genotype_result_fields(const ltr_genotype_result* r, int64_t l, ltr_locus_fields* out);

/* Genotyper's output switches (genotyper.cpp:339-346; CLI --output-gls etc., hipstr_main.cpp:178-183). */
typedef struct ltr_vcf_options {
  int32_t output_gls, output_pls, output_phased_gls, output_allreads, output_mallreads, output_filters, output_haplotype_data;
  float   max_flank_indel_frac;
} ltr_vcf_options;
void ltr_default_vcf_options(ltr_vcf_options* o);

/* Everything SeqStutterGenotyper::write_vcf_record (:894-1366) reads for one repeat block of one locus. */
typedef struct ltr_vcf_locus {
  const char*    chrom;                 /* Region::chrom() */
  int32_t        region_start, region_stop;   /* Region::start() / stop() (0-based, half open) */
  const char*    name;                  /* Region::name(), NULL or "" -> "." */
  const char*    motif;                 /* Region::motif() */
  const char*    period_str;            /* Region::period_str() */
  const uint8_t* chrom_seq;             /* reference bases from coordinate chrom_seq_start on (a window is enough: */
  int64_t        chrom_seq_start;       /* get_alleles reads [min(region_start, block start) - 1, region_stop))    */
  int64_t        chrom_seq_len;
  const ltr_haplotype_blocks* hap;
  int32_t        block;                 /* hap_block_index: the repeat block the record is for */
  const uint8_t* inexact_allele;        /* optional [alleles of the block] HapBlock::get_inexact */
  int32_t        n_reads, n_samples, haploid;
  const double*  log_aln_probs;         /* [R x H] log_aln_probs_ (ltr_calc_hap_aln_probs) */
  const double*  log_p1; const double* log_p2;   /* [R] */
  const int32_t* sample_label;          /* [R] */
  const ltr_alignment* alns;            /* optional [R]: ALLREADS (ExtractCigar over region +- 5) */
  const uint8_t* aln_deleted;           /* optional [R] Alignment::get_deleted() */
  const double*  log_sample_posteriors; /* [S x H x H] (ltr_posteriors) */
  const double*  sample_total_ll;       /* [S] */
  const int32_t* best_haplotypes;       /* [S x 2] */
  const int32_t* n_p1s; const int32_t* n_p2s;    /* optional [S] reads per phased haplotype (PDP) */
  const char* const* sample_names;      /* [S] the genotyper's samples */
  const char* const* sample_filter;     /* optional [S] call_sample_: NULL / "" = called, else the filter reason */
  int32_t        n_out_samples;         /* VCF columns; 0 = the genotyper's samples in order */
  const char* const* out_sample_names;
} ltr_vcf_locus;
/* get_alleles (:688-785): number of alleles; text in `out`, allele i at [allele_off[i], allele_off[i+1]); *pos 1-based. */
int32_t ltr_get_alleles(const ltr_vcf_locus* v, int32_t* pos, char* out, int64_t cap, int64_t* allele_off);
/* write_vcf_record for the long-read path (no alignment traces: DFLANKINDEL = 0): the VCF line without the
 * trailing newline, NUL-terminated.  Returns its length or a negative status. */
int64_t ltr_vcf_record(const ltr_vcf_locus* v, const ltr_vcf_options* opt, char* out, int64_t cap, int32_t* pos);
/* The two halves of ltr_vcf_record, which is their composition.
 * ltr_vcf_fields: the arithmetic (:916-927 = extract_genotypes_and_likelihoods, :929-1043 the per-read bookkeeping) on the
 * host; want_* as the output switches (gls are always computed: GLDIFF needs them).  The set owns the arrays
 * ltr_vcf_field_set_view points into.
 * ltr_vcf_record_from_fields: the text (:894-913 alleles, :1045-1366 counts, INFO, FORMAT, one column per sample; ALLREADS
 * through ExtractCigar, extract_indels.cpp:18-91).  Of v it does not read log_aln_probs, log_p1, log_p2, log_sample_posteriors,
 * sample_total_ll, best_haplotypes (they may be NULL).  LTR_ERR_INVALID, nothing written, when f is NULL, its S / R / V are
 * not the locus', an allele index is not below V, or an array a switch of *opt needs is NULL. */
typedef struct ltr_vcf_field_set ltr_vcf_field_set;
int  ltr_vcf_fields(const ltr_vcf_locus* v, int32_t want_gls, int32_t want_pls, int32_t want_phased_gls, ltr_vcf_field_set** out);
const ltr_locus_fields* ltr_vcf_field_set_view(const ltr_vcf_field_set* f);
void ltr_vcf_field_set_free(ltr_vcf_field_set* f);
int64_t ltr_vcf_record_from_fields(const ltr_vcf_locus* v, const ltr_locus_fields* f, const ltr_vcf_options* opt, char* out, int64_t cap, int32_t* pos);
/* Every locus' record of a ltr_plan_genotype_fields result through ltr_vcf_record_from_fields, on the library's worker pool
 * under the host-thread budget (ltr_ctx_set_host_threads); the text does not depend on the number of threads.
 * loci [n_loci]: hap, block and haploid of each are ignored: ltr_genotype_result_blocks, the block the fields were made for and the
 * ploidy the locus was genotyped with (ltr_genotype_result_haploid) are used, so a haploid locus gets FORMAT
 * GT:GB:Q:DP:DFLANKINDEL:GLDIFF and V-wide GL / PL, a diploid one the ten-field form, V(V+1)/2-wide GL / PL and PHASEDGL.
 * *text: the records back to back in locus order, each followed by '\n', NUL-terminated, to be released with
 * ltr_vcf_text_free; record l is [rec_off[l], rec_off[l + 1] - 1) (rec_off [n_loci + 1]); pos [n_loci] optional.
 * On an error (LTR_ERR_INVALID, ltr_last_error names the locus) *text stays NULL and rec_off / pos are not written. */
int  ltr_genotype_result_vcf_records(const ltr_genotype_result* r, const ltr_vcf_locus* loci, const ltr_vcf_options* opt,
                                     char** text, int64_t* rec_off, int32_t* pos);
void ltr_vcf_text_free(char* text);
/* Genotyper::get_vcf_header (genotyper.cpp:258-336): ##fileformat, ##command, ##reference, the FASTA's ##contig lines
 * (contig_lines = the text ltr_fasta_contig_lines gives, or NULL), the ##INFO / ##FORMAT definitions of every field
 * ltr_vcf_record writes (the optional ones by *opt, NULL = defaults), the #CHROM line with the sample names.
 * NUL-terminated text; returns its length or a negative status. */
int64_t ltr_vcf_header(const char* fasta_path, const char* full_command, const char* contig_lines, const ltr_vcf_options* opt,
                       const char* const* sample_names, int32_t n_samples, char* out, int64_t cap);

/* ---- on-disk formats that need no htslib ------------------------ */
/*
 * Where the reference ends the process on a malformed input (printErrorAndDie, src/error.cpp:6-10) these entry
 * points return LTR_ERR_INVALID and copy the reference's message into err (NUL-terminated, at most err_cap bytes;
 * err may be NULL).  BAM / CRAM input stays with the host program.
 */
/* readRegions (src/region.cpp:26-65): whitespace-separated CHROM START STOP MOTIF [NAME], START 1-based (stored
 * 0-based), at most max_regions regions, optionally only those on chrom_limit (NULL / "" = all).  orderRegions
 * (:67-69) = ltr_region_set_order.  period = Region::computePeriod (region.h:32-39: the common motif length, -1 when
 * the comma-separated motifs differ in length), period_str = Region::period_str (:63-71). */
typedef struct ltr_region_set ltr_region_set;
int         ltr_read_regions(const char* path, uint32_t max_regions, const char* chrom_limit, ltr_region_set** out, char* err, int err_cap);
int64_t     ltr_region_set_size(const ltr_region_set* rs);
int32_t     ltr_region_set_lines_read(const ltr_region_set* rs);     /* the reference's "Region file contains N regions" */
void        ltr_region_set_order(ltr_region_set* rs);
void        ltr_region_set_free(ltr_region_set* rs);
const char* ltr_region_chrom(const ltr_region_set* rs, int64_t i);
const char* ltr_region_name(const ltr_region_set* rs, int64_t i);     /* "" when the line has no fifth column */
const char* ltr_region_motif(const ltr_region_set* rs, int64_t i);
const char* ltr_region_period_str(const ltr_region_set* rs, int64_t i);
int32_t     ltr_region_start(const ltr_region_set* rs, int64_t i);
int32_t     ltr_region_stop(const ltr_region_set* rs, int64_t i);
int32_t     ltr_region_period(const ltr_region_set* rs, int64_t i);
/* FastaReader (src/fasta_reader.h:25-118, .cpp:10-95): one FASTA file with its .fai, or a directory whose *.fa files
 * each have one.  ltr_fasta_fetch = get_sequence(chrom, start, end): 0-based, end inclusive, clamped to the sequence
 * like faidx_fetch_seq; returns the number of bases.  ltr_fasta_seq_len: -1 for an unknown name.
 * ltr_fasta_contig_lines = write_all_contigs_to_vcf (the ##contig header lines). */
typedef struct ltr_fasta ltr_fasta;
int         ltr_fasta_open(const char* path, ltr_fasta** out, char* err, int err_cap);
void        ltr_fasta_close(ltr_fasta* fa);
int64_t     ltr_fasta_num_seqs(const ltr_fasta* fa);
const char* ltr_fasta_seq_name(const ltr_fasta* fa, int64_t i);
int64_t     ltr_fasta_seq_len(const ltr_fasta* fa, const char* chrom);
int64_t     ltr_fasta_fetch(ltr_fasta* fa, const char* chrom, int64_t start, int64_t end, char* out, int64_t cap, char* err, int err_cap);
int64_t     ltr_fasta_contig_lines(const ltr_fasta* fa, char* out, int64_t cap);
/* VCFWriter (src/vcf_writer.h:25-84, .cpp:3-36): records are held in a heap by position and written once no later
 * record of the chromosome can precede them (MAX_RECORD_PAD = 50 bp), all of them at a chromosome change and at
 * close.  A path ending in ".gz" / ".bgz" is written as BGZF like the reference's bgzfostream (src/bgzf_streams.h),
 * any other path as the same text uncompressed.  ltr_vcf_writer_close also frees the writer. */
typedef struct ltr_vcf_writer ltr_vcf_writer;
int ltr_vcf_writer_open(const char* path, ltr_vcf_writer** out);
int ltr_vcf_writer_header(ltr_vcf_writer* w, const char* text);
int ltr_vcf_writer_add_record(ltr_vcf_writer* w, const char* chrom, int32_t record_pos, const char* record_text);
int ltr_vcf_writer_close(ltr_vcf_writer* w);

/* Tabix-indexed VCF input without htslib (ltr_vcf_in.cpp), the --ref-vcf panel of candidate alleles.
 * ltr_vcf_reader_open = VCFReader::open (src/vcf_reader.cpp:74-105): a BGZF VCF and its <path>.tbi (magic "TBI\1": the BAI
 * binning and linear index behind format, col_seq / beg / end, meta char, skip and the reference names); an unreadable file,
 * a missing or damaged index return LTR_ERR_INVALID with the reference's message.  The # header lines are read past, not kept.
 * ltr_vcf_read_alleles = read_vcf_alleles (src/vcf_input.cpp:21-50): the records overlapping [max(0, start-50), stop+50),
 * those whose INFO lacks START or END skipped, the first with START == region_start+1 and END == region_stop taken, the scan
 * ended by a record with POS > region_start+50.  1 = found: *pos = POS-1, the alleles REF first then the ALTs in file order,
 * laid out like ltr_get_alleles (allele_off has n_alleles + 1 entries, at most cap + 1: no allele is empty); 0 = not found
 * (an unknown chromosome included), *pos = -1; < 0 = a malformed record or too small a buffer.
 * ltr_vcf_index = tabix -p vcf: writes <path>.tbi (format 2, columns 1 / 2 / 0, meta '#', skip 0) for a position-sorted
 * BGZF VCF; a record is binned by [POS-1, max(POS-1+len(REF), INFO END)), the interval a query tests, so that no query
 * misses it.  The bins need not match htslib's byte for byte.  Not read: .csi indexes, plain-text VCFs. */
typedef struct ltr_vcf_reader ltr_vcf_reader;
int  ltr_vcf_reader_open(const char* path, ltr_vcf_reader** out, char* err, int err_cap);
void ltr_vcf_reader_close(ltr_vcf_reader* r);
int  ltr_vcf_read_alleles(ltr_vcf_reader* r, const char* chrom, int32_t region_start, int32_t region_stop, int32_t* pos,
                          char* out, int64_t cap, int64_t* allele_off, int32_t* n_alleles);
int  ltr_vcf_index(const char* path);
/* Test hooks.  ltr_debug_vcf_query: the lines (each + '\n') of the records overlapping [start, end); returns their length.
 * ltr_debug_tbi_parse: a .tbi on its own; header[6] = format, col_seq, col_beg, col_end, meta, skip; counts[2r], counts[2r+1]
 * = bins and chunks of reference r (the metadata pseudo-bin excluded); names back to back, NUL-terminated; returns the number
 * of references, LTR_ERR_INVALID for an unreadable index or a chunk whose start lies after its end. */
int64_t ltr_debug_vcf_query(ltr_vcf_reader* r, const char* chrom, int64_t start, int64_t end, char* out, int64_t cap);
int32_t ltr_debug_tbi_parse(const char* tbi_path, int32_t* header, int64_t* counts, int32_t cap_refs, char* names, int64_t names_cap);

/* Indexed BAM input without htslib (ltr_bam.cpp): one or more position-sorted *.bam files, each with its *.bam.bai
 * (or *.bai), read as ONE stream like BamCramMultiReader (src/bam_io.h:520-583, src/bam_io.cpp:201-244):
 * merge_by_position != 0 orders the records of all files by position (ORDER_ALNS_BY_POSITION), 0 file by file.
 * ltr_bam_set_region(chrom, start, end) = SetRegion (bam_io.cpp:142-169, 201-220): the records overlapping the 0-based
 * half-open [start, end) (htslib region "chrom:start+1-end"), up to the first one that starts after end + 1.
 * ltr_bam_next = GetNextAlignment (bam_io.cpp:172-197, 222-244) + ExtractSequenceFields (:14-40): 1 = a record, 0 =
 * done; the pointers of the record stay valid until the next ltr_bam_next / ltr_bam_set_region on the handle.
 * The CIGAR comes as the two arrays ltr_alignment wants; quals are Phred + 33.  CRAM is not read. */
typedef struct ltr_bam ltr_bam;
typedef struct ltr_bam_record {
  const char*    name;
  int32_t        file_index;            /* which of the opened files */
  int32_t        ref_id, pos, end_pos;  /* 0-based start; end_pos = bam_endpos (one past the last reference base) */
  int32_t        mapq, flag;
  int32_t        mate_ref_id, mate_pos, tlen;
  int32_t        length;                /* l_seq */
  const char*    bases;                 /* [length] "=ACMGRSVTWYHKDBN" decoding, NUL-terminated */
  const char*    quals;                 /* [length] Phred + 33, NUL-terminated */
  int32_t        n_cigar;
  const char*    cigar_type;            /* [n_cigar] MIDNSHP=X */
  const int32_t* cigar_num;
  const uint8_t* aux; int32_t aux_len;  /* the raw tag block (ltr_bam_aux_*) */
} ltr_bam_record;
int         ltr_bam_open(const char* const* paths, int32_t n_files, int32_t merge_by_position, ltr_bam** out, char* err, int err_cap);
void        ltr_bam_close(ltr_bam* b);
int32_t     ltr_bam_num_refs(const ltr_bam* b);
const char* ltr_bam_ref_name(const ltr_bam* b, int32_t i);
int64_t     ltr_bam_ref_len(const ltr_bam* b, int32_t i);
int32_t     ltr_bam_num_read_groups(const ltr_bam* b);           /* @RG lines of all files (BamHeader::parse_read_groups, bam_io.cpp:43-70) */
const char* ltr_bam_read_group_id(const ltr_bam* b, int32_t i);
const char* ltr_bam_read_group_sample(const ltr_bam* b, int32_t i);
const char* ltr_bam_read_group_library(const ltr_bam* b, int32_t i);
int32_t     ltr_bam_read_group_file(const ltr_bam* b, int32_t i);
int         ltr_bam_set_region(ltr_bam* b, const char* chrom, int32_t start, int32_t end);
int         ltr_bam_next(ltr_bam* b, ltr_bam_record* rec);
/* BamAlignment::GetIntTag / GetFloatTag / GetCharTag / GetStringTag (src/bam_io.h:182-212): 1 = present with that type */
int         ltr_bam_aux_int(const ltr_bam_record* rec, const char tag[2], int64_t* value);
int         ltr_bam_aux_float(const ltr_bam_record* rec, const char tag[2], double* value);
int         ltr_bam_aux_char(const ltr_bam_record* rec, const char tag[2], char* value);
const char* ltr_bam_aux_string(const ltr_bam_record* rec, const char tag[2]);      /* NULL when absent */

/* ---- timers ------------------------------------------------------------------ */
/*
 * The reference's per-genotyper clocks, accumulated per context (wall-clock seconds here, clock() CPU
 * seconds there; reset != 0 zeroes them after the read):
 *   hap_build_s   total_hap_build_time_ (seq_stutter_genotyper.cpp:417,479-480): candidate generation and
 *                 haplotype construction -- ltr_build_haplotype, ltr_haplotype_align_to_ref
 *   hap_aln_s     total_hap_aln_time_ (:515,:561-562): everything inside ltr_process_reads, ltr_align_batch
 *                 and ltr_calc_hap_aln_probs (host preparation, upload, kernels, download, scatter)
 *   posterior_s   total_posterior_time_ (genotyper.cpp:46,:80-81): ltr_posteriors, ltr_plan_posteriors, ltr_plan_genotype
 *   dp_kernel_ms  device time of the DP kernels inside hap_aln_s (HIP events around every execute)
 *   nw_kernel_ms  device time of the Needleman-Wunsch kernels inside hap_build_s (HIP events, first launch to last)
 *   short_kernel_ms  device time of the seeded stutter path's kernels inside hap_aln_s (same)
 *   dp_cells, dp_pairs  what those DP kernels scored: nominal cells (ltr_plan_cells) and pairs of every plan executed and
 *                 fetched -- for ltr_calc_hap_aln_probs the pairs left AFTER pooling and the de-duplication of trimmed reads,
 *                 i.e. the work the call really did, not reads x haplotypes
 */
typedef struct ltr_timers {
  double  hap_build_s, hap_aln_s, posterior_s, dp_kernel_ms;
  int64_t hap_build_calls, hap_aln_calls, posterior_calls;
  double  nw_kernel_ms, short_kernel_ms;
  double  dp_cells;
  int64_t dp_pairs;
} ltr_timers;
int ltr_ctx_timers(ltr_ctx* ctx, ltr_timers* out, int reset);
/* The same for a caller built against another version of this header: at most out_bytes are written (a longer struct of a
 * newer caller keeps its tail; a shorter one of an older caller is not overrun). */
int ltr_ctx_timers_n(ltr_ctx* ctx, void* out, size_t out_bytes, int reset);
/* Measurement aid: with ltr_ctx_set_debug(ctx, "short_split", 1) the seeded stutter path (HapAligner.cpp:27-233) records events
 * between its launches; out_ms = device milliseconds summed over the calls since the last reset: [0] quality tables + flank rows
 * before the stutter block (:36-44, :112-159), [1] the stutter-block row (:64-111, StutterAlignerClass.cpp:59-154), [2] flank rows
 * after it, [3] the seed log-sum (compute_aln_logprob, :165-233). */
int ltr_ctx_short_kernel_split(ltr_ctx* ctx, double out_ms[4], int reset);

/* ---- host threads -------------------------------------------------------------- */
/*
 * The reference is one thread per process and N processes per node (README.md:78-82).  This library's host loops -- pooling,
 * trimming and planning inside ltr_calc_hap_aln_probs (seq_stutter_genotyper.cpp:514-563), the string passes of the NW call --
 * run on worker threads of the PROCESS (two pools), never more than the budget each:
 *   rule = min(CPUs of the affinity mask, cgroup CPU quota, hardware threads) / ranks on this host, clamped to 1 .. 16,
 * ranks on this host = LOCAL_WORLD_SIZE of the environment (torch.distributed.run sets it) or 1.  The helper thread that stages
 * the next chunk of ltr_calc_hap_aln_probs while the current one is planned is used from a budget of 12 up (below that two
 * thread teams on a handful of cores lose to one).  Results never depend on the budget.
 *   ltr_ctx_set_host_threads   n >= 1: the budget (per process: every context shares the pools); 0: back to the rule
 *   ltr_ctx_host_threads       the budget in force
 *   ltr_host_threads_rule      what the rule gives for `local_world_size` ranks on this host (<= 0: LOCAL_WORLD_SIZE); needs no
 *                              context: a launcher that knows its rank count calls ltr_ctx_set_host_threads(ctx, ltr_host_threads_rule(n))
 */
int ltr_ctx_set_host_threads(ltr_ctx* ctx, int n);
int ltr_ctx_host_threads(const ltr_ctx* ctx);
int ltr_host_threads_rule(int local_world_size);

/* ABI of this header: bumped whenever a struct grows or a capacity contract changes (6: ltr_timers carries dp_cells / dp_pairs
 * since round 5; ltr_plan_kernel_ranges may return up to ltr_num_kernels() ranges; round 6 added the functions above and
 * ltr_ctx_wg_first_pass).  A caller checks ltr_abi_version() == LTR_ABI_VERSION before passing structs. */
#define LTR_ABI_VERSION 6
int ltr_abi_version(void);
const char* ltr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LTR_GPU_H_ */
