// ltr_posterior_common.h -- the pieces that ltr_posterior.hip, ltr_plan_genotype.hip and ltr_plan_fields.hip have in common, once:
// the priors, the clamped column read, the normalise + first-maximum routine of the finish kernels, the upload of a posterior
// batch's read arrays.  Private to those three units.
#pragma once

#include <cmath>

#include "ltr_ctx.h"
#include "../../include/ltr_gpu_ploidy.h"

// int_log(v) == log(v) (mathops.cpp:14-22); priors of genotyper.cpp:21-33 (host libm)
inline void ltr_log_priors(int32_t H, int haploid, double* homoz, double* hetz) {
  const double lH = std::log((double)H), lH1 = std::log((double)(H + 1));
  *homoz = haploid ? -lH : std::log(2.0) - lH - lH1;
  *hetz = haploid ? -1.7976931348623157e308 / 2 : -lH - lH1;
}

// The ploidy of every locus of a call.  The reference decides it per chromosome (genotyper_bam_processor.cpp:248 -> :294, --haploid-chrs);
// a plan or an LL batch cuts across chromosomes, so the *_ploidy entry points take it per locus: the caller's array [n_loci]
// (pb->haploid is then not read), or null = pb->haploid for every locus.
struct LocusPloidy {
  const uint8_t* per_locus; int batch;
  LocusPloidy(const ltr_posterior_batch* pb, const uint8_t* locus_haploid) : per_locus(locus_haploid), batch(locus_haploid ? 0 : (pb->haploid ? 1 : 0)) {}
  int operator()(int64_t l) const { return per_locus ? (per_locus[l] ? 1 : 0) : batch; }
};
// ... and of every (locus, sample) (ltr_gpu_ploidy.h): the caller's array in unit order, or null = the locus's own for each of its
// samples.  all(l, u0, S): what stays per locus -- 1 exactly when every sample of the locus is haploid (a locus without a sample
// keeps the locus's own).
struct SamplePloidy {
  const uint8_t* per_unit; LocusPloidy locus;
  SamplePloidy(const ltr_posterior_batch* pb, const uint8_t* locus_haploid, const uint8_t* sample_haploid) : per_unit(sample_haploid), locus(pb, locus_haploid) {}
  int operator()(int64_t l, int64_t unit) const { return per_unit ? (per_unit[unit] ? 1 : 0) : locus(l); }
  int all(int64_t l, int64_t u0, int32_t S) const {
    if (!per_unit || S <= 0) return locus(l);
    for (int32_t s = 0; s < S; ++s) if (!per_unit[u0 + s]) return 0;
    return 1;
  }
};

// column a of a read's row in the final haplotype order (cmap: new_to_old, null = identity), clamped
__device__ __forceinline__ double ltr_clamped_ll(const double* __restrict__ row, const int32_t* __restrict__ cmap, int a) {
  const int src = cmap ? cmap[a] : a;
  double v = src >= 0 ? row[src] : -100000.0;                   // a haplotype without an old column, seq_stutter_genotyper.cpp:367
  if (v < -600.0) v = -600.0;                                   // genotyper.cpp:57-58
  return v;
}

// One thread, one [H x H] block: log_sum_exp normalise (genotyper.cpp:67-75, mathops.cpp:47-53) + argmax (:85-100).
// Single thread on purpose: the sum must run in index order to match the reference's rounding; the first maximum wins.
// Total and best pair go to slot `slot` of stl / gts.
__device__ __forceinline__ void ltr_normalise_argmax(double* p, int H, double* stl, int* gts, int slot) {
  const int nd = H * H;
  double mx = p[0];
  for (int i = 1; i < nd; ++i) if (mx < p[i]) mx = p[i];
  double tot = 0.0;
  for (int i = 0; i < nd; ++i) tot += exp(p[i] - mx);
  const double total = mx + log(tot);
  stl[slot] = total;
  double best = -1.7976931348623157e308; int b1 = -1, b2 = -1;
  for (int i = 0; i < nd; ++i) {
    const double v = p[i] - total;
    p[i] = v;
    if (v > best) { best = v; b1 = i / H; b2 = i % H; }
  }
  gts[2 * slot] = b1; gts[2 * slot + 1] = b2;
}

// Where the log-likelihoods of a genotype call (ltr_plan_genotype.hip, ltr_plan_fields.hip) lie and how they are read:
//   a plan's LL buffer    [P_l x H_l] blocks at the plan's offsets; a read's row is its pool's; seeds per pool, all loci back to back
//   per-read matrices     (ltr_ll_genotype) [R_l x H_l] blocks uploaded back to back; a read's row is its own; seeds per read
struct LlSource {
  const double* base = nullptr;                // device
  const int64_t* locus_off = nullptr;          // [n_loci] (host) the locus block in base
  const int32_t* H = nullptr;                  // [n_loci] (host) its row length
  const int32_t* P = nullptr;                  // [n_loci] (host) its rows; null with direct (one per read)
  bool direct = false;                         // the read-to-row rule: false = pool_index[r], true = r - r0 (no pool_index anywhere)
  const int32_t* pool_seed = nullptr;          // (host) seed position per pool
  const int32_t* const* read_seed = nullptr;   // direct: [n_loci] seed position per read; null, or a null entry: every read aligned
  const char* who = "ltr_plan_genotype";       // the entry point, for error texts
};

// the read arrays of a posterior batch on the device (pool_index: null when the LL source has a row per read)
struct DevReads { int32_t *pool_index = nullptr, *label = nullptr; double *lp1 = nullptr, *lp2 = nullptr; };
inline int upload_reads(ltr_ctx* ctx, DevLease& lease, const ltr_posterior_batch* pb, DevReads* d, bool with_pool_index = true) {
  const size_t nr = (size_t)pb->n_reads, n1 = std::max<size_t>(nr, 1);
  if (with_pool_index) DEV_TRY(ctx, lease.alloc(&d->pool_index, n1 * 4));
  DEV_TRY(ctx, lease.alloc(&d->label, n1 * 4));
  DEV_TRY(ctx, lease.alloc(&d->lp1, n1 * 8));
  DEV_TRY(ctx, lease.alloc(&d->lp2, n1 * 8));
  if (nr == 0) return LTR_OK;
  if (with_pool_index) DEV_TRY(ctx, hipMemcpyAsync(d->pool_index, pb->pool_index, nr * 4, hipMemcpyHostToDevice, lease.st));
  DEV_TRY(ctx, hipMemcpyAsync(d->label, pb->sample_label, nr * 4, hipMemcpyHostToDevice, lease.st));
  DEV_TRY(ctx, hipMemcpyAsync(d->lp1, pb->log_p1, nr * 8, hipMemcpyHostToDevice, lease.st));
  DEV_TRY(ctx, hipMemcpyAsync(d->lp2, pb->log_p2, nr * 8, hipMemcpyHostToDevice, lease.st));
  return LTR_OK;
}
