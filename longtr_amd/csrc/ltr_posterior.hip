// ltr_posterior.hip -- the consumer of the alignment scores: Genotyper::calc_log_sample_posteriors + get_optimal_haplotypes
// (reference genotyper.cpp:21-100) for one locus (ltr_posteriors) and for every locus of a resident plan (ltr_plan_posteriors).

#include <cmath>
#include <cstring>

#include "ltr_posterior_common.h"

using namespace ltrp;                            // class table, Rules, classify_pair, sort_by_class (ltr_plan.h)

namespace {

// ------------------------------------------------------------------------------------------
// posterior kernel (consumer): Genotyper::calc_log_sample_posteriors, genotyper.cpp:45-83
// one workgroup per sample; thread (a1,a2) loops over the sample's reads in read order.
// ------------------------------------------------------------------------------------------
__global__ void ltr_posterior_kernel(int S, int R, int H, double* __restrict__ ll,
                                     const double* __restrict__ lp1, const double* __restrict__ lp2,
                                     const int* __restrict__ sample_label, double homoz, double hetz,
                                     double* __restrict__ post) {
  const int s = blockIdx.x;
  const double LOG_ONE_HALF = -0.6931471805599453094;          // log(0.5), mathops.cpp:10
  const int nd = H * H;
  for (int idx = threadIdx.x; idx < nd; idx += blockDim.x) {
    const int a1 = idx / H, a2 = idx % H;
    double acc = (a1 == a2) ? homoz : hetz;                    // init_log_sample_priors, :35-43
    for (int r = 0; r < R; ++r) {
      if (sample_label[r] != s) continue;
      double v1 = ll[(size_t)r * H + a1], v2 = ll[(size_t)r * H + a2];
      if (v1 < -600.0) v1 = -600.0;                            // clamp, :57-58 (written back by the clamp kernel)
      if (v2 < -600.0) v2 = -600.0;
      acc += log(exp(v1 + lp1[r] + LOG_ONE_HALF) + exp(v2 + lp2[r] + LOG_ONE_HALF));   // :59
    }
    post[(size_t)s * nd + idx] = acc;
  }
}

__global__ void ltr_clamp_kernel(double* ll, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count && ll[i] < -600.0) ll[i] = -600.0;
}

// per sample: log_sum_exp normalise (genotyper.cpp:67-75, mathops.cpp:47-53) + argmax (:85-100), one thread each.
// The text of ltr_normalise_argmax (ltr_posterior_common.h), kept in place: with H uniform over the launch the inlined routine
// compiles to a different branch layout, and the counter summaries of profiles/ are matched to this unit's device code.
__global__ void ltr_posterior_finish_kernel(int S, int H, double* __restrict__ post,
                                            double* __restrict__ stl, int* __restrict__ gts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int nd = H * H;
  double* p = post + (size_t)s * nd;
  double mx = p[0];
  for (int k = 1; k < nd; ++k) if (mx < p[k]) mx = p[k];
  double tot = 0.0;
  for (int k = 0; k < nd; ++k) tot += exp(p[k] - mx);
  const double total = mx + log(tot);
  stl[s] = total;
  double best = -1.7976931348623157e308; int b1 = -1, b2 = -1;
  for (int k = 0; k < nd; ++k) {
    const double v = p[k] - total;
    p[k] = v;
    if (v > best) { best = v; b1 = k / H; b2 = k % H; }
  }
  gts[2 * s] = b1; gts[2 * s + 1] = b2;
}

// ---- batched, plan-resident posteriors: one workgroup per (locus, sample) --------------------
struct PostUnit {            // one (locus, sample)
  int64_t ll_off;            // locus block in the LL buffer ([P x H])
  int64_t post_off;          // this unit's [H x H] block in the posterior buffer
  int32_t r0, r1;            // reads of the locus
  int32_t H, sample;
  double homoz, hetz;        // priors, genotyper.cpp:21-33 (host libm)
};

__global__ void ltr_posterior_batch_kernel(const PostUnit* __restrict__ units, const double* __restrict__ ll,
                                           const int32_t* __restrict__ pool_index, const double* __restrict__ lp1,
                                           const double* __restrict__ lp2, const int32_t* __restrict__ label,
                                           double* __restrict__ post) {
  const PostUnit u = units[blockIdx.x];
  const double LOG_ONE_HALF = -0.6931471805599453094;          // log(0.5), mathops.cpp:10
  const int H = u.H, nd = H * H;
  for (int idx = threadIdx.x; idx < nd; idx += blockDim.x) {
    const int a1 = idx / H, a2 = idx % H;
    double acc = (a1 == a2) ? u.homoz : u.hetz;
    for (int r = u.r0; r < u.r1; ++r) {                         // reads in order, like :52-63
      if (label[r] != u.sample) continue;
      const double* row = ll + u.ll_off + (int64_t)pool_index[r] * H;   // the read's pool row (seq_stutter_genotyper.cpp:531-537)
      double v1 = row[a1], v2 = row[a2];
      if (v1 < -600.0) v1 = -600.0;                              // :57-58
      if (v2 < -600.0) v2 = -600.0;
      acc += log(exp(v1 + lp1[r] + LOG_ONE_HALF) + exp(v2 + lp2[r] + LOG_ONE_HALF));
    }
    post[u.post_off + idx] = acc;
  }
}

// normalise + argmax per unit
__global__ void ltr_posterior_batch_finish_kernel(int n_units, const PostUnit* __restrict__ units, double* __restrict__ post,
                                                  double* __restrict__ stl, int* __restrict__ gts) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_units) return;
  ltr_normalise_argmax(post + units[k].post_off, units[k].H, stl, gts, k);
}

}  // namespace

extern "C" {

// Genotyper::calc_log_sample_posteriors + get_optimal_haplotypes (genotyper.cpp:21-100)
int ltr_posteriors(ltr_ctx* ctx, int32_t S, int32_t R, int32_t H,
                   double* ll, const double* lp1, const double* lp2, const int32_t* sample_label,
                   int32_t haploid, double* post, double* stl, int32_t* gts, double* total_ll) {
  if (!ctx || S <= 0 || R < 0 || H <= 0 || !ll || !lp1 || !lp2 || !sample_label || !post || !stl) return LTR_ERR_INVALID;
  ltr::TimedCall timed(ctx, ltr::kTimerPosterior);             // total_posterior_time_, genotyper.cpp:46,:80-81
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int32_t r = 0; r < R; ++r) if (sample_label[r] < 0 || sample_label[r] >= S) { ltr::set_error(ctx, "sample label out of range"); return LTR_ERR_INVALID; }
  double homoz, hetz;
  ltr_log_priors(H, haploid, &homoz, &hetz);
  const size_t nll = (size_t)R * H, npost = (size_t)S * H * H;
  double *d_ll = nullptr, *d_p1 = nullptr, *d_p2 = nullptr, *d_post = nullptr, *d_stl = nullptr;
  int *d_lab = nullptr, *d_gts = nullptr;
  hipStream_t st = ctx->stream;
  DevLease lease(ctx, st);                               // (every host buffer the copies touch is the caller's or the lease's)
  DEV_TRY(ctx, lease.alloc(&d_ll, std::max<size_t>(nll, 1) * 8));
  DEV_TRY(ctx, lease.alloc(&d_p1, std::max<size_t>(R, 1) * 8));
  DEV_TRY(ctx, lease.alloc(&d_p2, std::max<size_t>(R, 1) * 8));
  DEV_TRY(ctx, lease.alloc(&d_lab, std::max<size_t>(R, 1) * 4));
  DEV_TRY(ctx, lease.alloc(&d_post, npost * 8));
  DEV_TRY(ctx, lease.alloc(&d_stl, (size_t)S * 8));
  DEV_TRY(ctx, lease.alloc(&d_gts, (size_t)S * 8));
  if (R > 0) {
    DEV_TRY(ctx, hipMemcpyAsync(d_ll, ll, nll * 8, hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipMemcpyAsync(d_p1, lp1, (size_t)R * 8, hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipMemcpyAsync(d_p2, lp2, (size_t)R * 8, hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipMemcpyAsync(d_lab, sample_label, (size_t)R * 4, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(ltr_posterior_kernel, dim3((unsigned)S), dim3(256), 0, st, S, R, H, d_ll, d_p1, d_p2, d_lab, homoz, hetz, d_post);
  if (nll) hipLaunchKernelGGL(ltr_clamp_kernel, dim3((unsigned)((nll + 255) / 256)), dim3(256), 0, st, d_ll, (int64_t)nll);
  hipLaunchKernelGGL(ltr_posterior_finish_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, S, H, d_post, d_stl, d_gts);
  DEV_TRY(ctx, hipGetLastError());
  if (nll) DEV_TRY(ctx, hipMemcpyAsync(ll, d_ll, nll * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, hipMemcpyAsync(post, d_post, npost * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, hipMemcpyAsync(stl, d_stl, (size_t)S * 8, hipMemcpyDeviceToHost, st));
  int32_t* g = lease.host<int32_t>((size_t)2 * S);             // (gts may be null; taken here, behind the queued work)
  DEV_TRY(ctx, hipMemcpyAsync(g, d_gts, (size_t)S * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, lease.drain());
  if (gts) std::memcpy(gts, g, (size_t)S * 8);
  if (total_ll) { double t = 0.0; for (int32_t s = 0; s < S; ++s) t += stl[s]; *total_ll = t; }   // sum(), genotyper.cpp:78
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

// Genotyper::calc_log_sample_posteriors + get_optimal_haplotypes for EVERY locus of a resident
// plan, straight from the LL buffer of the last execute (no host round trip of the LL matrix).
// locus_haploid: the ploidy of every locus (genotyper_bam_processor.cpp:248 -> :294 -> the priors, genotyper.cpp:21-33); null = pb->haploid.
// sample_haploid: the ploidy of every (locus, sample) in unit order (ltr_gpu_ploidy.h); null = the locus's.  Only the priors of a unit read it.
static int plan_posteriors(ltr_plan* plan, const ltr_posterior_batch* pb, const uint8_t* locus_haploid, const uint8_t* sample_haploid, double* post, double* sample_total_ll, int32_t* gts) {
  if (!plan || !pb || !post || !sample_total_ll) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  if (!plan->executed) { ltr::set_error(ctx, "ltr_plan_posteriors: execute the plan first"); return LTR_ERR_INVALID; }
  if (pb->n_loci != (int64_t)plan->locus_P.size()) { ltr::set_error(ctx, "posterior batch and plan disagree on the number of loci"); return LTR_ERR_INVALID; }
  ltr::TimedCall timed(ctx, ltr::kTimerPosterior);             // total_posterior_time_, genotyper.cpp:46,:80-81
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<PostUnit> units;                                 // (before the lease: a queued copy reads it)
  const SamplePloidy haploid(pb, locus_haploid, sample_haploid);
  int64_t post_off = 0;
  for (int64_t l = 0; l < pb->n_loci; ++l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1];
    const int32_t H = plan->locus_H[(size_t)l], P = plan->locus_P[(size_t)l], S = pb->n_samples[l];
    if (r0 < 0 || r1 < r0 || r1 > pb->n_reads || S < 0) { ltr::set_error(ctx, "bad posterior batch offsets"); return LTR_ERR_INVALID; }
    for (int64_t r = r0; r < r1; ++r)
      if (pb->pool_index[r] < 0 || pb->pool_index[r] >= P || pb->sample_label[r] < 0 || pb->sample_label[r] >= S) {
        ltr::set_error(ctx, "pool index / sample label out of range"); return LTR_ERR_INVALID;
      }
    for (int32_t sm = 0; sm < S; ++sm) {
      PostUnit u;
      u.ll_off = plan->locus_ll_off[(size_t)l]; u.post_off = post_off; u.r0 = (int32_t)r0; u.r1 = (int32_t)r1; u.H = H; u.sample = sm;
      ltr_log_priors(H, haploid(l, (int64_t)units.size()), &u.homoz, &u.hetz);
      units.push_back(u);
      post_off += (int64_t)H * H;
    }
  }
  const size_t nu = units.size();
  if (nu == 0) return LTR_OK;
  PostUnit* d_units = nullptr; int* d_gts = nullptr;
  double *d_post = nullptr, *d_stl = nullptr;
  DevReads rd;
  hipStream_t st = plan->last_stream;
  DevLease lease(ctx, st);
  DEV_TRY(ctx, lease.alloc(&d_units, nu * sizeof(PostUnit)));
  DEV_TRY(ctx, hipMemcpyAsync(d_units, units.data(), nu * sizeof(PostUnit), hipMemcpyHostToDevice, st));
  if (int rc = upload_reads(ctx, lease, pb, &rd)) return rc;
  DEV_TRY(ctx, lease.alloc(&d_post, (size_t)post_off * 8));
  DEV_TRY(ctx, lease.alloc(&d_stl, nu * 8));
  DEV_TRY(ctx, lease.alloc(&d_gts, nu * 8));
  hipLaunchKernelGGL(ltr_posterior_batch_kernel, dim3((unsigned)nu), dim3(128), 0, st, d_units, plan->last_out, rd.pool_index, rd.lp1, rd.lp2, rd.label, d_post);
  hipLaunchKernelGGL(ltr_posterior_batch_finish_kernel, dim3((unsigned)((nu + 63) / 64)), dim3(64), 0, st, (int)nu, d_units, d_post, d_stl, d_gts);
  DEV_TRY(ctx, hipGetLastError());
  DEV_TRY(ctx, hipMemcpyAsync(post, d_post, (size_t)post_off * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, hipMemcpyAsync(sample_total_ll, d_stl, nu * 8, hipMemcpyDeviceToHost, st));
  int32_t* g = lease.host<int32_t>(2 * nu);                    // (gts may be null; taken here, behind the queued work)
  DEV_TRY(ctx, hipMemcpyAsync(g, d_gts, nu * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, lease.drain());
  if (gts) std::memcpy(gts, g, nu * 8);
  return LTR_OK;
  LTR_GUARD_END(ctx)
}
int ltr_plan_posteriors_ploidy(ltr_plan* plan, const ltr_posterior_batch* pb, const uint8_t* locus_haploid, double* post, double* sample_total_ll, int32_t* gts) {
  return plan_posteriors(plan, pb, locus_haploid, nullptr, post, sample_total_ll, gts);
}
int ltr_plan_posteriors(ltr_plan* plan, const ltr_posterior_batch* pb, double* post, double* sample_total_ll, int32_t* gts) {
  return ltr_plan_posteriors_ploidy(plan, pb, nullptr, post, sample_total_ll, gts);
}
int ltr_plan_posteriors_sample_ploidy(ltr_plan* plan, const ltr_posterior_batch* pb, const uint8_t* sample_haploid, double* post, double* sample_total_ll, int32_t* gts) {
  return plan_posteriors(plan, pb, nullptr, sample_haploid, post, sample_total_ll, gts);
}

}  // extern "C"
