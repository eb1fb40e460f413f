// ltr_plan_fields.hip -- what SeqStutterGenotyper::write_vcf_record (reference seq_stutter_genotyper.cpp:894-1366) computes
// before it prints, for every locus of a genotyped plan, on the posterior blocks and the LL buffer where they lie on the device:
//   Genotyper::extract_genotypes_and_likelihoods (genotyper.cpp:132-256) with calc_PLs (:102-107) and calc_gl_diff (:109-130),
//   as ltr_genotype.cpp:60-155 restates them, operation for operation in that order;
//   the per-read bookkeeping of write_vcf_record (:929-1043, long path), as ltr_vcf.cpp's ltr_vcf_fields restates it.
// Host: the views (ltr_genotype_result_fields) and the records of a whole result (ltr_genotype_result_vcf_records).
// Built like every unit with -ffp-contract=off and correctly rounded FP32 division (hipcc's default); no fast-math.

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ltr_plan_fields.h"

namespace {

using ltrf::FieldArgs;
using ltrf::FieldLocus;
using ltrf::FieldUnit;

// fastexp / fastlog of fastonebigheader.h:189-204, :321-337 in float, as ltr_genotype.cpp:24-41
__device__ __forceinline__ float f_approx_pow2(float p) {
  const float offset = (p < 0) ? 1.0f : 0.0f;
  const float clipped = (p < -126) ? -126.0f : p;
  const int whole = (int)clipped;                                // truncation toward zero
  const float frac = clipped - (float)whole + offset;
  const float scaled = (float)(1 << 23) * (clipped + 121.2740575f + 27.7280233f / (4.84252568f - frac) - 1.49012907f * frac);
  return __uint_as_float((uint32_t)scaled);
}
__device__ __forceinline__ float f_approx_exp(float p) { return f_approx_pow2(1.442695040f * p); }
__device__ __forceinline__ float f_approx_log2(float x) {
  const uint32_t xi = __float_as_uint(x);
  const float mant = __uint_as_float((xi & 0x007FFFFFu) | 0x3f000000u);
  float y = (float)xi;
  y *= 1.1920928955078125e-7f;
  return y - 124.22551499f - 1.498030302f * mant - 1.72587999f / (0.3520887068f + mant);
}
__device__ __forceinline__ float f_approx_log(float x) { return 0.69314718f * f_approx_log2(x); }
// fast_log_sum_exp(double, double), mathops.cpp:87-96; log_thresh = log(0.001) from the host (mathops.h:36)
__device__ __forceinline__ double f_fast_lse2(double a, double b, double log_thresh) {
  const double hi = (a > b) ? a : b;
  const double diff = (a > b) ? (b - a) : (a - b);
  if (diff < log_thresh) return hi;
  return hi + f_approx_log(1 + f_approx_exp((float)diff));
}
__device__ __forceinline__ double f_lse2(double a, double b) {   // mathops.cpp:55-60
  return (a > b) ? a + log(1 + exp(b - a)) : b + log(1 + exp(a - b));
}
__device__ __forceinline__ double f_ll(const double* __restrict__ row, const int32_t* __restrict__ cmap, int a) {   // gt_ll of ltr_plan_genotype.hip
  const int src = cmap ? cmap[a] : a;
  double v = src >= 0 ? row[src] : -100000.0;                   // seq_stutter_genotyper.cpp:367
  if (v < -600.0) v = -600.0;                                   // genotyper.cpp:57-58
  return v;
}
// maximum over the workgroup (exact whatever the order); s_red: NT doubles
template <int NT>
__device__ __forceinline__ double block_max(double v, double* s_red, int tid) {
  s_red[tid] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) { const double w = s_red[tid + o]; if (s_red[tid] < w) s_red[tid] = w; }
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}

// One (locus, sample) per workgroup.
//  1. genotype posteriors (genotyper.cpp:152-172): thread per (allele, allele) cell; the streaming log-sum-exp
//     (mathops.cpp:70-85) of a cell visits its haplotype pairs `for h1 in haps(a) ascending, for h2 in haps(b) ascending`,
//     the host's (h1, h2) order restricted to the cell.  Every posterior is read once, from global memory; the V x V
//     table stays in LDS when it fits (cell_off < 0).
//  2. thread 0: best_gts, the haplotype and genotype posteriors of the best pair (:147-150, :174-198).
//  3. thread per genotype: GL (:204-241), PHASEDGL; then the maximum and the runner-up (exact in any order), calc_gl_diff, calc_PLs.
//  4. thread per read of the sample: the strand haplotype (:965-967) and its allele (:1038-1040); read counts (:1006-1012).
template <int NT>
__global__ __launch_bounds__(NT) void ltr_genotype_fields_kernel(const FieldArgs A, int unit0, double log_thresh) {
  extern __shared__ double s_cells[];
  __shared__ double s_red[NT];
  __shared__ int s_cnt[4];
  const double LOG_E_BASE_10 = 0.4342944819;                     // mathops.cpp:12
  const FieldUnit u = A.units[unit0 + (int)blockIdx.x];
  const FieldLocus L = A.loci[u.locus];
  const int tid = threadIdx.x, V = L.V, Hn = L.Hn, VV = V * V, n_gl = L.n_gl;
  const int32_t* __restrict__ h2a = A.tab + L.tab_off;
  const int32_t* __restrict__ afirst = h2a + Hn;
  const int32_t* __restrict__ alist = afirst + V + 1;
  const double* __restrict__ post = A.post[u.pass] + u.post_off;
  double* cells = u.cell_off >= 0 ? A.cells + u.cell_off : s_cells;
  const int ha = A.gts[u.pass][2 * u.src], hb = A.gts[u.pass][2 * u.src + 1];
  if (tid < 4) s_cnt[tid] = 0;
  if (ha < 0 || hb < 0) {                                        // no optimal pair (NaN scores): the host refuses the locus
    if (tid == 0) { A.best_gts[2 * u.out] = -1; A.best_gts[2 * u.out + 1] = -1; }
    return;
  }
  for (int g = tid; g < VV; g += NT) {
    const int a = g / V, b = g - a * V;
    double mx = -DBL_MAX / 2, tot = 0.0;
    for (int i = afirst[a]; i < afirst[a + 1]; ++i) {
      const double* row = post + (int64_t)alist[i] * Hn;
      for (int j = afirst[b]; j < afirst[b + 1]; ++j) {
        const double p = row[alist[j]];
        if (p <= mx) tot += exp(p - mx);
        else { tot *= exp(mx - p); tot += 1.0; mx = p; }
      }
    }
    cells[g] = mx + log(tot);
  }
  __syncthreads();
  const int ga = h2a[ha], gb = h2a[hb];
  if (tid == 0) {
    A.best_gts[2 * u.out] = ga; A.best_gts[2 * u.out + 1] = gb;
    const int64_t ia = (int64_t)ha * Hn + hb, ib = (int64_t)hb * Hn + ha;
    const double phased = cells[V * ga + gb];
    A.scalars[0 * A.nu + u.out] = phased;
    A.scalars[1 * A.nu + u.out] = (ga == gb) ? phased : f_lse2(phased, cells[V * gb + ga]);
    A.scalars[2 * A.nu + u.out] = post[ia];
    A.scalars[3 * A.nu + u.out] = (ia != ib) ? f_fast_lse2(post[ia], post[ib], log_thresh) : post[ia];
  }
  const double stl = A.stl[u.pass][u.src];
  double* gls = A.gls + L.gl_off + (int64_t)u.sample * n_gl;
  double my_max = -INFINITY;
  for (int k = tid; k < n_gl; k += NT) {
    int a = k, b = k;
    if (!L.haploid) {                                            // k = a (a + 1) / 2 + b, b <= a
      a = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > k) --a;
      while ((a + 1) * (a + 2) / 2 <= k) ++a;
      b = k - a * (a + 1) / 2;
    }
    const double ln_gl = stl - (a == b ? L.hom_gl : L.het_gl) + f_fast_lse2(cells[a * V + b], cells[b * V + a], log_thresh);
    const double gl = ln_gl * LOG_E_BASE_10;                     // ln -> log10, :234
    gls[k] = gl;
    if (my_max < gl) my_max = gl;
  }
  if (A.pgls) {
    double* __restrict__ pg = A.pgls + L.pgl_off + (int64_t)u.sample * L.n_pgl;
    for (int k = tid; k < L.n_pgl; k += NT) {
      const int a = L.haploid ? k : k / V, b = L.haploid ? k : k - a * V;
      pg[k] = (stl - (a == b ? L.hom_pgl : L.het_pgl) + cells[a * V + b]) * LOG_E_BASE_10;
    }
  }
  const double max_gl = block_max<NT>(my_max, s_red, tid);       // (its barriers also publish gls to the workgroup)
  double my_second = -DBL_MAX;
  for (int k = tid; k < n_gl; k += NT) { const double g = gls[k]; if (g < max_gl && g > my_second) my_second = g; }
  double second = block_max<NT>(my_second, s_red, tid);
  if (tid == 0) {                                                // calc_gl_diff, :109-130
    double d;
    if (Hn == 1) d = -1000;
    else {
      if (second == -DBL_MAX) second = max_gl;
      const int hi = ga > gb ? ga : gb, lo = ga < gb ? ga : gb;
      const double gi = gls[L.haploid ? ga : hi * (hi + 1) / 2 + lo];
      d = (fabs(max_gl - gi) < 1e-10) ? (max_gl - second) : gi - max_gl;
    }
    A.scalars[4 * A.nu + u.out] = d;
  }
  if (A.pls) {                                                   // calc_PLs, :102-107
    int32_t* __restrict__ pl = A.pls + L.gl_off + (int64_t)u.sample * n_gl;
    for (int k = tid; k < n_gl; k += NT) { const int v = (int)(-10 * (gls[k] - max_gl)); pl[k] = v < 999 ? v : 999; }
  }
  const int32_t* cmap = L.map_off >= 0 ? A.map + L.map_off : nullptr;
  for (int r = L.r0 + tid; r < L.r1; r += NT) {
    if (A.label[r] != u.sample) continue;
    const double p1 = A.lp1[r], p2 = A.lp2[r];
    int strand = 0;
    if (!L.haploid && ha != hb) {
      const double* row = A.ll + L.ll_off + (int64_t)A.pool_index[r] * L.H;
      strand = (p1 + f_ll(row, cmap, ha) > p2 + f_ll(row, cmap, hb)) ? 0 : 1;      // :965-967
    }
    A.read_allele[r] = strand == 0 ? ga : gb;
    atomicAdd(&s_cnt[0], 1);
    if (fabs(p1 - p2) > 1e-10) {                                 // TOLERANCE, :1006-1012
      atomicAdd(&s_cnt[1], 1);
      atomicAdd(p1 > p2 ? &s_cnt[2] : &s_cnt[3], 1);
    }
  }
  __syncthreads();
  if (tid < 4) A.counts[(int64_t)tid * A.nu + u.out] = s_cnt[tid];
}

}  // namespace

namespace ltrf {

void launch_fields(hipStream_t st, const FieldArgs& a, size_t n_small, int cell_cap_small, size_t n_large, int cell_cap_large) {
  const double log_thresh = std::log(0.001);                     // LOG_THRESH, mathops.h:36
  if (n_small)
    hipLaunchKernelGGL(ltr_genotype_fields_kernel<64>, dim3((unsigned)n_small), dim3(64), (size_t)cell_cap_small * sizeof(double), st, a, 0, log_thresh);
  if (n_large)
    hipLaunchKernelGGL(ltr_genotype_fields_kernel<256>, dim3((unsigned)n_large), dim3(256), (size_t)cell_cap_large * sizeof(double), st, a, (int)n_small, log_thresh);
}

}  // namespace ltrf

extern "C" {

int ltr_genotype_result_fields(const ltr_genotype_result* r, int64_t l, ltr_locus_fields* out) {
  if (!r || !out || !r->has_fields || l < 0 || l >= r->n_loci) return LTR_ERR_INVALID;
  const int64_t nu = r->unit_off[(size_t)r->n_loci], u0 = r->unit_off[(size_t)l];
  const int32_t S = r->S[(size_t)l], V = r->f_V[(size_t)l];
  out->S = S; out->R = (int32_t)(r->f_read_off[(size_t)l + 1] - r->f_read_off[(size_t)l]); out->V = V; out->block = r->f_block[(size_t)l];
  out->n_gl = r->haploid ? V : V * (V + 1) / 2; out->n_pgl = r->haploid ? V : V * V;
  const int32_t* i32 = r->f_i32.get();
  const double* f64 = r->f_f64.get();
  out->best_gts = i32 + 2 * u0;
  out->n_aligned = i32 + 2 * nu + u0; out->n_snp = i32 + 3 * nu + u0; out->n_s1 = i32 + 4 * nu + u0; out->n_s2 = i32 + 5 * nu + u0;
  out->read_allele = i32 + 6 * nu + r->f_read_off[(size_t)l];
  out->log_phased = f64 + u0; out->log_unphased = f64 + nu + u0; out->hap_log_phased = f64 + 2 * nu + u0;
  out->hap_log_unphased = f64 + 3 * nu + u0; out->gl_diffs = f64 + 4 * nu + u0;
  out->gls = r->f_gls ? r->f_gls.get() + r->f_gl_off[(size_t)l] : nullptr;
  out->pls = r->f_pls ? r->f_pls.get() + r->f_gl_off[(size_t)l] : nullptr;
  out->phased_gls = r->f_pgls ? r->f_pgls.get() + r->f_pgl_off[(size_t)l] : nullptr;
  return LTR_OK;
}

int ltr_genotype_result_vcf_records(const ltr_genotype_result* r, const ltr_vcf_locus* loci, const ltr_vcf_options* opt,
                                    char** text, int64_t* rec_off, int32_t* pos) {
  if (text) *text = nullptr;
  if (!r || !text || !rec_off || !r->has_fields || (r->n_loci > 0 && !loci)) return LTR_ERR_INVALID;
  ltr_ctx* ctx = r->ctx;
  LTR_GUARD_BEGIN
  const int64_t nl = r->n_loci;
  std::vector<std::string> rec((size_t)nl);
  std::vector<int32_t> rpos((size_t)nl, 0);
  std::vector<int64_t> status((size_t)nl, 0);
  std::atomic<int64_t> bad(-1);
  ltr::parallel_for(nl, 16, [&](int64_t l) {
    ltr_locus_fields f;
    ltr_vcf_locus v = loci[l];
    v.hap = ltr_genotype_result_blocks(r, l);                   // the final block list (the pruned copy, or the caller's)
    v.block = r->f_block[(size_t)l];
    int64_t rc = ltr_genotype_result_fields(r, l, &f);
    if (rc == LTR_OK) rc = ltr::vcf_record_string(&v, &f, opt, &rec[(size_t)l], &rpos[(size_t)l]);
    if (rc < 0) {
      status[(size_t)l] = rc;
      int64_t cur = bad.load();                                  // the first bad locus, whatever the thread count
      while ((cur < 0 || l < cur) && !bad.compare_exchange_weak(cur, l)) {}
    }
  }, 16);
  if (bad.load() >= 0) {
    const int64_t l = bad.load();
    const std::string where = "ltr_genotype_result_vcf_records: locus " + std::to_string(l) + ": ";
    if (status[(size_t)l] == LTR_ERR_NOMEM) { ltr::set_error(ctx, where + "out of host memory"); return LTR_ERR_NOMEM; }
    bool no_pair = false;                                        // best_gts = -1: the kernel found no optimal haplotype pair (NaN scores)
    const int64_t u0 = r->unit_off[(size_t)l];
    for (int32_t k = 0; k < 2 * r->S[(size_t)l]; ++k) no_pair = no_pair || r->f_i32[(size_t)(2 * u0 + k)] < 0;
    ltr::set_error(ctx, where + (no_pair ? "a sample without an optimal haplotype pair (best_gts = -1)"
                                         : "the fields do not fit the locus description (samples, reads, alleles of the block) or a field the options ask for was not computed"));
    return LTR_ERR_INVALID;
  }
  int64_t total = 0;
  for (int64_t l = 0; l < nl; ++l) total += (int64_t)rec[(size_t)l].size() + 1;
  char* buf = (char*)std::malloc((size_t)total + 1);
  if (!buf) { ltr::set_error(ctx, "out of host memory"); return LTR_ERR_NOMEM; }
  int64_t at = 0;
  for (int64_t l = 0; l < nl; ++l) {
    rec_off[l] = at;
    std::memcpy(buf + at, rec[(size_t)l].data(), rec[(size_t)l].size());
    at += (int64_t)rec[(size_t)l].size();
    buf[at++] = '\n';
    if (pos) pos[l] = rpos[(size_t)l];
  }
  rec_off[nl] = at;
  buf[at] = '\0';
  *text = buf;
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

}  // extern "C"
