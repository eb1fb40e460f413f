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
#include <atomic>
#include <string>

#include "ltr_plan_fields.h"

namespace ltrf {                  // (the kernel's argument types, of this unit only)

// One locus of the fields kernel.  A mixed locus (haploid and diploid samples, ltr_gpu_ploidy.h) has a second record after those
// of all loci, equal but for the constants, which are the haploid flavour there: its haploid units name that one (FieldUnit.locus).
struct FieldLocus {
  int64_t ll_off, map_off;       // the locus block in the LL buffer ([P x H]); new_to_old in the map buffer, -1: identity
  int64_t tab_off;               // in the table buffer: hap_to_allele [Hn], allele_first [V + 1], haps_by_allele [Hn] (allele, then haplotype, ascending)
  int64_t gl_off, pgl_off;       // sample 0 of the locus in gls / pls and in phased_gls
  int32_t r0, r1, H, Hn, V, haploid, n_gl, n_pgl;   // haploid: every sample of the locus is; n_gl / n_pgl: the row widths that follow from it (a mixed locus has the diploid ones)
  double hom_gl, het_gl, hom_pgl, het_pgl;   // prior + configuration term of a homozygous / heterozygous cell (genotyper.cpp:204-241; host libm), in the flavour of the units that name this record
};
// one (locus, sample)
struct FieldUnit {
  int64_t post_off;              // its [Hn x Hn] block in the posterior buffer of its pass
  int64_t cell_off;              // its [V x V] genotype posteriors in the workspace; -1: they fit LDS
  int32_t locus, sample, out;    // locus: its record in FieldArgs.loci; out: slot in the per-unit outputs
  int32_t src, pass;             // slot in the total / best-pair buffers of pass 0 (first) or 1 (second)
  int32_t haploid;               // the sample's ploidy (res->sample_haploid): the flavour of the constants, the index mapping and the strand rule
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

}  // namespace ltrf

namespace {

using namespace ltrf;

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
// DIRECT: the row rule of the LL source (LlSource): false = a read's row is its pool's, true = its own (A.pool_index null).
template <int NT, bool DIRECT>
__device__ __forceinline__ void fields_unit(const FieldArgs& A, int unit0, double log_thresh) {
  extern __shared__ double s_cells[];
  __shared__ double s_red[NT];
  __shared__ int s_cnt[4];
  const double LOG_E_BASE_10 = 0.4342944819;                     // mathops.cpp:12
  const FieldUnit u = A.units[unit0 + (int)blockIdx.x];
  const FieldLocus L = A.loci[u.locus];
  const int tid = threadIdx.x, V = L.V, Hn = L.Hn, VV = V * V, n_gl = L.n_gl;
  const bool hap = u.haploid != 0;                               // the SAMPLE's ploidy; L.haploid / n_gl / n_pgl are the locus's (row widths)
  const int n_out = hap ? V : n_gl;                              // values of this sample's gls / pls row: a haploid row of a mixed locus keeps 0 after its V
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
  for (int k = tid; k < n_out; k += NT) {
    int a = k, b = k;
    if (!hap) {                                                  // k = a (a + 1) / 2 + b, b <= a
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
    const int n_pout = hap ? (L.haploid ? V : 0) : L.n_pgl;     // a haploid sample of a mixed locus has no phased genotypes: its row stays 0.0
    for (int k = tid; k < n_pout; k += NT) {
      const int a = hap ? k : k / V, b = hap ? k : k - a * V;
      pg[k] = (stl - (a == b ? L.hom_pgl : L.het_pgl) + cells[a * V + b]) * LOG_E_BASE_10;
    }
  }
  const double max_gl = block_max<NT>(my_max, s_red, tid);       // (its barriers also publish gls to the workgroup)
  double my_second = -DBL_MAX;
  for (int k = tid; k < n_out; k += NT) { const double g = gls[k]; if (g < max_gl && g > my_second) my_second = g; }
  double second = block_max<NT>(my_second, s_red, tid);
  if (tid == 0) {                                                // calc_gl_diff, :109-130
    double d;
    if (Hn == 1) d = -1000;
    else {
      if (second == -DBL_MAX) second = max_gl;
      const int hi = ga > gb ? ga : gb, lo = ga < gb ? ga : gb;
      const double gi = gls[hap ? ga : hi * (hi + 1) / 2 + lo];
      d = (fabs(max_gl - gi) < 1e-10) ? (max_gl - second) : gi - max_gl;
    }
    A.scalars[4 * A.nu + u.out] = d;
  }
  if (A.pls) {                                                   // calc_PLs, :102-107
    int32_t* __restrict__ pl = A.pls + L.gl_off + (int64_t)u.sample * n_gl;
    for (int k = tid; k < n_out; k += NT) { const int v = (int)(-10 * (gls[k] - max_gl)); pl[k] = v < 999 ? v : 999; }
  }
  const int32_t* cmap = L.map_off >= 0 ? A.map + L.map_off : nullptr;
  for (int r = L.r0 + tid; r < L.r1; r += NT) {
    if (A.label[r] != u.sample) continue;
    const double p1 = A.lp1[r], p2 = A.lp2[r];
    int strand = 0;
    if (!hap && ha != hb) {
      const double* row = A.ll + L.ll_off + (DIRECT ? (int64_t)(r - L.r0) : (int64_t)A.pool_index[r]) * L.H;
      strand = (p1 + ltr_clamped_ll(row, cmap, ha) > p2 + ltr_clamped_ll(row, cmap, hb)) ? 0 : 1;      // :965-967
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
template <int NT>
__global__ __launch_bounds__(NT) void ltr_genotype_fields_kernel(const FieldArgs A, int unit0, double log_thresh) {
  fields_unit<NT, false>(A, unit0, log_thresh);
}
// ... on per-read matrices (ltr_ll_genotype)
template <int NT>
__global__ __launch_bounds__(NT) void ltr_ll_fields_kernel(const FieldArgs A, int unit0, double log_thresh) {
  fields_unit<NT, true>(A, unit0, log_thresh);
}

// units [0, n_small) in workgroups of 64 threads, [n_small, n_small + n_large) of 256; cell_cap_*: doubles of LDS for the V x V table
void launch_fields(hipStream_t st, const FieldArgs& a, bool direct, size_t n_small, int cell_cap_small, size_t n_large, int cell_cap_large) {
  const double log_thresh = std::log(0.001);                     // LOG_THRESH, mathops.h:36
  if (n_small)
    hipLaunchKernelGGL(direct ? ltr_ll_fields_kernel<64> : ltr_genotype_fields_kernel<64>, dim3((unsigned)n_small), dim3(64), (size_t)cell_cap_small * sizeof(double), st, a, 0, log_thresh);
  if (n_large)
    hipLaunchKernelGGL(direct ? ltr_ll_fields_kernel<256> : ltr_genotype_fields_kernel<256>, dim3((unsigned)n_large), dim3(256), (size_t)cell_cap_large * sizeof(double), st, a, (int)n_small, log_thresh);
}

// the constants of a record in one flavour: priors (the heterozygous one of a haploid call is 0, genotyper.cpp:210) and
// configuration terms (:204-241) as ltr_genotype.cpp:108-111
void set_constants(FieldLocus& F, int haploid) {
  double hom_prior, het_prior;
  ltr_log_priors(F.Hn, haploid, &hom_prior, &het_prior);
  if (haploid) het_prior = 0.0;
  const double lH = std::log((double)F.Hn), lV = std::log((double)F.V), l2 = std::log(2.0);
  const double gl_cfg = haploid ? l2 + lH - lV : l2 + 2 * (lH - lV), pgl_cfg = haploid ? lH - lV : 2 * (lH - lV);
  F.hom_gl = hom_prior + gl_cfg; F.het_gl = het_prior + gl_cfg; F.hom_pgl = hom_prior + pgl_cfg; F.het_pgl = het_prior + pgl_cfg;
}

// sizes and offsets of every locus (res->f_V, f_gl_off, f_pgl_off, f_read_off; floci when the kernel will run); the table entries needed.
// floci: [n_loci + mixed loci]; alt[l]: the second record of a mixed locus (the haploid flavour, for its haploid units), -1: none
int64_t layout_loci(const LlSource* src, const ltr_genotype_batch* gb, ltr_genotype_result* res, FieldLocus* floci, int32_t* alt) {
  const ltr_posterior_batch* pb = gb->pb;
  const int64_t nl = res->n_loci;
  res->f_gl_off.assign((size_t)nl + 1, 0); res->f_pgl_off.assign((size_t)nl + 1, 0);
  res->f_read_off.assign(pb->locus_read_off, pb->locus_read_off + nl + 1);
  int64_t tab = 0, mo = 0, n_alt = 0;
  for (int64_t l = 0; l < nl; ++l) {                             // (the block lists are warm from the caller's checks)
    const LtrPruned* p = res->pruned[(size_t)l].get();
    const ltr_haplotype_blocks* hb = p ? &p->blocks.view : gb->haps[l];
    const int32_t S = res->S[(size_t)l], H = res->H[(size_t)l], Hn = p ? p->Hn : H, V = hb->n_alleles[res->f_block[(size_t)l]];
    res->f_V[(size_t)l] = V;
    if (!floci || !alt) continue;                               // (sizes only: ltr_plan_fields_empty)
    FieldLocus& F = floci[(size_t)l];
    F.ll_off = src->locus_off[l]; F.map_off = p ? mo : -1; F.tab_off = tab;
    F.gl_off = res->f_gl_off[(size_t)l]; F.pgl_off = res->f_pgl_off[(size_t)l];
    const int haploid = res->haploid[(size_t)l];                 // the locus's own (genotyper_bam_processor.cpp:248 -> :294): widths, priors and offsets below follow it
    F.r0 = (int32_t)pb->locus_read_off[l]; F.r1 = (int32_t)pb->locus_read_off[l + 1]; F.H = H; F.Hn = Hn; F.V = V; F.haploid = haploid;
    F.n_gl = haploid ? V : V * (V + 1) / 2; F.n_pgl = haploid ? V : V * V;
    set_constants(F, haploid);
    alt[l] = -1;
    if (res->mixed(l)) {                                         // the same rows and widths, the haploid samples' constants
      alt[l] = (int32_t)(nl + n_alt);
      FieldLocus& A = floci[(size_t)(nl + n_alt++)];
      A = F;
      set_constants(A, 1);
    }
    if (p) mo += p->Hn;
    tab += 2 * (int64_t)Hn + V + 1;
    res->f_gl_off[(size_t)l + 1] = F.gl_off + (int64_t)S * F.n_gl;
    res->f_pgl_off[(size_t)l + 1] = F.pgl_off + (int64_t)S * F.n_pgl;
  }
  return tab;
}

// haps_to_alleles of the FINAL list (:240-248) and the haplotypes of every allele, per locus at F.tab_off; false: malformed blocks
bool fill_tables(const ltr_genotype_batch* gb, const ltr_genotype_result* res, const FieldLocus* floci, int32_t* ftab) {
  std::atomic<int> ferr(0);
  ltr::parallel_for(res->n_loci, 64, [&](int64_t l) {
    const LtrPruned* p = res->pruned[(size_t)l].get();
    const ltr_haplotype_blocks* hb = p ? &p->blocks.view : gb->haps[l];
    const FieldLocus& F = floci[(size_t)l];
    std::vector<int32_t> counts; int64_t nc = 0;
    if (ltr::haplotype_counts(hb, &counts, &nc) != LTR_OK || nc != F.Hn) { ferr.store(1); return; }
    int32_t* h2a = ftab + F.tab_off; int32_t* first = h2a + F.Hn; int32_t* list = first + F.V + 1;
    for (int32_t a = 0; a <= F.V; ++a) first[a] = 0;
    for (int32_t h = 0; h < F.Hn; ++h) {
      const int32_t a = counts[(size_t)((int64_t)h * hb->n_blocks + res->f_block[(size_t)l])];
      if (a < 0 || a >= F.V) { ferr.store(1); return; }
      h2a[h] = a; first[a + 1]++;
    }
    for (int32_t a = 0; a < F.V; ++a) first[a + 1] += first[a];
    std::vector<int32_t> at(first, first + F.V);
    for (int32_t h = 0; h < F.Hn; ++h) list[at[(size_t)h2a[h]]++] = h;
  }, 16);
  return ferr.load() == 0;
}

// units: those of up to kFieldSmallH haplotypes first (one wavefront each), then the others; a V x V table beyond LDS goes to a workspace
struct UnitLayout { size_t n_small = 0; int64_t ncells = 0; int cap_small = 1, cap_large = 1; };
UnitLayout layout_field_units(const ltr_genotype_result* res, const FieldLocus* floci, const int32_t* alt, FieldUnit* funits) {
  const int64_t nl = res->n_loci;
  UnitLayout L;
  for (int64_t l = 0; l < nl; ++l) if (floci[(size_t)l].Hn <= kFieldSmallH) L.n_small += (size_t)res->S[(size_t)l];
  size_t ks = 0, kl = L.n_small;
  int64_t unit2 = 0;                                             // first unit of a pruned locus in the second pass
  for (int64_t l = 0; l < nl; ++l) {
    const LtrPruned* p = res->pruned[(size_t)l].get();
    const FieldLocus& F = floci[(size_t)l];
    const bool small = F.Hn <= kFieldSmallH;
    const int64_t vv = (int64_t)F.V * F.V;
    for (int32_t s = 0; s < res->S[(size_t)l]; ++s) {
      FieldUnit& u = funits[small ? ks++ : kl++];
      u.locus = (int32_t)l; u.sample = s; u.out = (int32_t)(res->unit_off[(size_t)l] + s);
      u.pass = p ? 1 : 0; u.src = p ? (int32_t)(unit2 + s) : u.out;
      u.haploid = res->sample_haploid[(size_t)u.out];
      if (u.haploid && alt[l] >= 0) u.locus = alt[l];
      u.post_off = (p ? p->post_off : res->post1_off[(size_t)l]) + (int64_t)s * F.Hn * F.Hn;
      if (vv > kFieldCellCap) { u.cell_off = L.ncells; L.ncells += vv; }
      else { u.cell_off = -1; int& cap = small ? L.cap_small : L.cap_large; cap = std::max(cap, (int)vv); }
    }
    if (p) unit2 += res->S[(size_t)l];
  }
  return L;
}

}  // namespace

void ltr_plan_fields_empty(const ltr_genotype_batch* gb, ltr_genotype_result* res) {
  layout_loci(nullptr, gb, res, nullptr, nullptr);
  res->f_i32.reset(new int32_t[std::max<size_t>((size_t)gb->pb->n_reads, 1)]()); res->f_f64.reset(new double[1]());
}

int ltr_plan_fields_stage(ltr_ctx* ctx, const LlSource& src, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result* res,
                          const DevReads& rd, const int32_t* d_map, const DevPass pass[2], DevLease& lease) {
  hipStream_t st = lease.st;
  const int64_t nl = res->n_loci;
  const size_t nu = (size_t)res->unit_off[(size_t)nl], nr = (size_t)gb->pb->n_reads;
  size_t n_rec = (size_t)nl;                                     // one record per locus, a second one for a mixed locus
  for (int64_t l = 0; l < nl; ++l) if (res->mixed(l)) ++n_rec;
  FieldLocus* floci = lease.host<FieldLocus>(n_rec);
  int32_t* alt = lease.host<int32_t>((size_t)nl);
  const size_t ntab = (size_t)layout_loci(&src, gb, res, floci, alt);
  int32_t* ftab = lease.host<int32_t>(ntab);
  if (!fill_tables(gb, res, floci, ftab)) { ltr::set_error(ctx, std::string(src.direct ? "ltr_ll_genotype" : "ltr_plan_genotype_fields") + ": malformed haplotype blocks"); return LTR_ERR_INVALID; }
  FieldUnit* funits = lease.host<FieldUnit>(nu);
  const UnitLayout ul = layout_field_units(res, floci, alt, funits);
  const int64_t ngl = res->f_gl_off[(size_t)nl], npgl = res->f_pgl_off[(size_t)nl];
  const size_t ni32 = 6 * nu + nr;
  res->f_i32.reset(new int32_t[ni32]); res->f_f64.reset(new double[5 * nu]);
  if (fr->want_gls) res->f_gls.reset(new double[(size_t)std::max<int64_t>(ngl, 1)]);
  if (fr->want_pls) res->f_pls.reset(new int32_t[(size_t)std::max<int64_t>(ngl, 1)]);
  if (fr->want_phased_gls) res->f_pgls.reset(new double[(size_t)std::max<int64_t>(npgl, 1)]);
  FieldUnit* d_funits = nullptr; FieldLocus* d_floci = nullptr; int32_t *d_ftab = nullptr, *d_fi32 = nullptr, *d_fpls = nullptr;
  double *d_ff64 = nullptr, *d_fgls = nullptr, *d_fpgls = nullptr, *d_fcells = nullptr;
  DEV_TRY(ctx, lease.alloc(&d_funits, nu * sizeof(FieldUnit)));
  DEV_TRY(ctx, lease.alloc(&d_floci, n_rec * sizeof(FieldLocus)));
  DEV_TRY(ctx, lease.alloc(&d_ftab, ntab * 4));
  DEV_TRY(ctx, lease.alloc(&d_fi32, ni32 * 4));
  DEV_TRY(ctx, lease.alloc(&d_ff64, 5 * nu * 8));
  DEV_TRY(ctx, lease.alloc(&d_fgls, (size_t)std::max<int64_t>(ngl, 1) * 8));
  if (fr->want_pls) DEV_TRY(ctx, lease.alloc(&d_fpls, (size_t)std::max<int64_t>(ngl, 1) * 4));
  if (fr->want_phased_gls) DEV_TRY(ctx, lease.alloc(&d_fpgls, (size_t)std::max<int64_t>(npgl, 1) * 8));
  if (ul.ncells) DEV_TRY(ctx, lease.alloc(&d_fcells, (size_t)ul.ncells * 8));
  DEV_TRY(ctx, hipMemcpyAsync(d_funits, funits, nu * sizeof(FieldUnit), hipMemcpyHostToDevice, st));
  DEV_TRY(ctx, hipMemcpyAsync(d_floci, floci, n_rec * sizeof(FieldLocus), hipMemcpyHostToDevice, st));
  DEV_TRY(ctx, hipMemcpyAsync(d_ftab, ftab, ntab * 4, hipMemcpyHostToDevice, st));
  // a unit without an optimal pair (best_gts = -1) writes nothing else: its numbers read 0, not what the pool held before
  DEV_TRY(ctx, hipMemsetAsync(d_fi32, 0, 6 * nu * 4, st));
  DEV_TRY(ctx, hipMemsetAsync(d_ff64, 0, 5 * nu * 8, st));
  if (ngl) DEV_TRY(ctx, hipMemsetAsync(d_fgls, 0, (size_t)ngl * 8, st));
  if (fr->want_pls && ngl) DEV_TRY(ctx, hipMemsetAsync(d_fpls, 0, (size_t)ngl * 4, st));
  if (fr->want_phased_gls && npgl) DEV_TRY(ctx, hipMemsetAsync(d_fpgls, 0, (size_t)npgl * 8, st));
  if (nr) DEV_TRY(ctx, hipMemsetAsync(d_fi32 + 6 * nu, 0xff, nr * 4, st));   // (a read whose label no unit claims cannot exist: the labels were checked; -1 would be refused by the formatter)
  FieldArgs a;
  a.units = d_funits; a.loci = d_floci; a.tab = d_ftab;
  a.ll = src.base; a.pool_index = rd.pool_index; a.lp1 = rd.lp1; a.lp2 = rd.lp2; a.label = rd.label; a.map = d_map;
  for (int k = 0; k < 2; ++k) { a.post[k] = pass[k].post; a.stl[k] = pass[k].stl; a.gts[k] = pass[k].gts; }
  a.best_gts = d_fi32; a.counts = d_fi32 + 2 * nu; a.scalars = d_ff64; a.nu = (int64_t)nu;
  a.gls = d_fgls; a.pls = d_fpls; a.pgls = d_fpgls; a.cells = d_fcells; a.read_allele = d_fi32 + 6 * nu;
  launch_fields(st, a, src.direct, ul.n_small, ul.cap_small, nu - ul.n_small, ul.cap_large);
  DEV_TRY(ctx, hipGetLastError());
  DEV_TRY(ctx, hipMemcpyAsync(res->f_i32.get(), d_fi32, ni32 * 4, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, hipMemcpyAsync(res->f_f64.get(), d_ff64, 5 * nu * 8, hipMemcpyDeviceToHost, st));
  if (fr->want_gls && ngl) DEV_TRY(ctx, hipMemcpyAsync(res->f_gls.get(), d_fgls, (size_t)ngl * 8, hipMemcpyDeviceToHost, st));
  if (fr->want_pls && ngl) DEV_TRY(ctx, hipMemcpyAsync(res->f_pls.get(), d_fpls, (size_t)ngl * 4, hipMemcpyDeviceToHost, st));
  if (fr->want_phased_gls && npgl) DEV_TRY(ctx, hipMemcpyAsync(res->f_pgls.get(), d_fpgls, (size_t)npgl * 8, hipMemcpyDeviceToHost, st));
  return LTR_OK;
}

extern "C" {

int ltr_genotype_result_fields(const ltr_genotype_result* r, int64_t l, ltr_locus_fields* out) {
  if (!r || !out || !r->has_fields || l < 0 || l >= r->n_loci) return LTR_ERR_INVALID;
  const int64_t nu = r->unit_off[(size_t)r->n_loci], u0 = r->unit_off[(size_t)l];
  const int32_t S = r->S[(size_t)l], V = r->f_V[(size_t)l];
  out->S = S; out->R = (int32_t)(r->f_read_off[(size_t)l + 1] - r->f_read_off[(size_t)l]); out->V = V; out->block = r->f_block[(size_t)l];
  const bool haploid = r->haploid[(size_t)l] != 0;
  out->n_gl = haploid ? V : V * (V + 1) / 2; out->n_pgl = haploid ? V : V * V;
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
    v.haploid = r->haploid[(size_t)l];                          // the ploidy the fields were made with: FORMAT and the GL / PL / PHASEDGL widths
    // a mixed locus (v.haploid = 0: the ten-field form) carries the ploidy of its samples to the writer; every other locus is the per-locus case
    const uint8_t* sample_haploid = r->mixed(l) ? r->sample_haploid.data() + r->unit_off[(size_t)l] : nullptr;
    int64_t rc = ltr_genotype_result_fields(r, l, &f);
    if (rc == LTR_OK) rc = ltr::vcf_record_string(&v, &f, opt, &rec[(size_t)l], &rpos[(size_t)l], sample_haploid);
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
