// ltr_plan_genotype.hip -- SeqStutterGenotyper::genotype after the alignment (reference seq_stutter_genotyper.cpp:632-645) for
// every locus of an executed plan: posteriors (genotyper.cpp:21-100), get_unused_alleles (:250-308), remove_alleles ->
// add_and_remove_alleles (:317-409) and the posteriors over the smaller haplotype set (:405-408).
// Device: the posterior arithmetic of both passes and the per-read column gather.  Host (worker pool): the integer bookkeeping
// between the passes, from the first pass's best pairs.

#include <cmath>
#include <cstring>
#include <memory>

#include "ltr_ctx.h"
#include "ltr_plan_fields.h"

namespace {

constexpr int kTileMax = 1024;          // doubles per E table of a workgroup at most (2 tables + the posterior block: <= 32 KB of LDS)
constexpr int kPostCapMax = 2048;       // largest H' x H' block normalised in LDS (it borrows both E tables for its exp terms)

// one (locus, sample) of a pass
struct GtUnit {
  int64_t ll_off;            // locus block in the LL buffer ([P x H])
  int64_t post_off;          // this unit's [Hn x Hn] block in the pass's posterior buffer
  int64_t map_off;           // new_to_old of the locus in the map buffer; -1: identity (first pass)
  int32_t r0, r1;            // reads of the locus (the sample's are those labelled `sample`, taken in read order)
  int32_t H, Hn;             // row length of the LL block; haplotypes of this pass
  int32_t out, sample;       // slot in the pass's sample_total_ll / gts; the sample inside the locus
  double homoz, hetz;        // priors, genotyper.cpp:21-33 (host libm)
};

__device__ __forceinline__ double gt_ll(const double* __restrict__ row, const int32_t* __restrict__ cmap, int a) {
  const int src = cmap ? cmap[a] : a;
  double v = src >= 0 ? row[src] : -100000.0;                   // a haplotype without an old column, seq_stutter_genotyper.cpp:367
  if (v < -600.0) v = -600.0;                                   // genotyper.cpp:57-58
  return v;
}

// Genotyper::calc_log_sample_posteriors + get_optimal_haplotypes (genotyper.cpp:45-100), one workgroup per (locus, sample).
// The locus' reads are staged in tiles (a read of another sample keeps its slot, flagged, and costs nothing more): E1[j][a] = exp(ll + log_p1 + log(1/2)), E2[j][a] likewise, once per read and haplotype
// (2 R H' exponentials, where a loop per diplotype takes 2 R H'^2); thread (a1, a2) then adds log(E1[j][a1] + E2[j][a2]) over the
// tile's reads of the sample in read order, tiles in order, starting from the prior: the operands and the order of ltr_posterior_batch_kernel,
// so the same bits.  LDS rows are H' doubles, unpadded: in the sum every lane reads the same row j -- E2 at H' consecutive
// doubles, E1 at one or two addresses (broadcast) -- and staging writes consecutive doubles.
// An H' x H' block of at most post_cap doubles stays in LDS until it is normalised (log_sum_exp in index order, :67-75,
// mathops.cpp:47-53) and scanned for the first maximum of the NORMALISED values (:85-100); a larger one is accumulated in the
// posterior buffer and finished by ltr_genotype_finish_kernel.  A row that does not fit a tile (H' > tile_doubles) is not
// staged: its diplotype threads take the exponentials themselves.
template <int NT>
__global__ __launch_bounds__(NT) void ltr_genotype_kernel(const GtUnit* __restrict__ units, const double* __restrict__ ll,
                                                          const int32_t* __restrict__ pool_index, const double* __restrict__ lp1,
                                                          const double* __restrict__ lp2, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ map, const int32_t* __restrict__ list,
                                                          int tile_doubles, int post_cap,
                                                          double* __restrict__ post, double* __restrict__ stl, int* __restrict__ gts) {
  extern __shared__ double smem[];
  __shared__ double s_scalar[2];
  double* sE1 = smem;
  double* sE2 = smem + tile_doubles;
  double* sP = smem + 2 * tile_doubles;
  int* sMine = reinterpret_cast<int*>(sP + post_cap);          // [tile_doubles] read j of the tile is the sample's
  const GtUnit u = units[list ? list[blockIdx.x] : (int)blockIdx.x];   // (list: the units of this launch's shape)
  const double LOG_ONE_HALF = -0.6931471805599453094;          // log(0.5), mathops.cpp:10
  const int tid = threadIdx.x, Hn = u.Hn, nd = Hn * Hn;
  const int32_t* cmap = u.map_off >= 0 ? map + u.map_off : nullptr;
  const double* llb = ll + u.ll_off;
  const bool fused = nd <= post_cap;
  double* accp = fused ? sP : post + u.post_off;               // (entry idx is only ever touched by the thread that owns it)
  for (int idx = tid; idx < nd; idx += NT) accp[idx] = (idx / Hn == idx % Hn) ? u.homoz : u.hetz;   // init_log_sample_priors, :35-43
  if (Hn <= tile_doubles) {
    const int TR = tile_doubles / Hn;
    for (int t0 = u.r0; t0 < u.r1; t0 += TR) {
      const int n = min(TR, u.r1 - t0);
      __syncthreads();                                         // the tile before this one has been read
      for (int k = tid; k < n * Hn; k += NT) {
        const int j = k / Hn, a = k - j * Hn;
        const int r = t0 + j;
        const bool mine = label[r] == u.sample;
        if (a == 0) sMine[j] = mine;
        if (!mine) continue;
        const double v = gt_ll(llb + (int64_t)pool_index[r] * u.H, cmap, a);   // the read's pool row (seq_stutter_genotyper.cpp:531-537)
        sE1[k] = exp(v + lp1[r] + LOG_ONE_HALF);
        sE2[k] = exp(v + lp2[r] + LOG_ONE_HALF);
      }
      __syncthreads();
      for (int idx = tid; idx < nd; idx += NT) {
        const int a1 = idx / Hn, a2 = idx - a1 * Hn;
        double acc = accp[idx];
        for (int j = 0; j < n; ++j) if (sMine[j]) acc += log(sE1[j * Hn + a1] + sE2[j * Hn + a2]);   // :59, reads in order like :52-63
        accp[idx] = acc;
      }
    }
  } else {
    for (int idx = tid; idx < nd; idx += NT) {
      const int a1 = idx / Hn, a2 = idx - a1 * Hn;
      double acc = accp[idx];
      for (int r = u.r0; r < u.r1; ++r) {
        if (label[r] != u.sample) continue;
        const double* row = llb + (int64_t)pool_index[r] * u.H;
        acc += log(exp(gt_ll(row, cmap, a1) + lp1[r] + LOG_ONE_HALF) + exp(gt_ll(row, cmap, a2) + lp2[r] + LOG_ONE_HALF));
      }
      accp[idx] = acc;
    }
  }
  if (!fused) return;
  __syncthreads();
  if (tid == 0) {
    double mx = sP[0];
    for (int i = 1; i < nd; ++i) if (mx < sP[i]) mx = sP[i];
    s_scalar[0] = mx;
  }
  __syncthreads();
  {
    const double mx = s_scalar[0];
    for (int idx = tid; idx < nd; idx += NT) smem[idx] = exp(sP[idx] - mx);   // (both E tables are free now: nd <= post_cap <= 2 tile_doubles)
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int i = 0; i < nd; ++i) tot += smem[i];                // index order, like the reference's loop
    const double total = s_scalar[0] + log(tot);
    stl[u.out] = total;
    s_scalar[1] = total;
  }
  __syncthreads();
  {
    const double total = s_scalar[1];
    for (int idx = tid; idx < nd; idx += NT) { const double v = sP[idx] - total; sP[idx] = v; post[u.post_off + idx] = v; }
  }
  __syncthreads();
  if (tid == 0) {
    double best = -1.7976931348623157e308; int b = -1;
    for (int i = 0; i < nd; ++i) if (sP[i] > best) { best = sP[i]; b = i; }   // first maximum, :91-96
    gts[2 * u.out] = b < 0 ? -1 : b / Hn;
    gts[2 * u.out + 1] = b < 0 ? -1 : b % Hn;
  }
}

// normalise + argmax of the units whose H' x H' block did not fit LDS (one thread each; index-ordered sum, first maximum)
__global__ void ltr_genotype_finish_kernel(int n, const int32_t* __restrict__ list, const GtUnit* __restrict__ units,
                                           double* __restrict__ post, double* __restrict__ stl, int* __restrict__ gts) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const GtUnit u = units[list[k]];
  const int Hn = u.Hn, nd = Hn * Hn;
  double* p = post + u.post_off;
  double mx = p[0];
  for (int i = 1; i < nd; ++i) if (mx < p[i]) mx = p[i];
  double tot = 0.0;
  for (int i = 0; i < nd; ++i) tot += exp(p[i] - mx);
  const double total = mx + log(tot);
  stl[u.out] = total;
  double best = -1.7976931348623157e308; int b1 = -1, b2 = -1;
  for (int i = 0; i < nd; ++i) {
    const double v = p[i] - total;
    p[i] = v;
    if (v > best) { best = v; b1 = i / Hn; b2 = i % Hn; }
  }
  gts[2 * u.out] = b1; gts[2 * u.out + 1] = b2;
}

// log_aln_probs_ per READ of every locus: pool rows fanned out to reads (seq_stutter_genotyper.cpp:526-538), the surviving
// columns in their new places (:364-377), clamped like genotyper.cpp:57-58.  One workgroup per locus.
struct GtLocus {
  int64_t ll_off, out_off, map_off;
  int32_t r0, r1, H, Hn;
};
__global__ void ltr_genotype_gather_kernel(const GtLocus* __restrict__ loci, const double* __restrict__ ll,
                                           const int32_t* __restrict__ pool_index, const int32_t* __restrict__ map,
                                           double* __restrict__ out) {
  const GtLocus L = loci[blockIdx.x];
  const int32_t* cmap = L.map_off >= 0 ? map + L.map_off : nullptr;
  const int64_t n = (int64_t)(L.r1 - L.r0) * L.Hn;
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
    const int64_t j = k / L.Hn;
    const int a = (int)(k - j * L.Hn);
    out[L.out_off + k] = gt_ll(ll + L.ll_off + (int64_t)pool_index[L.r0 + j] * L.H, cmap, a);
  }
}

void set_priors(GtUnit* u, int32_t H, int haploid) {
  // int_log(v) == log(v) (mathops.cpp:14-22); priors of genotyper.cpp:21-33
  const double lH = std::log((double)H), lH1 = std::log((double)(H + 1));
  u->homoz = haploid ? -lH : std::log(2.0) - lH - lH1;
  u->hetz = haploid ? -1.7976931348623157e308 / 2 : -lH - lH1;
}

constexpr int kSmallH = 8;              // units of up to 8 haplotypes (64 diplotypes: one wavefront) run in workgroups of 64 threads, the others of 256

// The units of a pass by launch shape: [0] H' <= kSmallH, [1] the others.  Per shape: block size, tile (as large as the largest
// locus of the shape needs, up to kTileMax doubles per table), LDS, the units whose H'^2 block does not fit LDS.
struct LaunchShape { int nt = 64, tile = 64, post_cap = 1; size_t lds = 0, n = 0; std::vector<int32_t> list, unfused; };
struct PassShape {
  LaunchShape sh[2];
  bool one() const { return sh[0].n == 0 || sh[1].n == 0; }    // one shape only: no unit lists needed
};
PassShape shape_of(const GtUnit* units, size_t n_units) {
  PassShape ps;
  int64_t max_nd[2] = {1, 1}, want[2] = {64, 64};
  for (size_t k = 0; k < n_units; ++k) {
    const GtUnit& u = units[k];
    const int g = u.Hn <= kSmallH ? 0 : 1;
    ps.sh[g].n++;
    max_nd[g] = std::max<int64_t>(max_nd[g], (int64_t)u.Hn * u.Hn);
    if (u.Hn <= kTileMax) want[g] = std::max<int64_t>(want[g], std::min<int64_t>((int64_t)std::max(u.r1 - u.r0, 1) * u.Hn, kTileMax));
  }
  const bool one = ps.one();
  for (int g = 0; g < 2; ++g) {
    LaunchShape& s = ps.sh[g];
    s.nt = g == 0 ? 64 : 256;
    s.tile = (int)((want[g] + 63) / 64 * 64);
    s.post_cap = (int)std::min<int64_t>(std::min<int64_t>(max_nd[g], kPostCapMax), 2 * (int64_t)s.tile);
    s.lds = ((size_t)2 * s.tile + s.post_cap) * sizeof(double) + (size_t)s.tile * sizeof(int);
    if (!one) s.list.reserve(s.n);
  }
  for (size_t k = 0; k < n_units; ++k) {
    LaunchShape& s = ps.sh[units[k].Hn <= kSmallH ? 0 : 1];
    if (!one) s.list.push_back((int32_t)k);
    if ((int64_t)units[k].Hn * units[k].Hn > s.post_cap) s.unfused.push_back((int32_t)k);
  }
  return ps;
}

}  // namespace

#define G_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ltr::set_error(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); rc = LTR_ERR_HIP; goto done; } } while (0)

namespace {

// One pass: a launch per shape with units (d_lists: the unit lists of shape 0 then shape 1, or null when there is one shape), then
// the finish kernel over the units whose block did not fit LDS (d_unfused: shape 0's then shape 1's).
void launch_pass(const PassShape& ps, hipStream_t st, const GtUnit* d_units, const double* d_ll, const int32_t* d_pool,
                 const double* d_p1, const double* d_p2, const int32_t* d_label, const int32_t* d_map, const int32_t* d_lists,
                 const int32_t* d_unfused, double* d_post, double* d_stl, int* d_gts) {
  for (int g = 0; g < 2; ++g) {
    const LaunchShape& sh = ps.sh[g];
    if (sh.n == 0) continue;
    const int32_t* list = d_lists ? d_lists + (g == 0 ? 0 : ps.sh[0].n) : nullptr;
    if (g == 0)
      hipLaunchKernelGGL(ltr_genotype_kernel<64>, dim3((unsigned)sh.n), dim3(64), sh.lds, st, d_units, d_ll, d_pool, d_p1, d_p2, d_label, d_map,
                         list, sh.tile, sh.post_cap, d_post, d_stl, d_gts);
    else
      hipLaunchKernelGGL(ltr_genotype_kernel<256>, dim3((unsigned)sh.n), dim3(256), sh.lds, st, d_units, d_ll, d_pool, d_p1, d_p2, d_label, d_map,
                         list, sh.tile, sh.post_cap, d_post, d_stl, d_gts);
  }
  const size_t nf = ps.sh[0].unfused.size() + ps.sh[1].unfused.size();
  if (nf)
    hipLaunchKernelGGL(ltr_genotype_finish_kernel, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, st, (int)nf, d_unfused, d_units, d_post, d_stl, d_gts);
}
// the unit lists / unfused lists of a pass on the device (null: none needed); 0 or a hipError_t
hipError_t upload_lists(ltr_ctx* ctx, hipStream_t st, const PassShape& ps, int32_t** d_alloc, const int32_t** d_lists, const int32_t** d_unf, std::vector<int32_t>* stage) {
  *d_lists = nullptr; *d_unf = nullptr;
  stage->clear();
  if (!ps.one()) { stage->insert(stage->end(), ps.sh[0].list.begin(), ps.sh[0].list.end()); stage->insert(stage->end(), ps.sh[1].list.begin(), ps.sh[1].list.end()); }
  const size_t nlist = stage->size();
  stage->insert(stage->end(), ps.sh[0].unfused.begin(), ps.sh[0].unfused.end());
  stage->insert(stage->end(), ps.sh[1].unfused.begin(), ps.sh[1].unfused.end());
  if (stage->empty()) return hipSuccess;
  hipError_t e = ctx->pool.alloc((void**)d_alloc, stage->size() * 4);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(*d_alloc, stage->data(), stage->size() * 4, hipMemcpyHostToDevice, st);   // (pageable: staged before the call returns)
  if (nlist) *d_lists = *d_alloc;
  *d_unf = *d_alloc + nlist;
  return e;
}

}  // namespace

// ltr_plan_genotype (fr == null) and ltr_plan_genotype_fields: the same passes; with fr the fields kernel runs on their
// buffers before they go back to the pool, and the posterior blocks are fetched only when fr asks for them.
static int plan_genotype(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result** out) {
  if (out) *out = nullptr;
  if (!plan || !gb || !gb->pb || !out) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  const ltr_posterior_batch* pb = gb->pb;
  if (!plan->executed) { ltr::set_error(ctx, "ltr_plan_genotype: execute the plan first"); return LTR_ERR_INVALID; }
  const int64_t nl = pb->n_loci;
  if (nl != (int64_t)plan->locus_P.size()) { ltr::set_error(ctx, "genotype batch and plan disagree on the number of loci"); return LTR_ERR_INVALID; }
  if (!gb->haps && nl > 0 && (gb->prune || fr)) { ltr::set_error(ctx, "ltr_plan_genotype: no haplotype blocks"); return LTR_ERR_INVALID; }
  const bool need_haps = gb->prune || fr, fetch_post = !fr || fr->want_posteriors;
  if (nl > 0 && (!pb->locus_read_off || !pb->n_samples || (pb->n_reads > 0 && (!pb->pool_index || !pb->log_p1 || !pb->log_p2 || !pb->sample_label)))) {
    ltr::set_error(ctx, "ltr_plan_genotype: incomplete posterior batch"); return LTR_ERR_INVALID;
  }
  ltr::TimedCall timed(ctx, ltr::kTimerPosterior);             // total_posterior_time_, genotyper.cpp:46,:80-81
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<ltr_genotype_result> res(new ltr_genotype_result());
  res->n_loci = nl;
  res->S.assign(pb->n_samples, pb->n_samples + nl);
  res->H.assign(plan->locus_H.begin(), plan->locus_H.end());
  if (gb->haps) res->haps.assign(gb->haps, gb->haps + nl); else res->haps.assign((size_t)nl, nullptr);
  res->unit_off.assign((size_t)nl + 1, 0); res->post1_off.assign((size_t)nl + 1, 0);
  res->pruned.resize((size_t)nl); res->n_blocks.assign((size_t)nl, 0);
  std::vector<int64_t> pool_base((size_t)nl + 1, 0);          // first pool (= read of the plan) of every locus
  int32_t max_H = 1;
  for (int64_t l = 0; l < nl; ++l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1];
    const int32_t S = pb->n_samples[l], H = plan->locus_H[(size_t)l];
    if (r0 < 0 || r1 < r0 || r1 > pb->n_reads || S < 0 || r1 > 0x7fffffff) { ltr::set_error(ctx, "bad posterior batch offsets"); return LTR_ERR_INVALID; }
    if (H <= 0) { ltr::set_error(ctx, "ltr_plan_genotype: a locus without haplotypes"); return LTR_ERR_INVALID; }
    res->unit_off[(size_t)l + 1] = res->unit_off[(size_t)l] + S;
    res->post1_off[(size_t)l + 1] = res->post1_off[(size_t)l] + (int64_t)S * H * H;
    pool_base[(size_t)l + 1] = pool_base[(size_t)l] + plan->locus_P[(size_t)l];
    max_H = std::max(max_H, H);
  }
  const size_t nu = (size_t)res->unit_off[(size_t)nl], nr = (size_t)pb->n_reads;
  res->identity.resize((size_t)max_H);
  for (int32_t k = 0; k < max_H; ++k) res->identity[(size_t)k] = k;
  res->stl.assign(nu, 0.0); res->gts.assign(2 * nu, -1);

  // ---- host, all loci at once: labels checked, every sample's reads listed in read order, aligned_read (:262-266) ----
  LTR_DBG("genotype: %ld loci checked", (long)nl);
  ctx->gt_units.resize(nu * sizeof(GtUnit));                  // (kept by the context: 13 MB of fresh pages per call on a catalogue otherwise)
  GtUnit* units = reinterpret_cast<GtUnit*>(ctx->gt_units.p);
  std::vector<uint8_t> aligned(nu, 0);
  std::atomic<int> bad(0);
  std::atomic<int64_t> bad_haps(-1), bad_block(-1);
  if (fr) { res->has_fields = true; res->ctx = ctx; res->haploid = pb->haploid ? 1 : 0; res->f_block.assign((size_t)nl, 0); res->f_V.assign((size_t)nl, 0); }
  ltr::parallel_for(nl, 64, [&](int64_t l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1], u0 = res->unit_off[(size_t)l];
    const int32_t S = pb->n_samples[l], H = plan->locus_H[(size_t)l], P = plan->locus_P[(size_t)l];
    if (need_haps) {     // (prune == 0 never reads the block lists: 100 000 of them scattered over the caller's heap cost 2 ms of cache misses)
      if (!gb->haps[l] || ltr_haplotype_num_combs(gb->haps[l]) != H) { bad_haps.store(l); return; }
      res->n_blocks[(size_t)l] = gb->haps[l]->n_blocks;
    }
    if (fr) {            // the block of the record: pruning keeps the blocks, so the caller's list tells
      const ltr_haplotype_blocks* hb = gb->haps[l];
      int32_t b = fr->block ? fr->block[l] : 0;
      if (!fr->block) while (b < hb->n_blocks && !hb->is_repeat[b]) ++b;
      if (b < 0 || b >= hb->n_blocks) { bad_block.store(l); return; }
      res->f_block[(size_t)l] = b;
    }
    for (int64_t r = r0; r < r1; ++r) {
      const int32_t q = pb->pool_index[r], s = pb->sample_label[r];
      if (q < 0 || q >= P || s < 0 || s >= S) { bad.store(1); return; }
      if (plan->seed[(size_t)(pool_base[(size_t)l] + q)] >= 0) aligned[(size_t)(u0 + s)] = 1;     // seed_positions_[read] >= 0, :265
    }
    for (int32_t s = 0; s < S; ++s) {
      GtUnit& u = units[(size_t)(u0 + s)];
      u.ll_off = plan->locus_ll_off[(size_t)l]; u.post_off = res->post1_off[(size_t)l] + (int64_t)s * H * H; u.map_off = -1;
      u.r0 = (int32_t)r0; u.r1 = (int32_t)r1;
      u.H = H; u.Hn = H; u.out = (int32_t)(u0 + s); u.sample = s;
      set_priors(&u, H, pb->haploid);
    }
  });
  if (bad_haps.load() >= 0) {
    const int64_t l = bad_haps.load();
    ltr::set_error(ctx, "haplotype blocks of locus " + std::to_string(l) + " do not enumerate the plan's " + std::to_string(plan->locus_H[(size_t)l]) + " haplotypes");
    return LTR_ERR_INVALID;
  }
  if (bad_block.load() >= 0) {
    ltr::set_error(ctx, "ltr_plan_genotype_fields: locus " + std::to_string(bad_block.load()) + (fr->block ? ": block out of range" : ": no repeat block"));
    return LTR_ERR_INVALID;
  }
  if (bad.load()) { ltr::set_error(ctx, "pool index / sample label out of range"); return LTR_ERR_INVALID; }
  if (nu == 0) {                                               // (no sample anywhere: nothing to compute; read_ll stays NULL)
    if (fr) {
      res->f_gl_off.assign((size_t)nl + 1, 0); res->f_pgl_off.assign((size_t)nl + 1, 0);
      res->f_read_off.assign(pb->locus_read_off, pb->locus_read_off + nl + 1);
      for (int64_t l = 0; l < nl; ++l) res->f_V[(size_t)l] = gb->haps[l]->n_alleles[res->f_block[(size_t)l]];
      res->f_i32.reset(new int32_t[std::max<size_t>(nr, 1)]()); res->f_f64.reset(new double[1]());
    }
    *out = res.release(); return LTR_OK;
  }

  const int64_t npost1 = res->post1_off[(size_t)nl];
  if (fetch_post) res->post1.reset(new double[(size_t)std::max<int64_t>(npost1, 1)]);
  const PassShape sh1 = shape_of(units, nu);
  LTR_DBG("genotype: %zu units laid out", nu);
  GtUnit *d_units = nullptr, *d_units2 = nullptr; GtLocus* d_loci = nullptr;
  int32_t *d_pool = nullptr, *d_label = nullptr, *d_map = nullptr, *d_lists1 = nullptr, *d_lists2 = nullptr; int *d_gts = nullptr, *d_gts2 = nullptr;
  const int32_t *d_list = nullptr, *d_unf = nullptr;
  std::vector<int32_t> stage;
  double *d_p1 = nullptr, *d_p2 = nullptr, *d_post = nullptr, *d_stl = nullptr, *d_post2 = nullptr, *d_stl2 = nullptr, *d_rll = nullptr;
  ltrf::FieldUnit* d_funits = nullptr; ltrf::FieldLocus* d_floci = nullptr; int32_t *d_ftab = nullptr, *d_fi32 = nullptr, *d_fpls = nullptr;
  double *d_ff64 = nullptr, *d_fgls = nullptr, *d_fpgls = nullptr, *d_fcells = nullptr;
  std::vector<ltrf::FieldUnit> funits; std::vector<ltrf::FieldLocus> floci; std::vector<int32_t> ftab;
  int rc = LTR_OK;
  hipStream_t st = plan->last_stream;
  std::vector<GtUnit> units2; std::vector<int32_t> map; std::vector<GtLocus> gl; std::vector<int64_t> affected;
  std::vector<double> stl2; std::vector<int32_t> gts2;
  PassShape sh2;
  int64_t npost2 = 0;
  G_TRY(ctx->pool.alloc((void**)&d_units, nu * sizeof(GtUnit)));
  G_TRY(ctx->pool.alloc((void**)&d_pool, std::max<size_t>(nr, 1) * 4));
  G_TRY(ctx->pool.alloc((void**)&d_label, std::max<size_t>(nr, 1) * 4));
  G_TRY(ctx->pool.alloc((void**)&d_p1, std::max<size_t>(nr, 1) * 8));
  G_TRY(ctx->pool.alloc((void**)&d_p2, std::max<size_t>(nr, 1) * 8));
  G_TRY(ctx->pool.alloc((void**)&d_post, (size_t)std::max<int64_t>(npost1, 1) * 8));
  G_TRY(ctx->pool.alloc((void**)&d_stl, nu * 8));
  G_TRY(ctx->pool.alloc((void**)&d_gts, nu * 8));
  G_TRY(hipMemcpyAsync(d_units, units, nu * sizeof(GtUnit), hipMemcpyHostToDevice, st));
  if (nr) {
    G_TRY(hipMemcpyAsync(d_pool, pb->pool_index, nr * 4, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(d_label, pb->sample_label, nr * 4, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(d_p1, pb->log_p1, nr * 8, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(d_p2, pb->log_p2, nr * 8, hipMemcpyHostToDevice, st));
  }
  G_TRY(upload_lists(ctx, st, sh1, &d_lists1, &d_list, &d_unf, &stage));
  // ---- first pass: calc_log_sample_posteriors + get_optimal_haplotypes, :635 ----
  launch_pass(sh1, st, d_units, plan->last_out, d_pool, d_p1, d_p2, d_label, nullptr, d_list, d_unf, d_post, d_stl, d_gts);
  G_TRY(hipGetLastError());
  G_TRY(hipMemcpyAsync(res->gts.data(), d_gts, nu * 8, hipMemcpyDeviceToHost, st));
  G_TRY(hipMemcpyAsync(res->stl.data(), d_stl, nu * 8, hipMemcpyDeviceToHost, st));
  LTR_DBG("genotype: first pass queued");
  G_TRY(hipStreamSynchronize(st));                             // (the host needs the best pairs; the posterior blocks follow below)
  LTR_DBG("genotype: first pass done");
  if (fetch_post) G_TRY(hipMemcpyAsync(res->post1.get(), d_post, (size_t)npost1 * 8, hipMemcpyDeviceToHost, st));

  LTR_DBG("genotype: first posteriors fetched");
  // ---- between the passes (host, all loci at once): get_unused_alleles (:250-308), the new block lists and column maps ----
  if (gb->prune) {
    std::atomic<int> perr(0);
    ltr::parallel_for(nl, 64, [&](int64_t l) {
      const ltr_haplotype_blocks* hb = gb->haps[l];
      const int nb = hb->n_blocks;
      const int32_t S = res->S[(size_t)l], H = res->H[(size_t)l];
      if (H == 1) return;                                      // every block has one option, :274
      const int64_t u0 = res->unit_off[(size_t)l];
      std::vector<int32_t> counts; int64_t nc = 0;
      if (ltr::haplotype_counts(hb, &counts, &nc) != LTR_OK || nc != H) { perr.store(1); return; }
      std::vector<std::vector<int32_t>> removed((size_t)nb);
      int32_t aff_blocks = 0, aff_alleles = 0;
      for (int b = 0; b < nb; ++b) {
        const int n = hb->n_alleles[b];
        if (n == 1) continue;                                  // :274
        std::vector<uint8_t> called((size_t)n, 0);
        for (int32_t s = 0; s < S; ++s) {
          if (!aligned[(size_t)(u0 + s)] || (gb->sample_filtered && gb->sample_filtered[u0 + s])) continue;   // :289
          const int32_t g1 = res->gts[(size_t)(2 * (u0 + s))], g2 = res->gts[(size_t)(2 * (u0 + s) + 1)];
          if (g1 < 0 || g1 >= H || g2 < 0 || g2 >= H) { perr.store(2); return; }
          called[(size_t)counts[(size_t)((int64_t)g1 * nb + b)]] = 1;        // haps_to_alleles, :240-248, :290-291
          called[(size_t)counts[(size_t)((int64_t)g2 * nb + b)]] = 1;
        }
        for (int a = 1; a < n; ++a) if (!called[(size_t)a]) { removed[(size_t)b].push_back(a); ++aff_alleles; }   // :298-304
        if (!removed[(size_t)b].empty()) ++aff_blocks;
      }
      if (aff_alleles == 0) return;                            // :641
      std::unique_ptr<LtrPruned> p(new LtrPruned());
      if (ltr::prune_hap_blocks(hb, removed, &p->blocks) != LTR_OK || ltr::remap_haplotypes(hb, &p->blocks.view, &p->allele_mapping, nullptr) != LTR_OK) {
        perr.store(1); return;
      }
      p->Hn = (int32_t)ltr_haplotype_num_combs(&p->blocks.view);
      p->new_to_old.assign((size_t)p->Hn, -1);
      for (int32_t j = 0; j < H; ++j) if (p->allele_mapping[(size_t)j] >= 0) p->new_to_old[(size_t)p->allele_mapping[(size_t)j]] = j;
      p->removed.swap(removed); p->aff_blocks = aff_blocks; p->aff_alleles = aff_alleles;
      res->pruned[(size_t)l] = std::move(p);
    }, 16);
    if (perr.load()) {
      ltr::set_error(ctx, perr.load() == 2 ? "ltr_plan_genotype: a sample without an optimal haplotype pair (NaN scores?)" : "ltr_plan_genotype: malformed haplotype blocks");
      rc = LTR_ERR_INVALID; goto done;
    }
    for (int64_t l = 0; l < nl; ++l) {
      LtrPruned* p = res->pruned[(size_t)l].get();
      if (!p) continue;
      const int32_t S = res->S[(size_t)l];
      const int64_t map_off = (int64_t)map.size();
      map.insert(map.end(), p->new_to_old.begin(), p->new_to_old.end());
      p->post_off = npost2;
      for (int32_t s = 0; s < S; ++s) {
        GtUnit u = units[(size_t)(res->unit_off[(size_t)l] + s)];
        u.post_off = npost2 + (int64_t)s * p->Hn * p->Hn; u.map_off = map_off; u.Hn = p->Hn; u.out = (int32_t)units2.size();
        set_priors(&u, p->Hn, pb->haploid);                    // :405-408: priors of the new number of haplotypes
        units2.push_back(u);
      }
      npost2 += (int64_t)S * p->Hn * p->Hn;
      affected.push_back(l);
    }
  }
  LTR_DBG("genotype: %zu loci pruned", affected.size());
  // ---- second pass, the loci that lost alleles only: calc_log_sample_posteriors of add_and_remove_alleles, :405-408 ----
  if (!map.empty()) {
    G_TRY(ctx->pool.alloc((void**)&d_map, map.size() * 4));
    G_TRY(hipMemcpyAsync(d_map, map.data(), map.size() * 4, hipMemcpyHostToDevice, st));
  }
  if (!units2.empty()) {
    const size_t nu2 = units2.size();
    sh2 = shape_of(units2.data(), nu2);
    if (fetch_post) res->post2.reset(new double[(size_t)std::max<int64_t>(npost2, 1)]);
    stl2.resize(nu2); gts2.resize(2 * nu2);
    G_TRY(ctx->pool.alloc((void**)&d_units2, nu2 * sizeof(GtUnit)));
    G_TRY(ctx->pool.alloc((void**)&d_post2, (size_t)std::max<int64_t>(npost2, 1) * 8));
    G_TRY(ctx->pool.alloc((void**)&d_stl2, nu2 * 8));
    G_TRY(ctx->pool.alloc((void**)&d_gts2, nu2 * 8));
    G_TRY(hipMemcpyAsync(d_units2, units2.data(), nu2 * sizeof(GtUnit), hipMemcpyHostToDevice, st));
    G_TRY(upload_lists(ctx, st, sh2, &d_lists2, &d_list, &d_unf, &stage));
    launch_pass(sh2, st, d_units2, plan->last_out, d_pool, d_p1, d_p2, d_label, d_map, d_list, d_unf, d_post2, d_stl2, d_gts2);
    G_TRY(hipGetLastError());
    if (fetch_post) G_TRY(hipMemcpyAsync(res->post2.get(), d_post2, (size_t)npost2 * 8, hipMemcpyDeviceToHost, st));
    G_TRY(hipMemcpyAsync(stl2.data(), d_stl2, nu2 * 8, hipMemcpyDeviceToHost, st));
    G_TRY(hipMemcpyAsync(gts2.data(), d_gts2, nu2 * 8, hipMemcpyDeviceToHost, st));
  }
  // ---- log_aln_probs_ per read in the final columns ----
  if (gb->want_read_ll) {
    gl.resize((size_t)nl);
    res->read_ll_off.assign((size_t)nl + 1, 0);
    int64_t mo = 0;
    for (int64_t l = 0; l < nl; ++l) {
      const LtrPruned* p = res->pruned[(size_t)l].get();
      GtLocus& g = gl[(size_t)l];
      g.ll_off = plan->locus_ll_off[(size_t)l]; g.out_off = res->read_ll_off[(size_t)l]; g.map_off = p ? mo : -1;
      g.r0 = (int32_t)pb->locus_read_off[l]; g.r1 = (int32_t)pb->locus_read_off[l + 1]; g.H = res->H[(size_t)l]; g.Hn = p ? p->Hn : g.H;
      if (p) mo += p->Hn;
      res->read_ll_off[(size_t)l + 1] = g.out_off + (int64_t)(g.r1 - g.r0) * g.Hn;
    }
    const int64_t nrll = res->read_ll_off[(size_t)nl];
    res->read_ll.reset(new double[(size_t)std::max<int64_t>(nrll, 1)]);
    G_TRY(ctx->pool.alloc((void**)&d_loci, (size_t)nl * sizeof(GtLocus)));
    G_TRY(ctx->pool.alloc((void**)&d_rll, (size_t)std::max<int64_t>(nrll, 1) * 8));
    G_TRY(hipMemcpyAsync(d_loci, gl.data(), (size_t)nl * sizeof(GtLocus), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ltr_genotype_gather_kernel, dim3((unsigned)nl), dim3(64), 0, st, d_loci, plan->last_out, d_pool, d_map, d_rll);
    G_TRY(hipGetLastError());
    if (nrll) G_TRY(hipMemcpyAsync(res->read_ll.get(), d_rll, (size_t)nrll * 8, hipMemcpyDeviceToHost, st));
  }
  // ---- the VCF fields of every locus (ltr_plan_fields.hip), on the final posterior blocks where they lie ----
  if (fr) {
    res->f_gl_off.assign((size_t)nl + 1, 0); res->f_pgl_off.assign((size_t)nl + 1, 0);
    res->f_read_off.assign(pb->locus_read_off, pb->locus_read_off + nl + 1);
    floci.resize((size_t)nl);
    std::vector<int64_t> unit2_off((size_t)nl, -1);             // first unit of a pruned locus in the second pass
    { int64_t k = 0; for (int64_t l : affected) { unit2_off[(size_t)l] = k; k += res->S[(size_t)l]; } }
    int64_t tab = 0, mo = 0;
    for (int64_t l = 0; l < nl; ++l) {                           // sizes and offsets (the block lists are warm from the checks above)
      const LtrPruned* p = res->pruned[(size_t)l].get();
      const ltr_haplotype_blocks* hb = p ? &p->blocks.view : gb->haps[l];
      ltrf::FieldLocus& F = floci[(size_t)l];
      const int32_t S = res->S[(size_t)l], H = res->H[(size_t)l], Hn = p ? p->Hn : H, V = hb->n_alleles[res->f_block[(size_t)l]];
      res->f_V[(size_t)l] = V;
      F.ll_off = plan->locus_ll_off[(size_t)l]; F.map_off = p ? mo : -1; F.tab_off = tab;
      F.gl_off = res->f_gl_off[(size_t)l]; F.pgl_off = res->f_pgl_off[(size_t)l];
      F.r0 = (int32_t)pb->locus_read_off[l]; F.r1 = (int32_t)pb->locus_read_off[l + 1]; F.H = H; F.Hn = Hn; F.V = V; F.haploid = pb->haploid ? 1 : 0;
      F.n_gl = pb->haploid ? V : V * (V + 1) / 2; F.n_pgl = pb->haploid ? V : V * V;
      // priors (genotyper.cpp:21-33; the heterozygous one of a haploid call is 0, :210) and configuration terms (:204-241) as ltr_genotype.cpp:108-111
      const double lH = std::log((double)Hn), lH1 = std::log((double)(Hn + 1)), lV = std::log((double)V), l2 = std::log(2.0);
      const double hom_prior = pb->haploid ? -lH : l2 - lH - lH1, het_prior = pb->haploid ? 0.0 : -lH - lH1;
      const double gl_cfg = pb->haploid ? l2 + lH - lV : l2 + 2 * (lH - lV), pgl_cfg = pb->haploid ? lH - lV : 2 * (lH - lV);
      F.hom_gl = hom_prior + gl_cfg; F.het_gl = het_prior + gl_cfg; F.hom_pgl = hom_prior + pgl_cfg; F.het_pgl = het_prior + pgl_cfg;
      if (p) mo += p->Hn;
      tab += 2 * (int64_t)Hn + V + 1;
      res->f_gl_off[(size_t)l + 1] = F.gl_off + (int64_t)S * F.n_gl;
      res->f_pgl_off[(size_t)l + 1] = F.pgl_off + (int64_t)S * F.n_pgl;
    }
    ftab.resize((size_t)tab);
    std::atomic<int> ferr(0);
    ltr::parallel_for(nl, 64, [&](int64_t l) {                   // haps_to_alleles of the FINAL list (:240-248) and the haplotypes of every allele
      const LtrPruned* p = res->pruned[(size_t)l].get();
      const ltr_haplotype_blocks* hb = p ? &p->blocks.view : gb->haps[l];
      const ltrf::FieldLocus& F = floci[(size_t)l];
      std::vector<int32_t> counts; int64_t nc = 0;
      if (ltr::haplotype_counts(hb, &counts, &nc) != LTR_OK || nc != F.Hn) { ferr.store(1); return; }
      int32_t* h2a = ftab.data() + F.tab_off; int32_t* first = h2a + F.Hn; int32_t* list = first + F.V + 1;
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
    if (ferr.load()) { ltr::set_error(ctx, "ltr_plan_genotype_fields: malformed haplotype blocks"); rc = LTR_ERR_INVALID; goto done; }
    // units: those of up to kFieldSmallH haplotypes first (one wavefront each), then the others; a V x V table beyond LDS goes to a workspace
    funits.resize(nu);
    size_t n_small = 0;
    int64_t ncells = 0; int cap_small = 1, cap_large = 1;
    for (int64_t l = 0; l < nl; ++l) if (floci[(size_t)l].Hn <= ltrf::kFieldSmallH) n_small += (size_t)res->S[(size_t)l];
    {
      size_t ks = 0, kl = n_small;
      for (int64_t l = 0; l < nl; ++l) {
        const LtrPruned* p = res->pruned[(size_t)l].get();
        const ltrf::FieldLocus& F = floci[(size_t)l];
        const bool small = F.Hn <= ltrf::kFieldSmallH;
        const int64_t vv = (int64_t)F.V * F.V;
        for (int32_t s = 0; s < res->S[(size_t)l]; ++s) {
          ltrf::FieldUnit& u = funits[small ? ks++ : kl++];
          u.locus = (int32_t)l; u.sample = s; u.out = (int32_t)(res->unit_off[(size_t)l] + s);
          u.pass = p ? 1 : 0; u.src = p ? (int32_t)(unit2_off[(size_t)l] + s) : u.out;
          u.post_off = (p ? p->post_off : res->post1_off[(size_t)l]) + (int64_t)s * F.Hn * F.Hn;
          if (vv > ltrf::kFieldCellCap) { u.cell_off = ncells; ncells += vv; }
          else { u.cell_off = -1; int& cap = small ? cap_small : cap_large; cap = std::max(cap, (int)vv); }
        }
      }
    }
    const int64_t ngl = res->f_gl_off[(size_t)nl], npgl = res->f_pgl_off[(size_t)nl];
    const size_t ni32 = 6 * nu + nr;
    res->f_i32.reset(new int32_t[ni32]); res->f_f64.reset(new double[5 * nu]);
    if (fr->want_gls) res->f_gls.reset(new double[(size_t)std::max<int64_t>(ngl, 1)]);
    if (fr->want_pls) res->f_pls.reset(new int32_t[(size_t)std::max<int64_t>(ngl, 1)]);
    if (fr->want_phased_gls) res->f_pgls.reset(new double[(size_t)std::max<int64_t>(npgl, 1)]);
    G_TRY(ctx->pool.alloc((void**)&d_funits, nu * sizeof(ltrf::FieldUnit)));
    G_TRY(ctx->pool.alloc((void**)&d_floci, (size_t)nl * sizeof(ltrf::FieldLocus)));
    G_TRY(ctx->pool.alloc((void**)&d_ftab, ftab.size() * 4));
    G_TRY(ctx->pool.alloc((void**)&d_fi32, ni32 * 4));
    G_TRY(ctx->pool.alloc((void**)&d_ff64, 5 * nu * 8));
    G_TRY(ctx->pool.alloc((void**)&d_fgls, (size_t)std::max<int64_t>(ngl, 1) * 8));
    if (fr->want_pls) G_TRY(ctx->pool.alloc((void**)&d_fpls, (size_t)std::max<int64_t>(ngl, 1) * 4));
    if (fr->want_phased_gls) G_TRY(ctx->pool.alloc((void**)&d_fpgls, (size_t)std::max<int64_t>(npgl, 1) * 8));
    if (ncells) G_TRY(ctx->pool.alloc((void**)&d_fcells, (size_t)ncells * 8));
    G_TRY(hipMemcpyAsync(d_funits, funits.data(), nu * sizeof(ltrf::FieldUnit), hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(d_floci, floci.data(), (size_t)nl * sizeof(ltrf::FieldLocus), hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(d_ftab, ftab.data(), ftab.size() * 4, hipMemcpyHostToDevice, st));
    // a unit without an optimal pair (best_gts = -1) writes nothing else: its numbers read 0, not what the pool held before
    G_TRY(hipMemsetAsync(d_fi32, 0, 6 * nu * 4, st));
    G_TRY(hipMemsetAsync(d_ff64, 0, 5 * nu * 8, st));
    if (ngl) G_TRY(hipMemsetAsync(d_fgls, 0, (size_t)ngl * 8, st));
    if (fr->want_pls && ngl) G_TRY(hipMemsetAsync(d_fpls, 0, (size_t)ngl * 4, st));
    if (fr->want_phased_gls && npgl) G_TRY(hipMemsetAsync(d_fpgls, 0, (size_t)npgl * 8, st));
    if (nr) G_TRY(hipMemsetAsync(d_fi32 + 6 * nu, 0xff, nr * 4, st));   // (a read whose label no unit claims cannot exist: the labels were checked; -1 would be refused by the formatter)
    {
      ltrf::FieldArgs a;
      a.units = d_funits; a.loci = d_floci; a.tab = d_ftab;
      a.ll = plan->last_out; a.pool_index = d_pool; a.lp1 = d_p1; a.lp2 = d_p2; a.label = d_label; a.map = d_map;
      a.post[0] = d_post; a.post[1] = d_post2; a.stl[0] = d_stl; a.stl[1] = d_stl2; a.gts[0] = d_gts; a.gts[1] = d_gts2;
      a.best_gts = d_fi32; a.counts = d_fi32 + 2 * nu; a.scalars = d_ff64; a.nu = (int64_t)nu;
      a.gls = d_fgls; a.pls = d_fpls; a.pgls = d_fpgls; a.cells = d_fcells; a.read_allele = d_fi32 + 6 * nu;
      ltrf::launch_fields(st, a, n_small, cap_small, nu - n_small, cap_large);
    }
    G_TRY(hipGetLastError());
    G_TRY(hipMemcpyAsync(res->f_i32.get(), d_fi32, ni32 * 4, hipMemcpyDeviceToHost, st));
    G_TRY(hipMemcpyAsync(res->f_f64.get(), d_ff64, 5 * nu * 8, hipMemcpyDeviceToHost, st));
    if (fr->want_gls && ngl) G_TRY(hipMemcpyAsync(res->f_gls.get(), d_fgls, (size_t)ngl * 8, hipMemcpyDeviceToHost, st));
    if (fr->want_pls && ngl) G_TRY(hipMemcpyAsync(res->f_pls.get(), d_fpls, (size_t)ngl * 4, hipMemcpyDeviceToHost, st));
    if (fr->want_phased_gls && npgl) G_TRY(hipMemcpyAsync(res->f_pgls.get(), d_fpgls, (size_t)npgl * 8, hipMemcpyDeviceToHost, st));
  }
  G_TRY(hipStreamSynchronize(st));
  LTR_DBG("genotype: second pass and gather done");
  {                                                            // the pruned loci's totals and best pairs replace the first pass's
    size_t k = 0;
    for (int64_t l : affected) {
      const int32_t S = res->S[(size_t)l];
      const int64_t u0 = res->unit_off[(size_t)l];
      for (int32_t s = 0; s < S; ++s, ++k) {
        res->stl[(size_t)(u0 + s)] = stl2[k];
        res->gts[(size_t)(2 * (u0 + s))] = gts2[2 * k]; res->gts[(size_t)(2 * (u0 + s) + 1)] = gts2[2 * k + 1];
      }
    }
  }
done:
  if (rc != LTR_OK) (void)hipStreamSynchronize(st);            // (buffers go back to the context's pool: nothing may still use them)
  for (void* p : {(void*)d_units, (void*)d_units2, (void*)d_loci, (void*)d_pool, (void*)d_label, (void*)d_map, (void*)d_lists1, (void*)d_lists2,
                  (void*)d_gts, (void*)d_gts2, (void*)d_p1, (void*)d_p2, (void*)d_post, (void*)d_stl, (void*)d_post2, (void*)d_stl2, (void*)d_rll,
                  (void*)d_funits, (void*)d_floci, (void*)d_ftab, (void*)d_fi32, (void*)d_fpls, (void*)d_ff64, (void*)d_fgls, (void*)d_fpgls, (void*)d_fcells})
    ctx->pool.release(p);
  if (rc == LTR_OK) *out = res.release();
  return rc;
  LTR_GUARD_END(ctx)
}

extern "C" {

int ltr_plan_genotype(ltr_plan* plan, const ltr_genotype_batch* gb, ltr_genotype_result** out) { return plan_genotype(plan, gb, nullptr, out); }
int ltr_plan_genotype_fields(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result** out) {
  if (out) *out = nullptr;
  if (!fr) return LTR_ERR_INVALID;
  return plan_genotype(plan, gb, fr, out);
}

void ltr_genotype_result_free(ltr_genotype_result* r) { delete r; }

#define GT_LOCUS(r, l, fail) if (!(r) || (l) < 0 || (l) >= (r)->n_loci) return fail
int64_t ltr_genotype_result_n_loci(const ltr_genotype_result* r) { return r ? r->n_loci : LTR_ERR_INVALID; }
int32_t ltr_genotype_result_n_haps(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  return r->pruned[(size_t)l] ? r->pruned[(size_t)l]->Hn : r->H[(size_t)l];
}
const int32_t* ltr_genotype_result_new_to_old(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->pruned[(size_t)l] ? r->pruned[(size_t)l]->new_to_old.data() : r->identity.data();
}
const int32_t* ltr_genotype_result_allele_mapping(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->pruned[(size_t)l] ? r->pruned[(size_t)l]->allele_mapping.data() : r->identity.data();
}
int32_t ltr_genotype_result_removed(const ltr_genotype_result* r, int64_t l, int32_t block, const int32_t** alleles) {
  if (alleles) *alleles = nullptr;
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  const LtrPruned* p = r->pruned[(size_t)l].get();
  if (!p) return block < 0 ? LTR_ERR_INVALID : 0;
  if (block < 0 || block >= r->n_blocks[(size_t)l]) return LTR_ERR_INVALID;
  if (!p || p->removed[(size_t)block].empty()) return 0;
  if (alleles) *alleles = p->removed[(size_t)block].data();
  return (int32_t)p->removed[(size_t)block].size();
}
int32_t ltr_genotype_result_num_aff_blocks(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  return r->pruned[(size_t)l] ? r->pruned[(size_t)l]->aff_blocks : 0;
}
int32_t ltr_genotype_result_num_aff_alleles(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  return r->pruned[(size_t)l] ? r->pruned[(size_t)l]->aff_alleles : 0;
}
const ltr_haplotype_blocks* ltr_genotype_result_blocks(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->pruned[(size_t)l] ? &r->pruned[(size_t)l]->blocks.view : r->haps[(size_t)l];
}
const double* ltr_genotype_result_log_sample_posteriors(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  if (!r->post1) return nullptr;                               // (ltr_plan_genotype_fields without want_posteriors)
  return r->pruned[(size_t)l] ? r->post2.get() + r->pruned[(size_t)l]->post_off : r->post1.get() + r->post1_off[(size_t)l];
}
const double* ltr_genotype_result_sample_total_ll(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->stl.data() + r->unit_off[(size_t)l];
}
const int32_t* ltr_genotype_result_gts(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->gts.data() + 2 * r->unit_off[(size_t)l];
}
const double* ltr_genotype_result_read_ll(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, nullptr);
  return r->read_ll ? r->read_ll.get() + r->read_ll_off[(size_t)l] : nullptr;
}

}  // extern "C"
