// ltr_plan_genotype.hip -- SeqStutterGenotyper::genotype after the alignment (reference seq_stutter_genotyper.cpp:632-645) for
// every locus of an executed plan: posteriors (genotyper.cpp:21-100), get_unused_alleles (:250-308), remove_alleles ->
// add_and_remove_alleles (:317-409) and the posteriors over the smaller haplotype set (:405-408).
// Device: the posterior arithmetic of both passes and the per-read column gather.  Host (worker pool): the integer bookkeeping
// between the passes, from the first pass's best pairs.

#include <cmath>
#include <cstring>
#include <memory>

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
// DIRECT: the row rule of the LL source (LlSource): false = a read's row is its pool's (pool_index), true = its own (r - r0; pool_index null).
template <int NT, bool DIRECT>
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
        const double v = ltr_clamped_ll(llb + (DIRECT ? (int64_t)(r - u.r0) : (int64_t)pool_index[r]) * u.H, cmap, a);   // the read's pool row (seq_stutter_genotyper.cpp:531-537), or its own
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
        const double* row = llb + (DIRECT ? (int64_t)(r - u.r0) : (int64_t)pool_index[r]) * u.H;
        acc += log(exp(ltr_clamped_ll(row, cmap, a1) + lp1[r] + LOG_ONE_HALF) + exp(ltr_clamped_ll(row, cmap, a2) + lp2[r] + LOG_ONE_HALF));
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
  ltr_normalise_argmax(post + u.post_off, u.Hn, stl, gts, u.out);
}

// log_aln_probs_ per READ of every locus: pool rows fanned out to reads (seq_stutter_genotyper.cpp:526-538), the surviving
// columns in their new places (:364-377), clamped like genotyper.cpp:57-58.  One workgroup per locus.
struct GtLocus {
  int64_t ll_off, out_off, map_off;
  int32_t r0, r1, H, Hn;
};
template <bool DIRECT>
__global__ void ltr_genotype_gather_kernel(const GtLocus* __restrict__ loci, const double* __restrict__ ll,
                                           const int32_t* __restrict__ pool_index, const int32_t* __restrict__ map,
                                           double* __restrict__ out) {
  const GtLocus L = loci[blockIdx.x];
  const int32_t* cmap = L.map_off >= 0 ? map + L.map_off : nullptr;
  const int64_t n = (int64_t)(L.r1 - L.r0) * L.Hn;
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
    const int64_t j = k / L.Hn;
    const int a = (int)(k - j * L.Hn);
    out[L.out_off + k] = ltr_clamped_ll(ll + L.ll_off + (DIRECT ? j : (int64_t)pool_index[L.r0 + j]) * L.H, cmap, a);
  }
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

// The launches of a pass: one per shape with units (d_lists: the unit lists of shape 0 then shape 1, or null when there is one
// shape), then the finish kernel over the units whose block did not fit LDS (d_unfused: shape 0's then shape 1's).
void launch_pass(const PassShape& ps, hipStream_t st, const GtUnit* d_units, const LlSource& src, const DevReads& rd, const int32_t* d_map,
                 const int32_t* d_lists, const int32_t* d_unfused, const DevPass& out) {
  for (int g = 0; g < 2; ++g) {
    const LaunchShape& sh = ps.sh[g];
    if (sh.n == 0) continue;
    const int32_t* list = d_lists ? d_lists + (g == 0 ? 0 : ps.sh[0].n) : nullptr;
    // (sh.nt is the kernel's NT: shape_of sets 64 for shape 0, 256 for shape 1)
    const auto kernel = src.direct ? (g == 0 ? ltr_genotype_kernel<64, true> : ltr_genotype_kernel<256, true>)
                                   : (g == 0 ? ltr_genotype_kernel<64, false> : ltr_genotype_kernel<256, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)sh.n), dim3(sh.nt), sh.lds, st, d_units, src.base, rd.pool_index,
                       rd.lp1, rd.lp2, rd.label, d_map, list, sh.tile, sh.post_cap, out.post, out.stl, out.gts);
  }
  const size_t nf = ps.sh[0].unfused.size() + ps.sh[1].unfused.size();
  if (nf)
    hipLaunchKernelGGL(ltr_genotype_finish_kernel, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, st, (int)nf, d_unfused, d_units, out.post, out.stl, out.gts);
}
// the unit lists / unfused lists of a pass on the device (null: none needed; with one shape the unit lists are empty)
int upload_lists(ltr_ctx* ctx, DevLease& lease, const PassShape& ps, const int32_t** d_lists, const int32_t** d_unf) {
  *d_lists = nullptr; *d_unf = nullptr;
  const size_t nlist = ps.sh[0].list.size() + ps.sh[1].list.size(), n = nlist + ps.sh[0].unfused.size() + ps.sh[1].unfused.size();
  if (n == 0) return LTR_OK;
  int32_t* stage = lease.host<int32_t>(n);
  int32_t* at = stage;
  for (int g = 0; g < 2; ++g) at = std::copy(ps.sh[g].list.begin(), ps.sh[g].list.end(), at);
  for (int g = 0; g < 2; ++g) at = std::copy(ps.sh[g].unfused.begin(), ps.sh[g].unfused.end(), at);
  int32_t* d = nullptr;
  DEV_TRY(ctx, lease.alloc(&d, n * 4));
  DEV_TRY(ctx, hipMemcpyAsync(d, stage, n * 4, hipMemcpyHostToDevice, lease.st));
  if (nlist) *d_lists = d;
  *d_unf = d + nlist;
  return LTR_OK;
}

// the two pinned staging blocks of ltr_ll_genotype's upload, from the context's cache and back to it
struct PinnedPair {
  ltr_ctx* ctx; double* p[2] = {nullptr, nullptr};
  explicit PinnedPair(ltr_ctx* c) : ctx(c) {}
  PinnedPair(const PinnedPair&) = delete;
  ~PinnedPair() { ctx_give_pinned(ctx, p[0]); ctx_give_pinned(ctx, p[1]); }
};

// One call of ltr_plan_genotype / ltr_plan_genotype_fields / ltr_ll_genotype.  The ORDER of the members carries the invariant of
// DevLease: the host memory that queued copies read or write (the result's arrays, the second pass's units and column maps, the
// staging blocks of the LL upload) comes first and the lease last, so on every way out -- return, error return, exception -- the
// lease drains the stream and gives the blocks back before any of that memory is freed or handed to another call.  (The first
// pass's units live in the context; all other staging comes from lease.host().)
struct GtCall {
  ltr_ctx* ctx; const ltr_genotype_batch* gb; const ltr_posterior_batch* pb; const ltr_fields_request* fr;
  LlSource src;                                     // where the scores lie and how a read finds its row: the plan's buffer, or the block upload_ll fills
  std::vector<int64_t> ll_off;                      // ... the locus offsets of that block (src.locus_off)
  PinnedPair stage;                                 // ... its staging
  const uint8_t* locus_haploid;                     // the caller's ploidy per locus; null: pb->haploid for all (resolved into res->haploid by layout_units)
  const uint8_t* sample_haploid = nullptr;          // ... per (locus, sample) in unit order (ltr_gpu_ploidy.h); null: the locus's (resolved into res->sample_haploid there too)
  std::unique_ptr<ltr_genotype_result> res;
  GtUnit* units = nullptr; size_t nu = 0;           // the first pass's units (ctx->gt_units)
  std::vector<uint8_t> aligned;                     // per unit: one of the sample's reads was aligned (:262-266)
  std::vector<GtUnit> units2; std::vector<int32_t> map; std::vector<int64_t> affected; int64_t npost2 = 0;   // the second pass: units, new_to_old of its loci, the loci
  double* stl2 = nullptr; int32_t* gts2 = nullptr;  // ... its totals and best pairs (lease.host)
  DevReads rd; int32_t* d_map = nullptr; DevPass pass[2];
  DevLease lease;
  GtCall(ltr_ctx* x, hipStream_t st, const LlSource& s, const ltr_genotype_batch* g, const ltr_fields_request* f, const uint8_t* lh)
      : ctx(x), gb(g), pb(g->pb), fr(f), src(s), stage(x), locus_haploid(lh), res(new ltr_genotype_result()), lease(x, st) {}
};

// ---- host, all loci at once: the result laid out, labels checked, every sample's reads listed in read order, aligned_read (:262-266) ----
int layout_units(GtCall& c) {
  ltr_ctx* ctx = c.ctx; const LlSource& src = c.src; ltr_genotype_result* res = c.res.get();
  const ltr_genotype_batch* gb = c.gb; const ltr_posterior_batch* pb = c.pb; const ltr_fields_request* fr = c.fr;
  const int64_t nl = pb->n_loci;
  const bool need_haps = gb->prune || fr;
  const std::string who(src.who);
  res->n_loci = nl;
  res->S.assign(pb->n_samples, pb->n_samples + nl);
  res->H.assign(src.H, src.H + nl);
  if (gb->haps) res->haps.assign(gb->haps, gb->haps + nl); else res->haps.assign((size_t)nl, nullptr);
  res->unit_off.assign((size_t)nl + 1, 0); res->post1_off.assign((size_t)nl + 1, 0);
  res->pruned.resize((size_t)nl); res->n_blocks.assign((size_t)nl, 0);
  res->haploid.assign((size_t)std::max<int64_t>(nl, 0), 0);
  const SamplePloidy ploidy(pb, c.locus_haploid, c.sample_haploid);
  std::vector<int64_t> pool_base(src.direct ? 0 : (size_t)nl + 1, 0);   // first pool (= read of the plan) of every locus
  int32_t max_H = 1;
  for (int64_t l = 0; l < nl; ++l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1];
    const int32_t S = pb->n_samples[l], H = src.H[l];
    if (r0 < 0 || r1 < r0 || r1 > pb->n_reads || S < 0 || r1 > 0x7fffffff) { ltr::set_error(ctx, "bad posterior batch offsets"); return LTR_ERR_INVALID; }
    if (H <= 0) { ltr::set_error(ctx, who + ": a locus without haplotypes"); return LTR_ERR_INVALID; }
    res->unit_off[(size_t)l + 1] = res->unit_off[(size_t)l] + S;
    res->post1_off[(size_t)l + 1] = res->post1_off[(size_t)l] + (int64_t)S * H * H;
    if (!src.direct) pool_base[(size_t)l + 1] = pool_base[(size_t)l] + src.P[l];
    max_H = std::max(max_H, H);
    res->haploid[(size_t)l] = (uint8_t)ploidy.all(l, res->unit_off[(size_t)l], S);
  }
  const size_t nu = c.nu = (size_t)res->unit_off[(size_t)nl];
  res->sample_haploid.assign(nu, 0);
  res->identity.resize((size_t)max_H);
  for (int32_t k = 0; k < max_H; ++k) res->identity[(size_t)k] = k;
  res->stl.assign(nu, 0.0); res->gts.assign(2 * nu, -1);
  LTR_DBG("genotype: %ld loci checked", (long)nl);
  ctx->gt_units.resize(nu * sizeof(GtUnit));                  // (kept by the context: 13 MB of fresh pages per call on a catalogue otherwise)
  GtUnit* units = c.units = reinterpret_cast<GtUnit*>(ctx->gt_units.p);
  c.aligned.assign(nu, 0);
  std::atomic<int> bad(0);
  std::atomic<int64_t> bad_haps(-1), bad_block(-1);
  if (fr) { res->has_fields = true; res->ctx = ctx; res->f_block.assign((size_t)nl, 0); res->f_V.assign((size_t)nl, 0); }
  ltr::parallel_for(nl, 64, [&](int64_t l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1], u0 = res->unit_off[(size_t)l];
    const int32_t S = pb->n_samples[l], H = src.H[l];
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
    if (src.direct) {                                          // a row and a seed per read (null: every read aligned)
      const int32_t* seed = src.read_seed ? src.read_seed[l] : nullptr;
      for (int64_t r = r0; r < r1; ++r) {
        const int32_t s = pb->sample_label[r];
        if (s < 0 || s >= S) { bad.store(1); return; }
        if (!seed || seed[r - r0] >= 0) c.aligned[(size_t)(u0 + s)] = 1;
      }
    } else {
      const int32_t P = src.P[l];
      for (int64_t r = r0; r < r1; ++r) {
        const int32_t q = pb->pool_index[r], s = pb->sample_label[r];
        if (q < 0 || q >= P || s < 0 || s >= S) { bad.store(1); return; }
        if (src.pool_seed[pool_base[(size_t)l] + q] >= 0) c.aligned[(size_t)(u0 + s)] = 1;     // seed_positions_[read] >= 0, :265
      }
    }
    for (int32_t s = 0; s < S; ++s) {
      GtUnit& u = units[(size_t)(u0 + s)];
      u.ll_off = src.locus_off[l]; u.post_off = res->post1_off[(size_t)l] + (int64_t)s * H * H; u.map_off = -1;
      u.r0 = (int32_t)r0; u.r1 = (int32_t)r1;
      u.H = H; u.Hn = H; u.out = (int32_t)(u0 + s); u.sample = s;
      res->sample_haploid[(size_t)(u0 + s)] = (uint8_t)ploidy(l, u0 + s);
      ltr_log_priors(H, res->sample_haploid[(size_t)(u0 + s)], &u.homoz, &u.hetz);   // the priors of a unit follow its sample
    }
  });
  if (bad_haps.load() >= 0) {
    const int64_t l = bad_haps.load();
    ltr::set_error(ctx, "haplotype blocks of locus " + std::to_string(l) + " do not enumerate the " + (src.direct ? "batch's " : "plan's ") + std::to_string(src.H[l]) + " haplotypes");
    return LTR_ERR_INVALID;
  }
  if (bad_block.load() >= 0) {
    ltr::set_error(ctx, (src.direct ? who : who + "_fields") + ": locus " + std::to_string(bad_block.load()) + (fr->block ? ": block out of range" : ": no repeat block"));
    return LTR_ERR_INVALID;
  }
  if (bad.load()) { ltr::set_error(ctx, src.direct ? "sample label out of range" : "pool index / sample label out of range"); return LTR_ERR_INVALID; }
  return LTR_OK;
}

// ---- one pass over `units`: calc_log_sample_posteriors + get_optimal_haplotypes (genotyper.cpp:45-100) ----
// Totals and best pairs go to stl / gts, the blocks to post (null: they stay on the device).  wait: the host needs the best
// pairs before it goes on; the blocks follow behind its back.
int run_pass(GtCall& c, DevPass* dp, const GtUnit* units, size_t nu, int64_t npost, const int32_t* d_map, double* stl, int32_t* gts, double* post, bool wait) {
  ltr_ctx* ctx = c.ctx;
  hipStream_t st = c.lease.st;
  const PassShape ps = shape_of(units, nu);
  GtUnit* d_units = nullptr;
  const int32_t *d_lists = nullptr, *d_unf = nullptr;
  DEV_TRY(ctx, c.lease.alloc(&d_units, nu * sizeof(GtUnit)));
  DEV_TRY(ctx, c.lease.alloc(&dp->post, (size_t)std::max<int64_t>(npost, 1) * 8));
  DEV_TRY(ctx, c.lease.alloc(&dp->stl, nu * 8));
  DEV_TRY(ctx, c.lease.alloc(&dp->gts, nu * 8));
  DEV_TRY(ctx, hipMemcpyAsync(d_units, units, nu * sizeof(GtUnit), hipMemcpyHostToDevice, st));
  if (int rc = upload_lists(ctx, c.lease, ps, &d_lists, &d_unf)) return rc;
  launch_pass(ps, st, d_units, c.src, c.rd, d_map, d_lists, d_unf, *dp);
  DEV_TRY(ctx, hipGetLastError());
  DEV_TRY(ctx, hipMemcpyAsync(gts, dp->gts, nu * 8, hipMemcpyDeviceToHost, st));
  DEV_TRY(ctx, hipMemcpyAsync(stl, dp->stl, nu * 8, hipMemcpyDeviceToHost, st));
  if (wait) DEV_TRY(ctx, hipStreamSynchronize(st));
  if (post) DEV_TRY(ctx, hipMemcpyAsync(post, dp->post, (size_t)npost * 8, hipMemcpyDeviceToHost, st));
  return LTR_OK;
}

// get_unused_alleles (seq_stutter_genotyper.cpp:250-308) of one locus from the first pass's best pairs, then its new block list
// and column maps (remove_alleles -> add_and_remove_alleles, :317-377).  0, or 1: malformed blocks, 2: a sample without a pair
int prune_locus(const GtCall& c, int64_t l, std::unique_ptr<LtrPruned>* out) {
  const ltr_genotype_batch* gb = c.gb; const ltr_genotype_result* res = c.res.get();
  const ltr_haplotype_blocks* hb = gb->haps[l];
  const int nb = hb->n_blocks;
  const int32_t S = res->S[(size_t)l], H = res->H[(size_t)l];
  if (H == 1) return 0;                                        // every block has one option, :274
  const int64_t u0 = res->unit_off[(size_t)l];
  std::vector<int32_t> counts; int64_t nc = 0;
  if (ltr::haplotype_counts(hb, &counts, &nc) != LTR_OK || nc != H) return 1;
  std::vector<std::vector<int32_t>> removed((size_t)nb);
  int32_t aff_blocks = 0, aff_alleles = 0;
  for (int b = 0; b < nb; ++b) {
    const int n = hb->n_alleles[b];
    if (n == 1) continue;                                      // :274
    std::vector<uint8_t> called((size_t)n, 0);
    for (int32_t s = 0; s < S; ++s) {
      if (!c.aligned[(size_t)(u0 + s)] || (gb->sample_filtered && gb->sample_filtered[u0 + s])) continue;   // :289
      const int32_t g1 = res->gts[(size_t)(2 * (u0 + s))], g2 = res->gts[(size_t)(2 * (u0 + s) + 1)];
      if (g1 < 0 || g1 >= H || g2 < 0 || g2 >= H) return 2;
      called[(size_t)counts[(size_t)((int64_t)g1 * nb + b)]] = 1;        // haps_to_alleles, :240-248, :290-291
      called[(size_t)counts[(size_t)((int64_t)g2 * nb + b)]] = 1;
    }
    for (int a = 1; a < n; ++a) if (!called[(size_t)a]) { removed[(size_t)b].push_back(a); ++aff_alleles; }   // :298-304
    if (!removed[(size_t)b].empty()) ++aff_blocks;
  }
  if (aff_alleles == 0) return 0;                              // :641
  std::unique_ptr<LtrPruned> p(new LtrPruned());
  if (ltr::prune_hap_blocks(hb, removed, &p->blocks) != LTR_OK || ltr::remap_haplotypes(hb, &p->blocks.view, &p->allele_mapping, nullptr) != LTR_OK) return 1;
  p->Hn = (int32_t)ltr_haplotype_num_combs(&p->blocks.view);
  p->new_to_old.assign((size_t)p->Hn, -1);
  for (int32_t j = 0; j < H; ++j) if (p->allele_mapping[(size_t)j] >= 0) p->new_to_old[(size_t)p->allele_mapping[(size_t)j]] = j;
  p->removed.swap(removed); p->aff_blocks = aff_blocks; p->aff_alleles = aff_alleles;
  *out = std::move(p);
  return 0;
}

// ---- between the passes (host, all loci at once, no HIP): the loci that lost alleles and the units of the second pass ----
int prune_uncalled(GtCall& c) {
  ltr_genotype_result* res = c.res.get();
  const int64_t nl = res->n_loci;
  std::atomic<int> perr(0);
  ltr::parallel_for(nl, 64, [&](int64_t l) { if (const int e = prune_locus(c, l, &res->pruned[(size_t)l])) perr.store(e); }, 16);
  if (perr.load()) {
    ltr::set_error(c.ctx, std::string(c.src.who) + (perr.load() == 2 ? ": a sample without an optimal haplotype pair (NaN scores?)" : ": malformed haplotype blocks"));
    return LTR_ERR_INVALID;
  }
  for (int64_t l = 0; l < nl; ++l) {
    LtrPruned* p = res->pruned[(size_t)l].get();
    if (!p) continue;
    const int32_t S = res->S[(size_t)l];
    const int64_t map_off = (int64_t)c.map.size();
    c.map.insert(c.map.end(), p->new_to_old.begin(), p->new_to_old.end());
    p->post_off = c.npost2;
    for (int32_t s = 0; s < S; ++s) {
      GtUnit u = c.units[(size_t)(res->unit_off[(size_t)l] + s)];
      u.post_off = c.npost2 + (int64_t)s * p->Hn * p->Hn; u.map_off = map_off; u.Hn = p->Hn; u.out = (int32_t)c.units2.size();
      ltr_log_priors(p->Hn, res->sample_haploid[(size_t)(res->unit_off[(size_t)l] + s)], &u.homoz, &u.hetz);   // :405-408: priors of the new number of haplotypes, the sample's ploidy
      c.units2.push_back(u);
    }
    c.npost2 += (int64_t)S * p->Hn * p->Hn;
    c.affected.push_back(l);
  }
  return LTR_OK;
}

// ---- log_aln_probs_ per read in the final columns (ltr_genotype_gather_kernel) ----
int gather_read_ll(GtCall& c) {
  ltr_ctx* ctx = c.ctx; ltr_genotype_result* res = c.res.get();
  const ltr_posterior_batch* pb = c.pb;
  const int64_t nl = res->n_loci;
  hipStream_t st = c.lease.st;
  GtLocus* gl = c.lease.host<GtLocus>((size_t)nl);
  res->read_ll_off.assign((size_t)nl + 1, 0);
  int64_t mo = 0;
  for (int64_t l = 0; l < nl; ++l) {
    const LtrPruned* p = res->pruned[(size_t)l].get();
    GtLocus& g = gl[(size_t)l];
    g.ll_off = c.src.locus_off[l]; g.out_off = res->read_ll_off[(size_t)l]; g.map_off = p ? mo : -1;
    g.r0 = (int32_t)pb->locus_read_off[l]; g.r1 = (int32_t)pb->locus_read_off[l + 1]; g.H = res->H[(size_t)l]; g.Hn = p ? p->Hn : g.H;
    if (p) mo += p->Hn;
    res->read_ll_off[(size_t)l + 1] = g.out_off + (int64_t)(g.r1 - g.r0) * g.Hn;
  }
  const int64_t nrll = res->read_ll_off[(size_t)nl];
  res->read_ll.reset(new double[(size_t)std::max<int64_t>(nrll, 1)]);
  GtLocus* d_loci = nullptr; double* d_rll = nullptr;
  DEV_TRY(ctx, c.lease.alloc(&d_loci, (size_t)nl * sizeof(GtLocus)));
  DEV_TRY(ctx, c.lease.alloc(&d_rll, (size_t)std::max<int64_t>(nrll, 1) * 8));
  DEV_TRY(ctx, hipMemcpyAsync(d_loci, gl, (size_t)nl * sizeof(GtLocus), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(c.src.direct ? ltr_genotype_gather_kernel<true> : ltr_genotype_gather_kernel<false>, dim3((unsigned)nl), dim3(64), 0, st, d_loci,
                     c.src.base, c.rd.pool_index, c.d_map, d_rll);
  DEV_TRY(ctx, hipGetLastError());
  if (nrll) DEV_TRY(ctx, hipMemcpyAsync(res->read_ll.get(), d_rll, (size_t)nrll * 8, hipMemcpyDeviceToHost, st));
  return LTR_OK;
}

// the pruned loci's totals and best pairs replace the first pass's
void merge_second_pass(GtCall& c) {
  ltr_genotype_result* res = c.res.get();
  size_t k = 0;
  for (int64_t l : c.affected) {
    const int32_t S = res->S[(size_t)l];
    const int64_t u0 = res->unit_off[(size_t)l];
    for (int32_t s = 0; s < S; ++s, ++k) {
      res->stl[(size_t)(u0 + s)] = c.stl2[k];
      res->gts[(size_t)(2 * (u0 + s))] = c.gts2[2 * k]; res->gts[(size_t)(2 * (u0 + s) + 1)] = c.gts2[2 * k + 1];
    }
  }
}

// ---- ltr_ll_genotype: the caller's per-read matrices, one block on the device for the whole call (both passes, the gather and the
// fields stage read it).  The matrices are scattered pageable arrays: the worker pool copies the loci of a chunk into one of two
// pinned staging blocks while the copy of the chunk before is still on its way (an event per block says when it may be filled
// again).  Chunks: as many loci as fit kLlChunkBytes, at least one (debug knob ll_chunk_loci: that many loci).
constexpr size_t kLlChunkBytes = (size_t)8 << 20;
int upload_ll(GtCall& c, const ltr_ll_batch* lb) {
  ltr_ctx* ctx = c.ctx;
  hipStream_t st = c.lease.st;
  const int64_t nl = c.pb->n_loci, total = c.ll_off[(size_t)nl], knob = ctx->dbg.ll_chunk_loci;
  double* d_ll = nullptr;
  DEV_TRY(ctx, c.lease.alloc(&d_ll, (size_t)std::max<int64_t>(total, 1) * 8));
  c.src.base = d_ll;
  if (total == 0) return LTR_OK;
  std::vector<int64_t> cut(1, 0);                               // chunk k: loci [cut[k], cut[k + 1])
  int64_t largest = 0;
  for (int64_t l0 = 0; l0 < nl;) {
    int64_t l1 = l0 + 1;
    if (knob > 0) l1 = std::min(nl, l0 + knob);
    else while (l1 < nl && (size_t)(c.ll_off[(size_t)l1 + 1] - c.ll_off[(size_t)l0]) * 8 <= kLlChunkBytes) ++l1;
    largest = std::max(largest, c.ll_off[(size_t)l1] - c.ll_off[(size_t)l0]);
    cut.push_back(l1);
    l0 = l1;
  }
  const size_t nchunks = cut.size() - 1;
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int b = 0; b < (nchunks > 1 ? 2 : 1); ++b) {
    size_t cap = 0; double* dev = nullptr;
    c.stage.p[b] = ctx_take_pinned(ctx, (size_t)std::max<int64_t>(largest, 1) * 8, &cap, &dev);
    if (!c.stage.p[b]) { ltr::set_error(ctx, "ltr_ll_genotype: out of pinned host memory"); return LTR_ERR_NOMEM; }
    DEV_TRY(ctx, c.lease.event(&ev[b], false));
  }
  LTR_DBG("ll_genotype: upload of %lld bytes in %zu chunks begins", (long long)total * 8, nchunks);
  for (size_t k = 0; k < nchunks; ++k) {
    const int b = (int)(k & 1);
    const int64_t l0 = cut[k], l1 = cut[k + 1], base = c.ll_off[(size_t)l0], n = c.ll_off[(size_t)l1] - base;
    if (n == 0) continue;
    if (k >= 2) DEV_TRY(ctx, hipEventSynchronize(ev[b]));       // the copy of chunk k - 2 has left this block
    double* stage = c.stage.p[b];
    ltr::parallel_for(l1 - l0, 16, [&](int64_t i) {
      const int64_t l = l0 + i, len = c.ll_off[(size_t)l + 1] - c.ll_off[(size_t)l];
      if (len) std::memcpy(stage + (c.ll_off[(size_t)l] - base), lb->log_aln_probs[l], (size_t)len * 8);
    }, 16);
    DEV_TRY(ctx, hipMemcpyAsync(d_ll + base, stage, (size_t)n * 8, hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipEventRecord(ev[b], st));
  }
  if (ltr::g_trace.load(std::memory_order_relaxed)) {           // (the phase's own time: the trace waits for it, a plain call does not)
    DEV_TRY(ctx, hipStreamSynchronize(st));
    LTR_DBG("ll_genotype: upload of %lld bytes done", (long long)total * 8);
  }
  return LTR_OK;
}

// The stages of one call.  lb: the per-read matrices of ltr_ll_genotype, uploaded once every check has passed (null: c.src is a plan's buffer).
// With fr the fields stage runs on the passes' buffers before they go back to the pool, and the posterior blocks are fetched
// only when fr asks for them.
int genotype_stages(GtCall& c, const ltr_ll_batch* lb, ltr_genotype_result** out) {
  ltr_ctx* ctx = c.ctx; const ltr_genotype_batch* gb = c.gb; const ltr_posterior_batch* pb = c.pb; const ltr_fields_request* fr = c.fr;
  const int64_t nl = pb->n_loci;
  const bool fetch_post = !fr || fr->want_posteriors;
  ltr_genotype_result* res = c.res.get();
  if (int rc = layout_units(c)) return rc;
  if (c.nu == 0) {                                             // (no sample anywhere: nothing to compute; read_ll stays NULL)
    if (fr) ltr_plan_fields_empty(gb, res);
    *out = c.res.release(); return LTR_OK;
  }
  LTR_DBG("genotype: %zu units laid out", c.nu);
  if (lb) if (int rc = upload_ll(c, lb)) return rc;
  if (int rc = upload_reads(ctx, c.lease, pb, &c.rd, !c.src.direct)) return rc;
  // first pass: calc_log_sample_posteriors + get_optimal_haplotypes, :635
  const int64_t npost1 = res->post1_off[(size_t)nl];
  if (fetch_post) res->post1.reset(new double[(size_t)std::max<int64_t>(npost1, 1)]);
  if (int rc = run_pass(c, &c.pass[0], c.units, c.nu, npost1, nullptr, res->stl.data(), res->gts.data(), res->post1.get(), true)) return rc;
  LTR_DBG("genotype: first pass done");
  if (gb->prune) if (int rc = prune_uncalled(c)) return rc;
  LTR_DBG("genotype: %zu loci pruned", c.affected.size());
  // second pass, the loci that lost alleles only: calc_log_sample_posteriors of add_and_remove_alleles, :405-408
  if (!c.map.empty()) {
    DEV_TRY(ctx, c.lease.alloc(&c.d_map, c.map.size() * 4));
    DEV_TRY(ctx, hipMemcpyAsync(c.d_map, c.map.data(), c.map.size() * 4, hipMemcpyHostToDevice, c.lease.st));
  }
  if (!c.units2.empty()) {
    const size_t nu2 = c.units2.size();
    if (fetch_post) res->post2.reset(new double[(size_t)std::max<int64_t>(c.npost2, 1)]);
    c.stl2 = c.lease.host<double>(nu2); c.gts2 = c.lease.host<int32_t>(2 * nu2);
    if (int rc = run_pass(c, &c.pass[1], c.units2.data(), nu2, c.npost2, c.d_map, c.stl2, c.gts2, res->post2.get(), false)) return rc;
  }
  if (gb->want_read_ll) if (int rc = gather_read_ll(c)) return rc;
  // the VCF fields of every locus (ltr_plan_fields.hip), on the final posterior blocks where they lie
  if (fr) if (int rc = ltr_plan_fields_stage(ctx, c.src, gb, fr, res, c.rd, c.d_map, c.pass, c.lease)) return rc;
  DEV_TRY(ctx, c.lease.drain());
  LTR_DBG("genotype: second pass and gather done");
  merge_second_pass(c);
  *out = c.res.release();
  return LTR_OK;
}

}  // namespace

// ltr_plan_genotype (fr == null), ltr_plan_genotype_fields and ltr_plan_genotype_ploidy: the stages on the LL buffer of the plan's last execute
static int plan_genotype(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* locus_haploid, const uint8_t* sample_haploid,
                         ltr_genotype_result** out) {
  if (out) *out = nullptr;
  if (!plan || !gb || !gb->pb || !out) return LTR_ERR_INVALID;
  ltr_ctx* ctx = plan->ctx;
  if (!ctx) return LTR_ERR_INVALID;                          // the context was destroyed before this plan
  const ltr_posterior_batch* pb = gb->pb;
  if (!plan->executed) { ltr::set_error(ctx, "ltr_plan_genotype: execute the plan first"); return LTR_ERR_INVALID; }
  const int64_t nl = pb->n_loci;
  if (nl != (int64_t)plan->locus_P.size()) { ltr::set_error(ctx, "genotype batch and plan disagree on the number of loci"); return LTR_ERR_INVALID; }
  if (!gb->haps && nl > 0 && (gb->prune || fr)) { ltr::set_error(ctx, "ltr_plan_genotype: no haplotype blocks"); return LTR_ERR_INVALID; }
  if (nl > 0 && (!pb->locus_read_off || !pb->n_samples || (pb->n_reads > 0 && (!pb->pool_index || !pb->log_p1 || !pb->log_p2 || !pb->sample_label)))) {
    ltr::set_error(ctx, "ltr_plan_genotype: incomplete posterior batch"); return LTR_ERR_INVALID;
  }
  ltr::TimedCall timed(ctx, ltr::kTimerPosterior);             // total_posterior_time_, genotyper.cpp:46,:80-81
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LlSource src;                                                // the plan's buffer, byte for byte what the stages read before they took a source
  src.base = plan->last_out; src.locus_off = plan->locus_ll_off.data(); src.H = plan->locus_H.data(); src.P = plan->locus_P.data();
  src.pool_seed = plan->seed.data();
  GtCall c(ctx, plan->last_stream, src, gb, fr, locus_haploid);
  c.sample_haploid = sample_haploid;
  return genotype_stages(c, nullptr, out);
  LTR_GUARD_END(ctx)
}

extern "C" {

// the ploidy per locus (genotyper_bam_processor.cpp:248 -> :294); the two entry points below are this one with locus_haploid = null
int ltr_plan_genotype_ploidy(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* locus_haploid, ltr_genotype_result** out) {
  return plan_genotype(plan, gb, fr, locus_haploid, nullptr, out);
}
// ... per (locus, sample) (ltr_gpu_ploidy.h)
int ltr_plan_genotype_sample_ploidy(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* sample_haploid, ltr_genotype_result** out) {
  return plan_genotype(plan, gb, fr, nullptr, sample_haploid, out);
}
int ltr_plan_genotype(ltr_plan* plan, const ltr_genotype_batch* gb, ltr_genotype_result** out) { return ltr_plan_genotype_ploidy(plan, gb, nullptr, nullptr, out); }
int ltr_plan_genotype_fields(ltr_plan* plan, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result** out) {
  if (out) *out = nullptr;
  if (!fr) return LTR_ERR_INVALID;
  return ltr_plan_genotype_ploidy(plan, gb, fr, nullptr, out);
}

static int ll_genotype(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* locus_haploid,
                       const uint8_t* sample_haploid, ltr_genotype_result** out) {
  if (out) *out = nullptr;
  if (!ctx || !lb || !gb || !gb->pb || !out) return LTR_ERR_INVALID;
  const ltr_posterior_batch* pb = gb->pb;
  const int64_t nl = pb->n_loci;
  if (nl < 0) { ltr::set_error(ctx, "ltr_ll_genotype: a negative number of loci"); return LTR_ERR_INVALID; }
  if (nl > 0 && (!lb->log_aln_probs || !lb->n_haps)) { ltr::set_error(ctx, "ltr_ll_genotype: incomplete LL batch (locus 0: no matrix list or no n_haps)"); return LTR_ERR_INVALID; }
  if (!gb->haps && nl > 0 && (gb->prune || fr)) {
    ltr::set_error(ctx, "ltr_ll_genotype: no haplotype blocks (locus 0 and every other: pruning and the fields need them)"); return LTR_ERR_INVALID;
  }
  if (nl > 0 && (!pb->locus_read_off || !pb->n_samples || (pb->n_reads > 0 && (!pb->log_p1 || !pb->log_p2 || !pb->sample_label)))) {
    ltr::set_error(ctx, "ltr_ll_genotype: incomplete posterior batch"); return LTR_ERR_INVALID;
  }
  ltr::TimedCall timed(ctx, ltr::kTimerPosterior);
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LlSource src;
  src.direct = true; src.H = lb->n_haps; src.read_seed = lb->seed_positions; src.who = "ltr_ll_genotype";
  GtCall c(ctx, ctx->stream, src, gb, fr, locus_haploid);
  c.sample_haploid = sample_haploid;
  c.ll_off.assign((size_t)nl + 1, 0);                          // the blocks back to back, [R_l x H_l] each
  for (int64_t l = 0; l < nl; ++l) {
    const int64_t r0 = pb->locus_read_off[l], r1 = pb->locus_read_off[l + 1];
    const int32_t H = lb->n_haps[l];
    if (r0 < 0 || r1 < r0 || r1 > pb->n_reads || r1 > 0x7fffffff) { ltr::set_error(ctx, "bad posterior batch offsets (locus " + std::to_string(l) + ")"); return LTR_ERR_INVALID; }
    if (H <= 0) { ltr::set_error(ctx, "ltr_ll_genotype: locus " + std::to_string(l) + ": n_haps must be positive"); return LTR_ERR_INVALID; }
    if (r1 > r0 && !lb->log_aln_probs[l]) { ltr::set_error(ctx, "ltr_ll_genotype: locus " + std::to_string(l) + " has reads and no matrix"); return LTR_ERR_INVALID; }
    c.ll_off[(size_t)l + 1] = c.ll_off[(size_t)l] + (r1 - r0) * (int64_t)H;
  }
  c.src.locus_off = c.ll_off.data();
  return genotype_stages(c, lb, out);
  LTR_GUARD_END(ctx)
}
int ltr_ll_genotype_ploidy(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* locus_haploid,
                           ltr_genotype_result** out) {
  return ll_genotype(ctx, lb, gb, fr, locus_haploid, nullptr, out);
}
int ltr_ll_genotype_sample_ploidy(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr, const uint8_t* sample_haploid,
                                  ltr_genotype_result** out) {
  return ll_genotype(ctx, lb, gb, fr, nullptr, sample_haploid, out);
}
int ltr_ll_genotype(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb, const ltr_fields_request* fr, ltr_genotype_result** out) {
  return ltr_ll_genotype_ploidy(ctx, lb, gb, fr, nullptr, out);
}

void ltr_genotype_result_free(ltr_genotype_result* r) { delete r; }

#define GT_LOCUS(r, l, fail) if (!(r) || (l) < 0 || (l) >= (r)->n_loci) return fail
int64_t ltr_genotype_result_n_loci(const ltr_genotype_result* r) { return r ? r->n_loci : LTR_ERR_INVALID; }
int32_t ltr_genotype_result_haploid(const ltr_genotype_result* r, int64_t l) {
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  return r->haploid[(size_t)l] ? 1 : 0;
}
int32_t ltr_genotype_result_sample_haploid(const ltr_genotype_result* r, int64_t l, int32_t s) {
  GT_LOCUS(r, l, LTR_ERR_INVALID);
  if (s < 0 || s >= r->S[(size_t)l]) return LTR_ERR_INVALID;
  return r->sample_haploid[(size_t)(r->unit_off[(size_t)l] + s)] ? 1 : 0;
}
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
