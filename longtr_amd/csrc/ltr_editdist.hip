// ltr_editdist.hip -- ltr_edit_distances: capped unit-cost edit distance of all pairs of every group of sequences, the distance
// HaplotypeGenerator's needleman_wunsch (HaplotypeGenerator.cpp:201-234) takes cell by cell, by the bit-vector block algorithm
// (Myers 1999 in Hyyro's block form for the global distance): 64 rows of the pattern per lane in two 64-bit registers.
//
// Geometry: the shorter sequence of a pair is the pattern, cut into blocks of 64 rows; lane k of the pair's segment owns block k
// (Pv, Mv).  Text columns stream through the lanes skewed by one column per lane -- the DP kernels' anti-diagonal geometry
// (ltr_dp_kernel.hpp), turned to rows: at step t lane k works on column t - k.  What a block hands down per column, the
// horizontal difference hout in {-1, 0, +1} of its last row, goes to the next lane by DPP wave_shr:1 together with the column's
// text code; the head lane of a segment reads the text itself and takes hin = +1 (row 0 is D[0][j] = j).
// Match masks: the host remaps the bytes of a group to dense codes (at most 32); at the start of a pair every lane builds the
// masks of its own block, one 64-bit word per code, into the LDS table [code][lane].  Eq is then one ds_read_b64 per step, each
// lane in its own column of the table: consecutive lanes read consecutive 8-byte words, which is conflict free.
// Packing: LP = the power of two >= ceil(n / 64) lanes per pair, 64 / LP pairs per wavefront (the scheme of ltr_dp_pack.hpp), pairs
// sorted by (LP, text length) because the pairs of a wavefront run in lock step.  A pattern of more than 4096 rows runs in
// passes of 4096 rows: the last lane's hout per column, two bits a column, is the next pass's hin of the head lane; the strip lies
// in LDS up to kEdStripLdsCols columns and in a global strip of the call's lease beyond.
// The launch is a plain grid, one wavefront per workgroup: no work queue, no atomics, no persistent loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ltr_gpu.h"
#include "ltr_ctx.h"

namespace {

constexpr int kEdPassRows = 4096;          // rows of the pattern per pass: 64 lanes x 64 rows
constexpr int kEdStripLdsCols = 8192;      // columns of the pass boundary kept in LDS (2 bits a column: 2 KB)
constexpr int kEdMaxCodes = 32;
constexpr int kEdPad = 64;                 // 0xFF bytes behind every sequence of the device buffer (a code that matches nothing)

struct EdPair { int64_t pat_off, txt_off; int32_t n, m; };      // offsets into the code buffer (multiples of 64); 1 <= n <= m
struct EdWave { int64_t strip_off; int32_t first_pair, n_pairs, lp_log2, max_m, n_pass, n_codes; };   // strip_off: words into the global strips, -1 = LDS

__device__ __forceinline__ int ed_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true); }

// bit q of the result = (byte q of w == c)
__device__ __forceinline__ uint32_t ed_eq_bytes(uint64_t w, uint64_t c_rep) {
  const uint64_t x = w ^ c_rep, k7 = 0x7f7f7f7f7f7f7f7full;
  const uint64_t y = ~(((x & k7) + k7) | x | k7);               // 0x80 in every byte of x that is zero
  return (uint32_t)(((y >> 7) * 0x0102040810204080ull) >> 56);
}

__global__ __launch_bounds__(64) void ltr_editdist_kernel(const EdWave* __restrict__ waves, const EdPair* __restrict__ pairs,
                                                          const uint8_t* __restrict__ codes, uint32_t* strips, int32_t cap,
                                                          int32_t table_codes, int32_t* __restrict__ out) {
  extern __shared__ uint64_t ed_lds[];
  uint64_t* const tab = ed_lds;                                 // [code][lane]
  uint32_t* const lds_strip = reinterpret_cast<uint32_t*>(ed_lds + (size_t)table_codes * 64);
  const int lane = threadIdx.x;
  const EdWave w = waves[blockIdx.x];
  const int LP = 1 << w.lp_log2, seg = lane >> w.lp_log2, k = lane & (LP - 1);
  const bool have = seg < w.n_pairs;
  EdPair p = {0, 0, 0, 0};
  if (have) p = pairs[w.first_pair + seg];
  const int n = p.n, m = p.m, nb_total = (n + 63) >> 6;
  const int T = w.max_m + LP - 1;
  uint32_t* const gstrip = w.strip_off >= 0 ? strips + w.strip_off : nullptr;
  int score = n;
  bool owner = false;                                           // this lane holds the pattern's last block
  for (int pass = 0; pass < w.n_pass; ++pass) {
    const int b = pass * 64 + k;
    const bool block_on = have && b < nb_total;
    if (pass > 0) __syncthreads();                              // (the table and the LDS strip of the pass before are read no more)
    {
      uint64_t wd[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wd[q] = block_on ? reinterpret_cast<const uint64_t*>(codes + p.pat_off + (int64_t)b * 64)[q] : ~0ull;
      for (int c = 0; c < w.n_codes; ++c) {
        const uint64_t c_rep = (uint64_t)c * 0x0101010101010101ull;
        uint64_t mask = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) mask |= (uint64_t)ed_eq_bytes(wd[q], c_rep) << (8 * q);
        tab[c * 64 + lane] = mask;
      }
    }
    if (gstrip) __threadfence();
    __syncthreads();
    const bool last_block = block_on && b == nb_total - 1;
    const bool write_strip = block_on && k == 63 && pass + 1 < w.n_pass;
    const int out_bit = last_block ? ((n - 1) & 63) : 63;
    owner = last_block;
    uint64_t Pv = ~0ull, Mv = 0, chunk = 0;
    int carry = 0;                                              // (text code << 2) | (hout + 1) of the step before
    uint32_t strip_in = 0, strip_out = 0;
    for (int t = 0; t < T; ++t) {
      const int j = t - k;
      const int prev = ed_shr1(carry);
      int code, hin;
      if (k == 0) {
        if ((t & 7) == 0 && t < m) chunk = *reinterpret_cast<const uint64_t*>(codes + p.txt_off + t);
        code = (int)((chunk >> (8 * (t & 7))) & 0xff);
        hin = 1;
        if (pass > 0 && t < m) {
          if ((t & 15) == 0) strip_in = gstrip ? __hip_atomic_load(gstrip + (t >> 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : lds_strip[t >> 4];
          hin = (int)((strip_in >> (2 * (t & 15))) & 3u) - 1;
        }
      } else {
        code = prev >> 2;
        hin = (prev & 3) - 1;
      }
      const bool act = block_on && j >= 0 && j < m;
      uint64_t Eq = tab[(act ? code : 0) * 64 + lane];
      if (hin < 0) Eq |= 1ull;
      const uint64_t Xv = Eq | Mv;
      const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      uint64_t Ph = Mv | ~(Xh | Pv);
      uint64_t Mh = Pv & Xh;
      const int hout = (int)((Ph >> out_bit) & 1ull) - (int)((Mh >> out_bit) & 1ull);
      Ph = (Ph << 1) | (hin > 0 ? 1ull : 0ull);
      Mh = (Mh << 1) | (hin < 0 ? 1ull : 0ull);
      if (act) {
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        if (last_block) score += hout;
      }
      carry = (code << 2) | (hout + 1);
      if (write_strip && act) {
        strip_out |= (uint32_t)(hout + 1) << (2 * (j & 15));
        if ((j & 15) == 15 || j == m - 1) {
          if (gstrip) __hip_atomic_store(gstrip + (j >> 4), strip_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else lds_strip[j >> 4] = strip_out;
          strip_out = 0;
        }
      }
    }
  }
  if (owner) out[w.first_pair + seg] = score < cap ? score : cap;
}

struct HostPair { EdPair d; int64_t at, mirror; int32_t lp_log2, n_codes; };

}  // namespace

extern "C" {

int ltr_edit_distances(ltr_ctx* ctx, const ltr_seq_groups* sg, int32_t cap, int32_t* dist, const int64_t* dist_off) {
  if (!ctx) return LTR_ERR_NO_DEVICE;                           // (a context exists only on a device: there is no CPU fallback)
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  auto bad = [&](const std::string& msg) { ltr::set_error(ctx, "ltr_edit_distances: " + msg); return LTR_ERR_INVALID; };
  if (!sg || sg->n_groups < 0 || sg->n_seqs < 0 || cap < 1 || cap > 32767) return bad("bad arguments (1 <= cap <= 32767)");
  if (sg->n_groups == 0) return LTR_OK;
  if (!sg->group_seq_off || !sg->seq_off || !dist || !dist_off || (sg->seq_off[sg->n_seqs] > 0 && !sg->seq_bytes)) return bad("null array");
  for (int64_t s = 0; s < sg->n_seqs; ++s)
    if (sg->seq_off[s] < 0 || sg->seq_off[s + 1] < sg->seq_off[s]) return bad("sequence offsets of sequence " + std::to_string(s) + " are not ascending");
  // per group: the dense codes of its bytes; every sequence once in the code buffer, padded to blocks of 64
  std::vector<int64_t> code_off((size_t)sg->n_seqs + 1, -1);
  std::vector<int32_t> group_codes((size_t)sg->n_groups, 0);
  int64_t code_bytes = 0;
  int max_codes = 1;
  for (int64_t g = 0; g < sg->n_groups; ++g) {
    const int64_t s0 = sg->group_seq_off[g], s1 = sg->group_seq_off[g + 1];
    if (s0 < 0 || s1 < s0 || s1 > sg->n_seqs) return bad("group " + std::to_string(g) + ": sequence range out of bounds");
    if (dist_off[g] < 0) return bad("group " + std::to_string(g) + ": negative offset of its matrix");
    bool seen[256] = {false};
    int n_codes = 0;
    for (int64_t b = sg->seq_off[s0]; b < sg->seq_off[s1]; ++b) if (!seen[sg->seq_bytes[b]]) { seen[sg->seq_bytes[b]] = true; ++n_codes; }
    if (n_codes > kEdMaxCodes) return bad("group " + std::to_string(g) + ": " + std::to_string(n_codes) + " distinct bytes (at most 32)");
    group_codes[(size_t)g] = n_codes;
    max_codes = std::max(max_codes, n_codes);
    if (s1 - s0 <= 1) continue;
    for (int64_t s = s0; s < s1; ++s) {
      if (code_off[(size_t)s] >= 0) return bad("group " + std::to_string(g) + ": sequence " + std::to_string(s) + " lies in an earlier group too");
      code_off[(size_t)s] = code_bytes;
      code_bytes += ((sg->seq_off[s + 1] - sg->seq_off[s] + 63) / 64) * 64 + kEdPad;
    }
  }
  std::vector<uint8_t> codes((size_t)std::max<int64_t>(code_bytes, 64), 0xFF);
  std::vector<HostPair> hp;
  for (int64_t g = 0; g < sg->n_groups; ++g) {
    const int64_t s0 = sg->group_seq_off[g], s1 = sg->group_seq_off[g + 1], U = s1 - s0;
    if (U <= 1) continue;
    uint8_t map[256]; std::memset(map, 0xFF, sizeof(map));
    int next = 0;
    for (int64_t b = sg->seq_off[s0]; b < sg->seq_off[s1]; ++b) if (map[sg->seq_bytes[b]] == 0xFF) map[sg->seq_bytes[b]] = (uint8_t)next++;
    for (int64_t s = s0; s < s1; ++s)
      for (int64_t b = sg->seq_off[s], o = code_off[(size_t)s]; b < sg->seq_off[s + 1]; ++b, ++o) codes[(size_t)o] = map[sg->seq_bytes[b]];
    for (int64_t i = 0; i < U; ++i)
      for (int64_t j = i + 1; j < U; ++j) {
        const int64_t li = sg->seq_off[s0 + i + 1] - sg->seq_off[s0 + i], lj = sg->seq_off[s0 + j + 1] - sg->seq_off[s0 + j];
        const int64_t n = std::min(li, lj), m = std::max(li, lj);
        if (n == 0 || m - n >= cap) continue;                   // written by the host below
        if (m > INT32_MAX - 128) return bad("group " + std::to_string(g) + ": a sequence is too long");
        HostPair h;
        const int64_t a = li <= lj ? s0 + i : s0 + j, t = li <= lj ? s0 + j : s0 + i;
        h.d.pat_off = code_off[(size_t)a]; h.d.txt_off = code_off[(size_t)t]; h.d.n = (int32_t)n; h.d.m = (int32_t)m;
        h.at = dist_off[g] + i * U + j; h.mirror = dist_off[g] + j * U + i;
        const int64_t nb = (n + 63) / 64;
        h.lp_log2 = 0; h.n_codes = group_codes[(size_t)g];
        while (h.lp_log2 < 6 && ((int64_t)1 << h.lp_log2) < nb) ++h.lp_log2;
        hp.push_back(h);
      }
  }
  std::stable_sort(hp.begin(), hp.end(), [](const HostPair& a, const HostPair& b) { return a.lp_log2 != b.lp_log2 ? a.lp_log2 < b.lp_log2 : a.d.m < b.d.m; });
  std::vector<EdPair> pairs(hp.size());
  std::vector<EdWave> waves;
  int64_t strip_words = 0;
  bool any_multipass = false;
  for (size_t i = 0; i < hp.size();) {
    const int per_wave = 64 >> hp[i].lp_log2;
    size_t e = i;
    EdWave w; w.first_pair = (int32_t)i; w.lp_log2 = hp[i].lp_log2; w.max_m = 0; w.n_pass = 1; w.strip_off = -1; w.n_codes = 1;
    while (e < hp.size() && (int)(e - i) < per_wave && hp[e].lp_log2 == hp[i].lp_log2) { w.max_m = std::max(w.max_m, hp[e].d.m); w.n_codes = std::max(w.n_codes, hp[e].n_codes); ++e; }
    w.n_pairs = (int32_t)(e - i);
    if (hp[i].lp_log2 == 6) {
      w.n_pass = (hp[i].d.n + kEdPassRows - 1) / kEdPassRows;
      if (w.n_pass > 1) {
        any_multipass = true;
        if (w.max_m > kEdStripLdsCols) { w.strip_off = strip_words; strip_words += (w.max_m + 15) / 16; }
      }
    }
    waves.push_back(w);
    i = e;
  }
  for (size_t i = 0; i < hp.size(); ++i) pairs[i] = hp[i].d;
  if (hp.size() > (size_t)INT32_MAX || waves.size() > (size_t)INT32_MAX) return bad("too many pairs for one call");
  std::vector<int32_t> res(hp.size());
  if (!hp.empty()) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevLease lease(ctx, st);                                    // (codes, pairs, waves, res: declared before it)
    EdWave* d_waves = nullptr; EdPair* d_pairs = nullptr; uint8_t* d_codes = nullptr; uint32_t* d_strips = nullptr; int32_t* d_out = nullptr;
    DEV_TRY(ctx, lease.alloc(&d_waves, waves.size() * sizeof(EdWave)));
    DEV_TRY(ctx, lease.alloc(&d_pairs, pairs.size() * sizeof(EdPair)));
    DEV_TRY(ctx, lease.alloc(&d_codes, codes.size()));
    DEV_TRY(ctx, lease.alloc(&d_strips, (size_t)std::max<int64_t>(strip_words, 1) * 4));
    DEV_TRY(ctx, lease.alloc(&d_out, pairs.size() * 4));
    DEV_TRY(ctx, hipMemcpyAsync(d_waves, waves.data(), waves.size() * sizeof(EdWave), hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * sizeof(EdPair), hipMemcpyHostToDevice, st));
    DEV_TRY(ctx, hipMemcpyAsync(d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)max_codes * 64 * 8 + (any_multipass ? kEdStripLdsCols / 4 : 0);
    hipLaunchKernelGGL(ltr_editdist_kernel, dim3((unsigned)waves.size()), dim3(64), lds, st, d_waves, d_pairs, d_codes, d_strips, cap, (int32_t)max_codes, d_out);
    DEV_TRY(ctx, hipGetLastError());
    DEV_TRY(ctx, hipMemcpyAsync(res.data(), d_out, pairs.size() * 4, hipMemcpyDeviceToHost, st));
    DEV_TRY(ctx, lease.drain());
  }
  for (int64_t g = 0; g < sg->n_groups; ++g) {                  // the diagonal and the pairs the length difference decides
    const int64_t s0 = sg->group_seq_off[g], U = sg->group_seq_off[g + 1] - s0;
    int32_t* d = dist + dist_off[g];
    for (int64_t i = 0; i < U; ++i) {
      d[i * U + i] = 0;
      for (int64_t j = i + 1; j < U; ++j) {
        const int64_t li = sg->seq_off[s0 + i + 1] - sg->seq_off[s0 + i], lj = sg->seq_off[s0 + j + 1] - sg->seq_off[s0 + j];
        const int64_t n = std::min(li, lj), m = std::max(li, lj);
        if (n == 0 || m - n >= cap) d[i * U + j] = d[j * U + i] = (int32_t)std::min<int64_t>(m - n, cap);
      }
    }
  }
  for (size_t i = 0; i < hp.size(); ++i) dist[hp[i].at] = dist[hp[i].mirror] = res[i];
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

}  // extern "C"
