// ltr_poa.hip -- ltr_poa_consensus: the consensus of every group of sequences by partial-order alignment, the step
// HaplotypeGenerator::poa (HaplotypeGenerator.cpp:167-199, called at :427) hands to spoa.  This is the PUBLISHED method (Lee, Grasso &
// Sharlow 2002; heaviest-bundle consensus) with the scoring of :169 (global, linear gap, match +1, mismatch -1, gap -1) and every
// tie rule fixed (tests/poa_util.py); it is not spoa's bytes.
//
// Geometry: ONE wavefront owns a group from its first sequence to its consensus (a plain grid, one wavefront per workgroup, group
// = blockIdx.x: no work queue, no atomics, nothing between workgroups).  Per sequence s of m bases:
//   rows      one row of H per node, in topological order (Kahn, smallest ready id: a bitmap of ready nodes, searched 64 words
//             at a time from the lowest word that can hold one).  The lanes lie across the columns of s, 64 columns a block; a
//             row's predecessors (at most 30: one per sequence) sit one per lane and are broadcast; the horizontal term is a
//             max-scan of t[j] + j over the lanes with the block's carry, as tests/cluster_util.lev does with a min.
//   cells     the rows stay in the group's scratch block for the traceback: int16 while nodes + m <= 32767 is certain from the
//             group's sizes (|H[v][j]| <= nodes + m: every step changes H by one), else int32.
//   serial    traceback, adding the alignment and the consensus walk are one chain of dependent reads: every lane makes the same
//             reads and the same writes (same address, same value), so no lane reads what only another lane wrote; where lanes
//             write different cells (rows, fills) a barrier follows.
// Graph arrays (letters, edge lists sorted by predecessor id, the rings of aligned nodes, the ready bitmap): in LDS while they fit
// kPoaLdsGraphBytes, in the scratch block otherwise.  Every loop is bounded by a size known at launch.
// Memory rule: a group's scratch (graph arrays + score rows) is at most the per-group cap; the rows of one alignment take
// (nodes + 1) * (m + 1) cells, known only as the graph grows, so the wavefront tests it before every alignment and gives the group
// up (status 1) when it does not fit; groups are launched in sets whose blocks together stay within the per-call budget.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ltr_gpu.h"
#include "ltr_ctx.h"

namespace {

constexpr int kPoaMaxMembers = 30;                       // :171
constexpr int kPoaLdsGraphBytes = 16 << 10;              // graph arrays of at most this go to LDS (up to ten wavefronts a CU)
constexpr int64_t kPoaGroupCapBytes = (int64_t)512 << 20;     // see ltr_gpu.h for the arithmetic
constexpr int64_t kPoaCallBudgetBytes = (int64_t)16 << 30;
constexpr int kPoaNeg = -(1 << 29);
constexpr int kPoaOk = 0, kPoaOverCap = 1, kPoaInternal = 2;

// the graph arrays of a group with at most n nodes (and edges) and sequences of at most l bases, carved from one block
struct PoaGraph {
  int32_t *in_head, *out_head, *ring, *indeg, *work, *score, *cpred;       // [n] per node
  int32_t *e_from, *e_to, *e_next_in, *e_next_out, *e_w;                   // [n] per edge
  uint32_t* ready;                                                          // [(n + 31) / 32]
  int32_t* aln;                                                             // [l]
  uint8_t* letter;                                                          // [n]
};
__host__ __device__ inline int64_t poa_graph_bytes(int64_t n, int64_t l) {
  return 12 * 4 * n + 4 * ((n + 31) / 32) + 4 * l + ((n + 15) / 16) * 16;
}
__device__ inline PoaGraph poa_carve(uint8_t* base, int64_t n, int64_t l) {
  PoaGraph g;
  int32_t* p = reinterpret_cast<int32_t*>(base);
  g.in_head = p; p += n; g.out_head = p; p += n; g.ring = p; p += n; g.indeg = p; p += n; g.work = p; p += n; g.score = p; p += n; g.cpred = p; p += n;
  g.e_from = p; p += n; g.e_to = p; p += n; g.e_next_in = p; p += n; g.e_next_out = p; p += n; g.e_w = p; p += n;
  g.ready = reinterpret_cast<uint32_t*>(p); p += (n + 31) / 32;
  g.aln = p; p += l;
  g.letter = reinterpret_cast<uint8_t*>(p);
  return g;
}

struct PoaState {
  PoaGraph g;
  int n_nodes, n_edges, n_ub, lo;                         // lo: no ready node lies in a bitmap word below this one
};

__device__ __forceinline__ int poa_bcast(int v, int lane) { return __shfl(v, lane); }

// Kahn, smallest ready id first
__device__ inline void kahn_begin(PoaState& S, int lane) {
  const PoaGraph& g = S.g;
  const int words = (S.n_nodes + 31) >> 5;
  for (int w = lane; w < words; w += 64) {
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      const int v = w * 32 + b;
      if (v < S.n_nodes) { const int d = g.indeg[v]; g.work[v] = d; if (d == 0) bits |= 1u << b; }
    }
    g.ready[w] = bits;
  }
  S.lo = 0;
  __syncthreads();
}
__device__ inline int kahn_pop(PoaState& S, int lane) {
  const PoaGraph& g = S.g;
  const int words = (S.n_nodes + 31) >> 5;
  for (int base = S.lo; base < words; base += 64) {
    const int w = base + lane;
    const uint32_t word = w < words ? g.ready[w] : 0u;
    const unsigned long long mask = __ballot(word != 0u);
    if (mask) {
      const int first = __ffsll((long long)mask) - 1;
      const uint32_t sel = (uint32_t)poa_bcast((int)word, first);
      const int bit = __ffs((int)sel) - 1;
      g.ready[base + first] = sel & ~(1u << bit);
      S.lo = base + first;
      return (base + first) * 32 + bit;
    }
  }
  return -1;
}
__device__ inline void kahn_release(PoaState& S, int v) {
  const PoaGraph& g = S.g;
  int e = g.out_head[v];
  for (int k = 0; k <= kPoaMaxMembers && e >= 0; ++k) {
    const int to = g.e_to[e];
    const int left = g.work[to] - 1;
    g.work[to] = left;
    if (left == 0) { g.ready[to >> 5] |= 1u << (to & 31); S.lo = min(S.lo, to >> 5); }
    e = g.e_next_out[e];
  }
}

// one row of H: node v against the m bases of s
template <class CT> __device__ inline void poa_row(const PoaState& S, CT* H, const uint8_t* s, int m, int v, int lane) {
  const PoaGraph& g = S.g;
  int mine = 0, np = 0;                                       // the row (node + 1; 0 = the virtual row) of this lane's predecessor
  for (int e = g.in_head[v]; e >= 0 && np <= kPoaMaxMembers; e = g.e_next_in[e], ++np)
    if (lane == np) mine = g.e_from[e] + 1;
  if (np == 0) np = 1;
  const size_t stride = (size_t)m + 1;
  const int c = g.letter[v];
  int h0 = kPoaNeg;
  for (int k = 0; k < np; ++k) h0 = max(h0, (int)H[(size_t)poa_bcast(mine, k) * stride]);
  h0 -= 1;
  CT* const row = H + (size_t)(v + 1) * stride;
  row[0] = (CT)h0;
  int carry = h0;                                             // max over the columns so far of t[k] + k
  for (int base = 0; base < m; base += 64) {
    const int j = base + lane + 1;
    const bool on = j <= m;
    int best = kPoaNeg;
    const int sc = (on && s[j - 1] == c) ? 1 : -1;
    for (int k = 0; k < np; ++k) {
      const CT* hp = H + (size_t)poa_bcast(mine, k) * stride;   // (every lane takes part in the broadcast)
      if (on) best = max(best, max((int)hp[j - 1] + sc, (int)hp[j] - 1));
    }
    int x = on ? best + j : kPoaNeg;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x = max(x, y); }
    x = max(x, carry);
    if (on) row[j] = (CT)(x - j);
    carry = poa_bcast(x, 63);
  }
}

__device__ inline int poa_new_node(PoaState& S, int c) {
  const PoaGraph& g = S.g;
  const int v = S.n_nodes++;
  g.letter[v] = (uint8_t)c; g.in_head[v] = -1; g.out_head[v] = -1; g.ring[v] = v; g.indeg[v] = 0;
  return v;
}

// the edge a -> b walked once more; in-lists stay sorted by predecessor id.  false: the edge arrays are full (cannot happen: one edge per base)
__device__ inline bool poa_add_edge(PoaState& S, int a, int b) {
  const PoaGraph& g = S.g;
  int prev = -1, e = g.in_head[b];
  for (int k = 0; k <= kPoaMaxMembers && e >= 0; ++k) {
    const int f = g.e_from[e];
    if (f == a) { g.e_w[e] += 1; return true; }
    if (f > a) break;
    prev = e; e = g.e_next_in[e];
  }
  if (S.n_edges >= S.n_ub) return false;
  const int ne = S.n_edges++;
  g.e_from[ne] = a; g.e_to[ne] = b; g.e_w[ne] = 1;
  g.e_next_in[ne] = e;
  if (prev < 0) g.in_head[b] = ne; else g.e_next_in[prev] = ne;
  g.e_next_out[ne] = g.out_head[a]; g.out_head[a] = ne;
  g.indeg[b] += 1;
  return true;
}

// the bases of s onto the graph: aln[i] = the node base i is aligned to, or -1
__device__ inline bool poa_add_alignment(PoaState& S, const uint8_t* s, int m) {
  const PoaGraph& g = S.g;
  int prev = -1;
  for (int i = 0; i < m; ++i) {
    const int a = g.aln[i], c = s[i];
    int cur = -1;
    if (a >= 0) {
      if (g.letter[a] == c) cur = a;
      else {
        int x = g.ring[a];
        for (int k = 0; k < 256 && x != a; ++k) { if (g.letter[x] == c) { cur = x; break; } x = g.ring[x]; }
      }
    }
    if (cur < 0) {
      if (S.n_nodes >= S.n_ub) return false;
      cur = poa_new_node(S, c);
      if (a >= 0) { g.ring[cur] = g.ring[a]; g.ring[a] = cur; }
    }
    if (prev >= 0 && !poa_add_edge(S, prev, cur)) return false;
    prev = cur;
  }
  return true;
}

// the node without successors with the largest key (ties: the lowest id); key(v) read by the lanes side by side
template <class Key> __device__ inline int poa_best_end(const PoaState& S, int lane, const Key& key) {
  int best = kPoaNeg, at = INT32_MAX;
  for (int v = lane; v < S.n_nodes; v += 64)
    if (S.g.out_head[v] < 0) { const int k = key(v); if (k > best) { best = k; at = v; } }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int ob = __shfl_xor(best, d), oa = __shfl_xor(at, d);
    if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
  }
  return at;
}

template <class CT> __device__ inline int poa_align(PoaState& S, CT* H, const uint8_t* s, int m, int lane) {
  const PoaGraph& g = S.g;
  const size_t stride = (size_t)m + 1;
  for (int j = lane; j <= m; j += 64) H[j] = (CT)(-j);         // the virtual row
  kahn_begin(S, lane);
  for (int k = 0; k < S.n_nodes; ++k) {
    const int v = kahn_pop(S, lane);
    if (v < 0) return kPoaInternal;
    poa_row<CT>(S, H, s, m, v, lane);
    kahn_release(S, v);
    __syncthreads();
  }
  int v = poa_best_end(S, lane, [&](int u) { return (int)H[(size_t)(u + 1) * stride + m]; });
  if (v == INT32_MAX) return kPoaInternal;
  // traceback: diagonal over the predecessors in increasing id, then vertical likewise, then horizontal
  int j = m;
  const int max_steps = S.n_nodes + m + 2;
  for (int step = 0; step < max_steps && (v >= 0 || j > 0); ++step) {
    if (v < 0) { g.aln[--j] = -1; continue; }
    const CT* row = H + (size_t)(v + 1) * stride;
    const int h = row[j];
    const int sc = (j > 0 && s[j - 1] == g.letter[v]) ? 1 : -1;
    int move = 0, to = -1;                                     // 1 diagonal, 2 vertical
    const int first = g.in_head[v];
    if (j > 0) {
      if (first < 0) { if ((int)H[j - 1] + sc == h) move = 1; }
      else {
        int e = first;
        for (int k = 0; k <= kPoaMaxMembers && e >= 0; ++k) {
          const int p = g.e_from[e];
          if ((int)H[(size_t)(p + 1) * stride + j - 1] + sc == h) { move = 1; to = p; break; }
          e = g.e_next_in[e];
        }
      }
    }
    if (move == 0) {
      if (first < 0) { if ((int)H[j] - 1 == h) move = 2; }
      else {
        int e = first;
        for (int k = 0; k <= kPoaMaxMembers && e >= 0; ++k) {
          const int p = g.e_from[e];
          if ((int)H[(size_t)(p + 1) * stride + j] - 1 == h) { move = 2; to = p; break; }
          e = g.e_next_in[e];
        }
      }
    }
    if (move == 1) { g.aln[j - 1] = v; v = to; --j; }
    else if (move == 2) v = to;
    else { if (j <= 0) return kPoaInternal; g.aln[--j] = -1; }
  }
  if (v >= 0 || j > 0) return kPoaInternal;
  return poa_add_alignment(S, s, m) ? kPoaOk : kPoaInternal;
}

// heaviest bundle: per node the predecessor of the largest (edge weight, predecessor's score, lower id)
__device__ inline int poa_consensus(PoaState& S, uint8_t* out, int lane, int* out_len) {
  const PoaGraph& g = S.g;
  kahn_begin(S, lane);
  for (int k = 0; k < S.n_nodes; ++k) {
    const int v = kahn_pop(S, lane);
    if (v < 0) return kPoaInternal;
    int bw = -1, bs = -1, bp = -1, e = g.in_head[v];
    for (int q = 0; q <= kPoaMaxMembers && e >= 0; ++q) {
      const int p = g.e_from[e], w = g.e_w[e], sp = g.score[p];
      if (w > bw || (w == bw && sp > bs)) { bw = w; bs = sp; bp = p; }
      e = g.e_next_in[e];
    }
    g.score[v] = bp < 0 ? 0 : bs + bw;
    g.cpred[v] = bp;
    kahn_release(S, v);
  }
  __syncthreads();
  const int end = poa_best_end(S, lane, [&](int u) { return g.score[u]; });
  if (end == INT32_MAX) return kPoaInternal;
  int len = 0;
  for (int v = end, k = 0; v >= 0 && k < S.n_nodes; v = g.cpred[v], ++k) ++len;
  for (int v = end, k = len - 1; v >= 0 && k >= 0; v = g.cpred[v], --k) out[k] = g.letter[v];
  *out_len = len;
  return kPoaOk;
}

template <class CT> __device__ inline int poa_group(const ltrk::PoaGroup& G, const ltrk::PoaSeq* seqs, const uint8_t* bytes, PoaState& S, uint8_t* h_block,
                                                     uint8_t* out, int lane, int* out_len) {
  CT* const H = reinterpret_cast<CT*>(h_block);
  const ltrk::PoaSeq first = seqs[G.first_seq];
  for (int i = lane; i < first.len; i += 64) S.g.aln[i] = -1;
  __syncthreads();
  if (!poa_add_alignment(S, bytes + first.off, first.len)) return kPoaInternal;   // the first sequence is a chain
  for (int q = 1; q < G.n_members; ++q) {
    const ltrk::PoaSeq sq = seqs[G.first_seq + q];
    if (((int64_t)S.n_nodes + 1) * ((int64_t)sq.len + 1) * (int64_t)sizeof(CT) > G.h_bytes) return kPoaOverCap;
    const int rc = poa_align<CT>(S, H, bytes + sq.off, sq.len, lane);
    if (rc != kPoaOk) return rc;
  }
  return poa_consensus(S, out, lane, out_len);
}

__global__ __launch_bounds__(64) void ltr_poa_kernel(const ltrk::PoaGroup* __restrict__ groups, const ltrk::PoaSeq* __restrict__ seqs,
                                                     const uint8_t* __restrict__ bytes, uint8_t* scratch, uint8_t* out, int32_t* out_len,
                                                     int32_t* status) {
  extern __shared__ __align__(16) uint8_t poa_lds[];
  const int lane = threadIdx.x;
  const ltrk::PoaGroup G = groups[blockIdx.x];
  uint8_t* const block = scratch + G.scratch_off;
  PoaState S;
  S.g = poa_carve(G.graph_in_lds ? poa_lds : block, G.n_ub, G.l_max);
  S.n_nodes = 0; S.n_edges = 0; S.n_ub = G.n_ub; S.lo = 0;
  uint8_t* const h_block = block + (G.graph_in_lds ? 0 : G.graph_bytes);
  int len = 0;
  const int rc = G.wide ? poa_group<int32_t>(G, seqs, bytes, S, h_block, out + G.out_off, lane, &len)
                        : poa_group<int16_t>(G, seqs, bytes, S, h_block, out + G.out_off, lane, &len);
  if (lane == 0) { status[G.slot] = rc; out_len[G.slot] = rc == kPoaOk ? len : 0; }
}

}  // namespace

namespace ltrk {
void launch_poa(dim3 grid, size_t lds_bytes, hipStream_t st, const PoaGroup* groups, const PoaSeq* seqs, const uint8_t* bytes, uint8_t* scratch,
                uint8_t* out, int32_t* out_len, int32_t* status) {
  hipLaunchKernelGGL(ltr_poa_kernel, grid, dim3(64), lds_bytes, st, groups, seqs, bytes, scratch, out, out_len, status);
}
}  // namespace ltrk

namespace {

// the members a group's alignment takes (tests/poa_util.used_members): empty ones dropped, of more than 30 those at floor(k n / 30)
void poa_used_members(const ltr_seq_groups* sg, int64_t g, std::vector<int64_t>* used) {
  used->clear();
  for (int64_t s = sg->group_seq_off[g]; s < sg->group_seq_off[g + 1]; ++s) if (sg->seq_off[s + 1] > sg->seq_off[s]) used->push_back(s);
  const int64_t n = (int64_t)used->size();
  if (n > kPoaMaxMembers) {
    std::vector<int64_t> pick;
    for (int64_t k = 0; k < kPoaMaxMembers; ++k) pick.push_back((*used)[(size_t)((k * n) / kPoaMaxMembers)]);
    used->swap(pick);
  }
}

// LTR_OK, or LTR_ERR_INVALID with *msg
int poa_check(const ltr_seq_groups* sg, std::string* msg) {
  if (!sg || sg->n_groups < 0 || sg->n_seqs < 0) { *msg = "bad arguments"; return LTR_ERR_INVALID; }
  if (sg->n_groups == 0) return LTR_OK;
  if (!sg->group_seq_off || !sg->seq_off || (sg->seq_off[sg->n_seqs] > 0 && !sg->seq_bytes)) { *msg = "null array"; return LTR_ERR_INVALID; }
  for (int64_t s = 0; s < sg->n_seqs; ++s)
    if (sg->seq_off[s] < 0 || sg->seq_off[s + 1] < sg->seq_off[s]) { *msg = "sequence offsets of sequence " + std::to_string(s) + " are not ascending"; return LTR_ERR_INVALID; }
  for (int64_t g = 0; g < sg->n_groups; ++g) {
    const int64_t s0 = sg->group_seq_off[g], s1 = sg->group_seq_off[g + 1];
    if (s0 < 0 || s1 < s0 || s1 > sg->n_seqs) { *msg = "group " + std::to_string(g) + ": sequence range out of bounds"; return LTR_ERR_INVALID; }
  }
  return LTR_OK;
}

int64_t poa_capacity(const ltr_seq_groups* sg) {
  int64_t cap = 0;
  for (int64_t g = 0; g < sg->n_groups; ++g) cap += sg->seq_off[sg->group_seq_off[g + 1]] - sg->seq_off[sg->group_seq_off[g]];
  return cap;
}

}  // namespace

extern "C" {

int64_t ltr_poa_consensus_capacity(const ltr_seq_groups* sg) {
  std::string msg;
  if (poa_check(sg, &msg) != LTR_OK) return LTR_ERR_INVALID;
  return poa_capacity(sg);
}

int ltr_poa_consensus(ltr_ctx* ctx, const ltr_seq_groups* sg, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off, uint8_t* status) {
  if (!ctx) return LTR_ERR_NO_DEVICE;                           // (a context exists only on a device: there is no CPU fallback)
  std::lock_guard<std::mutex> lk(ctx->mu);
  LTR_GUARD_BEGIN
  auto bad = [&](const std::string& msg) { ltr::set_error(ctx, "ltr_poa_consensus: " + msg); return LTR_ERR_INVALID; };
  std::string msg;
  if (poa_check(sg, &msg) != LTR_OK) return bad(msg);
  if (sg->n_groups == 0) return LTR_OK;
  if (!out_off || !status || out_cap < 0 || (out_cap > 0 && !out_bytes)) return bad("null array");
  if (out_cap < poa_capacity(sg)) return bad("out_cap " + std::to_string(out_cap) + " is below ltr_poa_consensus_capacity = " + std::to_string(poa_capacity(sg)));
  const ltr::DebugKnobs dbg = ctx->dbg;
  const int64_t budget = dbg.poa_call_budget_bytes > 0 ? dbg.poa_call_budget_bytes : kPoaCallBudgetBytes;
  const int64_t cap = std::min(dbg.poa_group_cap_bytes > 0 ? dbg.poa_group_cap_bytes : kPoaGroupCapBytes, budget);
  // per group: its members; one member (or none) is the answer itself, the others are laid out for the launch
  struct HostGroup { ltrk::PoaGroup d; int64_t group; int64_t block_bytes; };
  std::vector<HostGroup> hg;
  std::vector<ltrk::PoaSeq> seqs;
  std::vector<std::string> result((size_t)sg->n_groups);
  std::vector<uint8_t> st((size_t)sg->n_groups, 0);
  std::vector<int64_t> used;
  for (int64_t g = 0; g < sg->n_groups; ++g) {
    poa_used_members(sg, g, &used);
    if (used.size() <= 1) {
      if (used.size() == 1) result[(size_t)g].assign((const char*)sg->seq_bytes + sg->seq_off[used[0]], (size_t)(sg->seq_off[used[0] + 1] - sg->seq_off[used[0]]));
      continue;
    }
    int64_t n_ub = 0, l_max = 0;
    for (int64_t s : used) { const int64_t len = sg->seq_off[s + 1] - sg->seq_off[s]; n_ub += len; l_max = std::max(l_max, len); }
    HostGroup h;
    h.group = g;
    const int64_t graph = ((poa_graph_bytes(n_ub, l_max) + 255) / 256) * 256;
    const bool lds = graph <= kPoaLdsGraphBytes;
    const bool wide = n_ub + l_max > 32767;
    if (n_ub > (int64_t)1 << 30 || (!lds && graph > cap)) { st[(size_t)g] = 1; continue; }     // the graph arrays alone are over the cap
    // rows: at most (nodes before the last sequence + 1) x (longest + 1) cells, and never more than the cap leaves
    const int64_t h_ub = (n_ub + 1) * (l_max + 1) * (wide ? 4 : 2);
    const int64_t h_bytes = std::min(h_ub, cap - (lds ? 0 : graph));
    h.d.first_seq = (int64_t)seqs.size(); h.d.scratch_off = 0; h.d.out_off = 0;
    h.d.h_bytes = h_bytes; h.d.graph_bytes = graph;
    h.d.n_members = (int32_t)used.size(); h.d.n_ub = (int32_t)n_ub; h.d.l_max = (int32_t)l_max; h.d.wide = wide ? 1 : 0; h.d.graph_in_lds = lds ? 1 : 0; h.d.slot = 0;
    h.block_bytes = (((lds ? 0 : graph) + h_bytes + 255) / 256) * 256;
    for (int64_t s : used) { ltrk::PoaSeq q; q.off = sg->seq_off[s]; q.len = (int32_t)(sg->seq_off[s + 1] - sg->seq_off[s]); q.pad = 0; seqs.push_back(q); }
    hg.push_back(h);
  }
  if (!hg.empty()) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const int64_t n_bytes = sg->seq_off[sg->n_seqs];
    std::vector<ltrk::PoaGroup> set;
    std::vector<uint8_t> h_out;
    std::vector<int32_t> h_len, h_status;
    for (size_t i = 0; i < hg.size();) {                        // launch sets: as many groups as the budget holds, at least one
      size_t e = i;
      int64_t scratch_bytes = 0, out_bytes_set = 0;
      size_t lds_bytes = 0;
      set.clear();
      while (e < hg.size() && (e == i || scratch_bytes + hg[e].block_bytes <= budget)) {
        ltrk::PoaGroup d = hg[e].d;
        d.scratch_off = scratch_bytes; d.out_off = out_bytes_set; d.slot = (int32_t)(e - i);
        scratch_bytes += hg[e].block_bytes; out_bytes_set += d.n_ub;
        if (d.graph_in_lds) lds_bytes = std::max(lds_bytes, (size_t)d.graph_bytes);
        set.push_back(d);
        ++e;
      }
      h_out.resize((size_t)out_bytes_set); h_len.resize(set.size()); h_status.resize(set.size());
      {
        DevLease lease(ctx, stream);                            // (set, seqs, h_out, h_len, h_status: declared before it)
        ltrk::PoaGroup* d_groups = nullptr; ltrk::PoaSeq* d_seqs = nullptr; uint8_t* d_bytes = nullptr; uint8_t* d_scratch = nullptr; uint8_t* d_out = nullptr;
        int32_t* d_len = nullptr; int32_t* d_status = nullptr;
        DEV_TRY(ctx, lease.alloc(&d_groups, set.size() * sizeof(ltrk::PoaGroup)));
        DEV_TRY(ctx, lease.alloc(&d_seqs, seqs.size() * sizeof(ltrk::PoaSeq)));
        DEV_TRY(ctx, lease.alloc(&d_bytes, (size_t)std::max<int64_t>(n_bytes, 1)));
        DEV_TRY(ctx, lease.alloc(&d_scratch, (size_t)std::max<int64_t>(scratch_bytes, 256)));
        DEV_TRY(ctx, lease.alloc(&d_out, (size_t)std::max<int64_t>(out_bytes_set, 1)));
        DEV_TRY(ctx, lease.alloc(&d_len, set.size() * 4));
        DEV_TRY(ctx, lease.alloc(&d_status, set.size() * 4));
        DEV_TRY(ctx, hipMemcpyAsync(d_groups, set.data(), set.size() * sizeof(ltrk::PoaGroup), hipMemcpyHostToDevice, stream));
        DEV_TRY(ctx, hipMemcpyAsync(d_seqs, seqs.data(), seqs.size() * sizeof(ltrk::PoaSeq), hipMemcpyHostToDevice, stream));
        DEV_TRY(ctx, hipMemcpyAsync(d_bytes, sg->seq_bytes, (size_t)n_bytes, hipMemcpyHostToDevice, stream));
        DEV_TRY(ctx, hipMemsetAsync(d_status, 0xFF, set.size() * 4, stream));
        ltrk::launch_poa(dim3((unsigned)set.size()), lds_bytes, stream, d_groups, d_seqs, d_bytes, d_scratch, d_out, d_len, d_status);
        DEV_TRY(ctx, hipGetLastError());
        DEV_TRY(ctx, hipMemcpyAsync(h_out.data(), d_out, (size_t)out_bytes_set, hipMemcpyDeviceToHost, stream));
        DEV_TRY(ctx, hipMemcpyAsync(h_len.data(), d_len, set.size() * 4, hipMemcpyDeviceToHost, stream));
        DEV_TRY(ctx, hipMemcpyAsync(h_status.data(), d_status, set.size() * 4, hipMemcpyDeviceToHost, stream));
        DEV_TRY(ctx, lease.drain());
      }
      for (size_t k = 0; k < set.size(); ++k) {
        const int64_t g = hg[i + k].group;
        if (h_status[k] == kPoaOverCap) st[(size_t)g] = 1;
        else if (h_status[k] != kPoaOk || h_len[k] < 0 || h_len[k] > set[k].n_ub) {
          ltr::set_error(ctx, "ltr_poa_consensus: group " + std::to_string(g) + ": the kernel gave up (status " + std::to_string(h_status[k]) + ")");
          return LTR_ERR_HIP;
        } else result[(size_t)g].assign((const char*)h_out.data() + set[k].out_off, (size_t)h_len[k]);
      }
      i = e;
    }
  }
  int64_t at = 0;
  for (int64_t g = 0; g < sg->n_groups; ++g) {
    out_off[g] = at;
    if (!result[(size_t)g].empty()) std::memcpy(out_bytes + at, result[(size_t)g].data(), result[(size_t)g].size());
    at += (int64_t)result[(size_t)g].size();
    status[g] = st[(size_t)g];
  }
  out_off[sg->n_groups] = at;
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

}  // extern "C"
