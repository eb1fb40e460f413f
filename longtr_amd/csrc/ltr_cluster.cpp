// ltr_cluster.cpp -- the clustering step of HaplotypeGenerator::gen_candidate_seqs (src/SeqAlignment/HaplotypeGenerator.cpp:376-472):
// the reads of a sample whose repeat sequence is no candidate allele are clustered by edit distance, the cluster centres become
// inexact alleles.  Host code on a distance matrix; the matrix comes from ltr_edit_distances (ltr_editdist.hip).
//   greedy_clustering        :237-268
//   merge_clusters           :271-293
//   the threshold ladder, refinement, acceptance   :397-470
// The centre of a cluster (poa, :427; spoa, un-vendored, sampling its input with std::random_device) comes in two forms:
//   ltr_cluster_sequences, ltr_build_haplotypes_clustered   the cluster's MEDOID, the member with the smallest count-weighted sum of
//       distances to the members: deterministic and one of the reads, errors included (the documented deviation of these two)
//   ltr_build_haplotypes_consensus   the partial-order-alignment consensus of its members by the published method with every tie rule
//       fixed (ltr_poa_consensus, ltr_poa.hip): not spoa's bytes; the refinement then runs in rounds over all groups of the call
// needleman_wunsch(a, b, score, T) (:201-234) is not run: for T <= 700, score < T <=> d(a, b) < T, and the score is the distance
// whenever it is < T (its row test :225-230 is a lower bound of the final distance).  One exception is reproduced by argument
// position: with an empty SECOND argument and a non-empty first the inner loop never runs and the answer is T + 1 (nw_below).
#include <algorithm>
#include <climits>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ltr_internal.h"
#include "ltr_prep.h"

struct ltr_cluster_result {
  int32_t threshold = -1;
  std::vector<std::vector<int32_t>> members;                    // caller's indices, in the order the reference's vectors hold them
  std::vector<int32_t> centroid;                                // ... of the centre, -1 where it is none of the sequences (a consensus)
  std::vector<std::string> centre;
  std::vector<uint8_t> is_new, counted;
};

namespace {

const int kThresholds[] = {20, 50, 80, 100, 150, 200, 300, 400, 500, 600, 700};   // :405
const int kNumThresholds = (int)(sizeof(kThresholds) / sizeof(kThresholds[0]));
const int kMaxCentroids = 15;                                                      // :261
const int32_t kClusterCap = 701;

// The one owner of the greedy step, the merge and the acceptance.  Where a cluster's centre comes from -- its medoid (run) or
// its partial-order-alignment consensus (ltr_build_haplotypes_consensus, which drives the same steps in rounds) -- is the caller's.
struct Clusterer {
  const std::vector<std::string>& seqs;
  const int32_t* counts;
  const int32_t* dist;
  const int32_t U;
  int64_t ignored = 0;
  std::vector<int32_t> lex_rank, ls_rank, by_lex;               // rank of each sequence in std::map order / in length-then-sequence order
  typedef std::map<std::string, std::vector<int32_t>> Clusters; // key: the centroid, as the reference's std::map<std::string, ..>

  Clusterer(const std::vector<std::string>& s, const int32_t* c, const int32_t* d) : seqs(s), counts(c), dist(d), U((int32_t)s.size()) {
    std::vector<int32_t> ls((size_t)U);
    by_lex.resize((size_t)U);
    for (int32_t i = 0; i < U; ++i) { by_lex[(size_t)i] = ls[(size_t)i] = i; ignored += counts[i]; }
    std::sort(by_lex.begin(), by_lex.end(), [&](int32_t x, int32_t y) { return seqs[(size_t)x] < seqs[(size_t)y]; });
    std::sort(ls.begin(), ls.end(), [&](int32_t x, int32_t y) { return ltr::by_len_seq(seqs[(size_t)x], seqs[(size_t)y]); });
    lex_rank.resize((size_t)U); ls_rank.resize((size_t)U);
    for (int32_t r = 0; r < U; ++r) { lex_rank[(size_t)by_lex[(size_t)r]] = r; ls_rank[(size_t)ls[(size_t)r]] = r; }
  }
  int32_t index_of(const std::string& s) const {                // the sequence equal to s, or -1
    auto it = std::lower_bound(by_lex.begin(), by_lex.end(), s, [&](int32_t x, const std::string& v) { return seqs[(size_t)x] < v; });
    return (it != by_lex.end() && seqs[(size_t)*it] == s) ? *it : -1;
  }
  // needleman_wunsch(a, b, score, T) from d = min(distance, 701): is score < T?  (*score = the score when it is)
  static bool nw_below(const std::string& a, const std::string& b, int32_t d, int T, int* score) {
    if (b.empty() && !a.empty()) return false;                  // min_score_per_row stays 1000: T + 1
    *score = d;
    return d < T;
  }
  std::vector<int32_t> first_order() const {                    // :399-403: the first std::map key stays first
    std::vector<int32_t> order = by_lex;
    std::sort(order.begin() + 1, order.end(), [&](int32_t x, int32_t y) { return ls_rank[(size_t)x] < ls_rank[(size_t)y]; });
    return order;
  }
  bool greedy(const std::vector<int32_t>& order, Clusters& clusters, int T) const {      // :237-268
    std::vector<int32_t> centroids{order[0]};
    clusters[seqs[(size_t)order[0]]].push_back(order[0]);
    for (size_t i = 1; i < order.size(); ++i) {
      int min_score = INT_MAX, min_cntr = -1;
      for (size_t j = 0; j < centroids.size(); ++j) {
        int score = -1;
        if (nw_below(seqs[(size_t)order[i]], seqs[(size_t)centroids[j]], dist[(size_t)order[i] * (size_t)U + (size_t)centroids[j]], T, &score) && score < min_score) { min_cntr = (int)j; min_score = score; }
      }
      if (min_cntr != -1) clusters[seqs[(size_t)centroids[(size_t)min_cntr]]].push_back(order[i]);
      else {
        centroids.push_back(order[i]);
        if ((int)centroids.size() > kMaxCentroids) return false;
        clusters[seqs[(size_t)order[i]]].push_back(order[i]);
      }
    }
    return true;
  }
  int32_t medoid(const std::vector<int32_t>& members) const {   // stands in for poa (:427)
    int32_t best = -1; int64_t best_sum = 0;
    for (int32_t x : members) {
      int64_t sum = 0;
      for (int32_t y : members) sum += (int64_t)counts[y] * dist[(size_t)x * (size_t)U + (size_t)y];
      if (best < 0 || sum < best_sum || (sum == best_sum && ls_rank[(size_t)x] < ls_rank[(size_t)best])) { best = x; best_sum = sum; }
    }
    return best;
  }
  // :424-437: every cluster (in std::map order) takes its new centre centres[c]; equal centres fold into one cluster (:428-434);
  // the centres are sorted from the second on (:437)
  void recentre(const Clusters& clusters, const std::vector<std::string>& centres, Clusters* updated, std::vector<std::string>* cents) const {
    size_t c = 0;
    for (const auto& kv : clusters) {
      const std::string& centre = centres[c++];
      std::vector<int32_t>& dst = (*updated)[centre];
      if (std::find(cents->begin(), cents->end(), centre) == cents->end()) { cents->push_back(centre); dst = kv.second; }
      else dst.insert(dst.end(), kv.second.begin(), kv.second.end());
    }
    std::sort(cents->begin() + 1, cents->end(), ltr::by_len_seq);
  }
  // d(i, j) = min(distance of cents[i] and cents[j], 701)
  template <class D> bool merge(const std::vector<std::string>& cents, Clusters& clusters, int T, const D& d) const {       // :271-293
    bool updated = false;
    for (size_t i = 0; i < cents.size(); ++i)
      for (size_t j = 1; j < cents.size(); ++j)
        if (i != j && clusters.count(cents[i]) && clusters.count(cents[j])) {
          int score = -1;
          if (nw_below(cents[i], cents[j], d(i, j), T, &score)) {
            updated = true;
            std::vector<int32_t>& dst = clusters[cents[i]];
            const std::vector<int32_t> src = clusters[cents[j]];
            dst.insert(dst.end(), src.begin(), src.end());
            clusters.erase(cents[j]);
          }
        }
    return updated;
  }
  bool accept(const Clusters& clusters, int T, ltr_cluster_result* out) const {          // :446-469 (who is a new allele: flag_new)
    int64_t covered = 0;
    std::vector<uint8_t> counted;
    for (const auto& kv : clusters) {
      int64_t sum = 0;
      for (int32_t y : kv.second) sum += counts[y];
      const bool big = sum > std::min<int64_t>((int)((double)ignored * 0.10), 10);
      if (big) covered += sum;
      counted.push_back(big ? 1 : 0);
    }
    if (covered < (int)(0.80 * (double)ignored)) return false;
    out->threshold = T;
    for (const auto& kv : clusters) { out->centre.push_back(kv.first); out->centroid.push_back(index_of(kv.first)); out->members.push_back(kv.second); }
    out->counted = counted;
    return true;
  }
  template <class IsCandidate> static void flag_new(const IsCandidate& is_candidate, ltr_cluster_result* out) {             // :457-458
    out->is_new.clear();
    for (size_t c = 0; c < out->centre.size(); ++c) out->is_new.push_back(out->counted[c] && !is_candidate(out->centre[c]) ? 1 : 0);
  }
  // the ladder with the medoid as a cluster's centre
  template <class IsCandidate> void run(const IsCandidate& is_candidate, ltr_cluster_result* out) const {
    out->threshold = -1;
    if (U == 0) return;
    const std::vector<int32_t> order = first_order();
    for (int T : kThresholds) {
      Clusters clusters;
      if (!greedy(order, clusters, T)) continue;
      for (bool not_converged = true; not_converged;) {          // :418-440
        Clusters updated;
        std::vector<std::string> centres, cents;
        for (const auto& kv : clusters) centres.push_back(seqs[(size_t)medoid(kv.second)]);
        recentre(clusters, centres, &updated, &cents);
        not_converged = merge(cents, updated, T, [&](size_t i, size_t j) { return dist[(size_t)index_of(cents[i]) * (size_t)U + (size_t)index_of(cents[j])]; });
        clusters.swap(updated);
      }
      if (accept(clusters, T, out)) { flag_new(is_candidate, out); return; }
    }
  }
};

// the unique sequences of a list and how often each occurs, in std::map order
void unique_counts(const std::vector<std::string>& all, const std::vector<std::string>& candidates, std::vector<std::string>* seqs, std::vector<int32_t>* counts) {
  std::map<std::string, int32_t> m;
  for (const std::string& s : all) if (std::find(candidates.begin(), candidates.end(), s) == candidates.end()) m[s] += 1;
  for (const auto& kv : m) { seqs->push_back(kv.first); counts->push_back(kv.second); }
}

}  // namespace

extern "C" {

int ltr_cluster_sequences(const uint8_t* seq_bytes, const int64_t* seq_off, const int32_t* counts, int32_t n_seqs, const int32_t* dist,
                          const uint8_t* cand_bytes, const int64_t* cand_off, int32_t n_cands, ltr_cluster_result** out) {
  if (!out || n_seqs < 0 || n_cands < 0 || (n_seqs > 0 && (!seq_off || !counts || !dist)) || (n_cands > 0 && !cand_off)) return LTR_ERR_INVALID;
  *out = nullptr;
  try {
    std::vector<std::string> seqs, cands;
    for (int32_t i = 0; i < n_seqs; ++i) {
      if (seq_off[i] < 0 || seq_off[i + 1] < seq_off[i] || counts[i] < 1 || (seq_off[i + 1] > seq_off[i] && !seq_bytes)) return LTR_ERR_INVALID;
      seqs.emplace_back((const char*)seq_bytes + seq_off[i], (size_t)(seq_off[i + 1] - seq_off[i]));
    }
    for (int32_t i = 0; i < n_cands; ++i) {
      if (cand_off[i] < 0 || cand_off[i + 1] < cand_off[i] || (cand_off[i + 1] > cand_off[i] && !cand_bytes)) return LTR_ERR_INVALID;
      cands.emplace_back((const char*)cand_bytes + cand_off[i], (size_t)(cand_off[i + 1] - cand_off[i]));
    }
    {
      std::vector<std::string> sorted = seqs;
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return LTR_ERR_INVALID;     // the keys of a std::map
    }
    for (int64_t k = 0; k < (int64_t)n_seqs * n_seqs; ++k) if (dist[k] < 0) return LTR_ERR_INVALID;
    std::unique_ptr<ltr_cluster_result> res(new ltr_cluster_result());
    Clusterer(seqs, counts, dist).run([&](const std::string& s) { return std::find(cands.begin(), cands.end(), s) != cands.end(); }, res.get());
    *out = res.release();
    return LTR_OK;
  } catch (const std::bad_alloc&) { return LTR_ERR_NOMEM; } catch (...) { return LTR_ERR_INVALID; }
}
int32_t ltr_cluster_result_threshold(const ltr_cluster_result* r) { return r ? r->threshold : -1; }
int32_t ltr_cluster_result_n_clusters(const ltr_cluster_result* r) { return r ? (int32_t)r->centroid.size() : 0; }
const int32_t* ltr_cluster_result_centroids(const ltr_cluster_result* r) { return r && !r->centroid.empty() ? r->centroid.data() : nullptr; }
const uint8_t* ltr_cluster_result_new_allele(const ltr_cluster_result* r) { return r && !r->is_new.empty() ? r->is_new.data() : nullptr; }
const uint8_t* ltr_cluster_result_counted(const ltr_cluster_result* r) { return r && !r->counted.empty() ? r->counted.data() : nullptr; }
const int32_t* ltr_cluster_result_members(const ltr_cluster_result* r, int32_t cluster, int32_t* n) {
  if (!r || cluster < 0 || cluster >= (int32_t)r->members.size()) { if (n) *n = 0; return nullptr; }
  if (n) *n = (int32_t)r->members[(size_t)cluster].size();
  return r->members[(size_t)cluster].data();
}
void ltr_cluster_result_free(ltr_cluster_result* r) { delete r; }

}  // extern "C"

namespace {

// a sample that needs clustering: its unique unplaced sequences; with the consensus as the centre also what the rounds left
struct Group {
  std::vector<std::string> seqs; std::vector<int32_t> counts; int32_t sample = 0; int64_t dist_off = 0;
  ltr_cluster_result cr; int32_t rounds = 0, medoid_kept = 0;
};

// The refinement (:418-440) with the consensus of a cluster as its centre, for all groups of a call at once.  A consensus is none of
// the group's sequences, so the merge needs distances the group's matrix does not hold: the loop runs as rounds --
//   host   per group that starts a threshold: the ladder step and greedy_clustering (a 16th centroid: the next threshold)
//   GPU    ONE ltr_poa_consensus call over every cluster of every group in refinement whose ordered member list has not been
//          aligned before in this call (the reference aligns unchanged clusters again; the method is deterministic)
//   GPU    ONE ltr_edit_distances call, cap 701, over each group's new centres (equal ones folded, sorted from the second on)
//   host   merge_clusters; a group that merged stays in refinement, the others go to acceptance, and on to the next threshold
//          when they do not pass
// A cluster over the memory cap of ltr_poa_consensus keeps its medoid.  Who is a new allele is decided afterwards, per locus in sample order.
int consensus_rounds(ltr_ctx* ctx, const std::vector<Group*>& groups, const int32_t* dist) {
  struct State {
    Group* g; Clusterer cl; std::vector<int32_t> order; int t_idx = 0; bool refining = false, done = false;
    Clusterer::Clusters clusters, updated;
    std::vector<std::string> cents;
    std::map<std::vector<int32_t>, std::pair<std::string, bool>> centre_of;   // ordered member list -> (centre, it is the medoid)
    std::map<std::string, bool> kept;                            // centres of the last round that are medoids
    State(Group* grp, const int32_t* d) : g(grp), cl(grp->seqs, grp->counts.data(), d) {}
  };
  std::vector<std::unique_ptr<State>> st;
  for (Group* g : groups) {
    g->cr = ltr_cluster_result(); g->rounds = 0; g->medoid_kept = 0;
    if (g->seqs.empty()) continue;
    st.emplace_back(new State(g, dist + g->dist_off));
    st.back()->order = st.back()->cl.first_order();
  }
  for (;;) {
    bool any = false;
    for (auto& sp : st) {                                       // the ladder step and the greedy clustering
      State& s = *sp;
      while (!s.done && !s.refining) {
        if (s.t_idx >= kNumThresholds) { s.done = true; break; }
        s.clusters.clear();
        if (s.cl.greedy(s.order, s.clusters, kThresholds[s.t_idx])) s.refining = true; else ++s.t_idx;
      }
      any = any || s.refining;
    }
    if (!any) break;
    // the consensus of every cluster that has none yet
    std::vector<std::pair<State*, const std::vector<int32_t>*>> asked;
    std::vector<int64_t> group_seq_off{0}, seq_off{0};
    std::vector<uint8_t> bytes;
    for (auto& sp : st) {
      State& s = *sp;
      if (!s.refining) continue;
      std::set<std::vector<int32_t>> in_this_round;
      for (const auto& kv : s.clusters) {
        if (s.centre_of.count(kv.second) || !in_this_round.insert(kv.second).second) continue;
        for (int32_t x : kv.second) { const std::string& q = s.g->seqs[(size_t)x]; bytes.insert(bytes.end(), q.begin(), q.end()); seq_off.push_back((int64_t)bytes.size()); }
        group_seq_off.push_back((int64_t)seq_off.size() - 1);
        asked.emplace_back(&s, &kv.second);
      }
    }
    if (!asked.empty()) {
      if (bytes.empty()) bytes.push_back(0);
      ltr_seq_groups sg;
      sg.n_groups = (int64_t)asked.size(); sg.group_seq_off = group_seq_off.data(); sg.n_seqs = (int64_t)seq_off.size() - 1;
      sg.seq_bytes = bytes.data(); sg.seq_off = seq_off.data();
      const int64_t cap = ltr_poa_consensus_capacity(&sg);
      std::vector<uint8_t> cons((size_t)std::max<int64_t>(cap, 1)), status(asked.size());
      std::vector<int64_t> off(asked.size() + 1);
      const int rc = ltr_poa_consensus(ctx, &sg, cons.data(), cap, off.data(), status.data());
      if (rc != LTR_OK) return rc;
      for (size_t a = 0; a < asked.size(); ++a) {
        State& s = *asked[a].first;
        const std::vector<int32_t>& members = *asked[a].second;
        if (status[a]) s.centre_of[members] = std::make_pair(s.g->seqs[(size_t)s.cl.medoid(members)], true);
        else s.centre_of[members] = std::make_pair(std::string((const char*)cons.data() + off[a], (size_t)(off[a + 1] - off[a])), false);
      }
    }
    // the new centres of every group, and their distances
    std::vector<State*> measured;
    std::vector<int64_t> dist_off;
    int64_t dist_size = 0;
    group_seq_off.assign(1, 0); seq_off.assign(1, 0); bytes.clear();
    for (auto& sp : st) {
      State& s = *sp;
      if (!s.refining) continue;
      std::vector<std::string> centres;
      s.updated.clear(); s.cents.clear(); s.kept.clear();
      for (const auto& kv : s.clusters) {
        const std::pair<std::string, bool>& c = s.centre_of[kv.second];
        centres.push_back(c.first);
        s.kept.emplace(c.first, c.second);                      // (the first cluster of a centre decides, as it owns the folded cluster)
      }
      s.cl.recentre(s.clusters, centres, &s.updated, &s.cents);
      if (s.cents.size() < 2) continue;
      for (const std::string& q : s.cents) { bytes.insert(bytes.end(), q.begin(), q.end()); seq_off.push_back((int64_t)bytes.size()); }
      group_seq_off.push_back((int64_t)seq_off.size() - 1);
      dist_off.push_back(dist_size);
      dist_size += (int64_t)s.cents.size() * (int64_t)s.cents.size();
      measured.push_back(&s);
    }
    std::vector<int32_t> cdist((size_t)std::max<int64_t>(dist_size, 1), 0);
    if (!measured.empty()) {
      if (bytes.empty()) bytes.push_back(0);
      ltr_seq_groups sg;
      sg.n_groups = (int64_t)measured.size(); sg.group_seq_off = group_seq_off.data(); sg.n_seqs = (int64_t)seq_off.size() - 1;
      sg.seq_bytes = bytes.data(); sg.seq_off = seq_off.data();
      const int rc = ltr_edit_distances(ctx, &sg, kClusterCap, cdist.data(), dist_off.data());
      if (rc != LTR_OK) return rc;
    }
    // merge; acceptance of the groups that did not merge
    size_t m = 0;
    for (auto& sp : st) {
      State& s = *sp;
      if (!s.refining) continue;
      const int T = kThresholds[s.t_idx];
      bool merged = false;
      if (s.cents.size() >= 2) {
        const int32_t* d = cdist.data() + dist_off[m++];
        const size_t C = s.cents.size();
        merged = s.cl.merge(s.cents, s.updated, T, [&](size_t i, size_t j) { return d[i * C + j]; });
      }
      s.g->rounds += 1;
      s.clusters.swap(s.updated);
      if (merged) continue;
      s.refining = false;
      if (s.cl.accept(s.clusters, T, &s.g->cr)) {
        s.done = true;
        for (const std::string& c : s.g->cr.centre) { auto it = s.kept.find(c); if (it != s.kept.end() && it->second) s.g->medoid_kept += 1; }
      } else ++s.t_idx;
    }
  }
  return LTR_OK;
}

int build_haplotypes_clustering(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len, ltr_hap_result** out, bool consensus) {
  const std::string name = consensus ? "ltr_build_haplotypes_consensus" : "ltr_build_haplotypes_clustered";
  if (!out || n_loci < 0 || (n_loci > 0 && !loci) || indel_flank_len < 0) return LTR_ERR_INVALID;
  for (int64_t l = 0; l < n_loci; ++l) out[l] = nullptr;
  if (!ctx) return LTR_ERR_NO_DEVICE;
  for (int64_t l = 0; l < n_loci; ++l)
    if (!loci[l].rs || loci[l].n_samples <= 0 || !loci[l].chrom_seq || loci[l].period < 1) { ltr::set_error(ctx, name + ": bad locus " + std::to_string(l)); return LTR_ERR_INVALID; }
  ltr::TimedCall timed(ctx, ltr::kTimerHapBuild);
  LTR_GUARD_BEGIN
  struct Work { ltr::HapDraft d; int rc = LTR_OK; std::vector<Group> groups; ltr_hap_result* res = nullptr; };
  std::vector<Work> work((size_t)n_loci);
  struct Owner { std::vector<Work>& w; bool keep = false; ~Owner() { if (!keep) for (Work& x : w) ltr_hap_result_free(x.res); } } owner{work};
  // phase A: the exact alleles of every locus, and the unplaced sequences of every sample that needs clustering (:376-395)
  ltr::parallel_for(n_loci, 1, [&](int64_t l) {
    Work& w = work[(size_t)l];
    const ltr_hap_build_locus& L = loci[l];
    w.rc = ltr::hap_draft(L.rs, L.n_samples, L.region_start, L.region_stop, L.period, L.chrom_seq, L.chrom_seq_start, L.chrom_seq_len, L.chrom_len, indel_flank_len, &w.d);
    if (w.rc != LTR_OK || !w.d.failure.empty()) return;
    for (int32_t s = 0; s < L.n_samples; ++s) {
      if (!(w.d.ignored[(size_t)s] > (int)w.d.per_sample[(size_t)s].size() * 0.25)) continue;      // :392
      Group g; g.sample = s; g.dist_off = 0;
      unique_counts(w.d.per_sample[(size_t)s], w.d.seqs, &g.seqs, &g.counts);
      w.groups.push_back(std::move(g));
    }
  }, 1);
  for (int64_t l = 0; l < n_loci; ++l)
    if (work[(size_t)l].rc != LTR_OK) { ltr::set_error(ctx, name + ": locus " + std::to_string(l) + " could not be prepared"); return work[(size_t)l].rc; }
  // phase B: one distance call over all groups of all loci
  std::vector<int64_t> group_seq_off{0}, seq_off{0}, dist_off;
  std::vector<uint8_t> bytes;
  int64_t dist_size = 0;
  for (Work& w : work)
    for (Group& g : w.groups) {
      for (const std::string& s : g.seqs) { bytes.insert(bytes.end(), s.begin(), s.end()); seq_off.push_back((int64_t)bytes.size()); }
      group_seq_off.push_back((int64_t)seq_off.size() - 1);
      g.dist_off = dist_size; dist_off.push_back(dist_size);
      dist_size += (int64_t)g.seqs.size() * (int64_t)g.seqs.size();
    }
  std::vector<int32_t> dist((size_t)std::max<int64_t>(dist_size, 1), 0);
  if (!dist_off.empty()) {
    if (bytes.empty()) bytes.push_back(0);
    ltr_seq_groups sg;
    sg.n_groups = (int64_t)dist_off.size(); sg.group_seq_off = group_seq_off.data(); sg.n_seqs = (int64_t)seq_off.size() - 1;
    sg.seq_bytes = bytes.data(); sg.seq_off = seq_off.data();
    const int rc = ltr_edit_distances(ctx, &sg, kClusterCap, dist.data(), dist_off.data());
    if (rc != LTR_OK) return rc;
  }
  if (consensus) {                                              // the ladder of every group with the consensus as the centre, in rounds
    std::vector<Group*> all;
    for (Work& w : work) for (Group& g : w.groups) all.push_back(&g);
    const int rc = consensus_rounds(ctx, all, dist.data());
    if (rc != LTR_OK) return rc;
  }
  // phase C: per locus the samples in order (:398), each against the candidates so far (:457-458); then sort, trim, fuse
  ltr::parallel_for(n_loci, 1, [&](int64_t l) {
    Work& w = work[(size_t)l];
    const ltr_hap_build_locus& L = loci[l];
    std::vector<std::string> seqs = w.d.seqs;
    std::vector<uint8_t> inexact(seqs.size(), 0);
    std::vector<int32_t> thr((size_t)L.n_samples, 0), rounds((size_t)L.n_samples, 0), kept((size_t)L.n_samples, 0);
    for (Group& g : w.groups) {
      const auto is_candidate = [&](const std::string& s) { return std::find(seqs.begin(), seqs.end(), s) != seqs.end(); };
      if (consensus) Clusterer::flag_new(is_candidate, &g.cr);
      else Clusterer(g.seqs, g.counts.data(), dist.data() + g.dist_off).run(is_candidate, &g.cr);
      thr[(size_t)g.sample] = g.cr.threshold; rounds[(size_t)g.sample] = g.rounds; kept[(size_t)g.sample] = g.medoid_kept;
      for (size_t c = 0; c < g.cr.centre.size(); ++c) if (g.cr.is_new[c]) { seqs.push_back(g.cr.centre[c]); inexact.push_back(1); }
    }
    w.rc = ltr::hap_finish(w.d, std::move(seqs), std::move(inexact), L.chrom_seq, L.chrom_seq_start, L.chrom_seq_len, L.chrom_len, &w.res);
    if (w.rc == LTR_OK && w.res) { w.res->cluster_threshold = thr; w.res->consensus_rounds = rounds; w.res->medoid_kept = kept; }
  }, 1);
  for (int64_t l = 0; l < n_loci; ++l) if (work[(size_t)l].rc != LTR_OK) return work[(size_t)l].rc;
  for (int64_t l = 0; l < n_loci; ++l) out[l] = work[(size_t)l].res;
  owner.keep = true;
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

}  // namespace

extern "C" {

int ltr_build_haplotypes_clustered(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len, ltr_hap_result** out) {
  return build_haplotypes_clustering(ctx, loci, n_loci, indel_flank_len, out, false);
}
int ltr_build_haplotypes_consensus(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len, ltr_hap_result** out) {
  return build_haplotypes_clustering(ctx, loci, n_loci, indel_flank_len, out, true);
}
int32_t ltr_hap_result_consensus_rounds(const ltr_hap_result* r, int32_t sample) {
  return (!r || sample < 0 || sample >= (int32_t)r->consensus_rounds.size()) ? 0 : r->consensus_rounds[(size_t)sample];
}
int32_t ltr_hap_result_medoid_kept(const ltr_hap_result* r, int32_t sample) {
  return (!r || sample < 0 || sample >= (int32_t)r->medoid_kept.size()) ? 0 : r->medoid_kept[(size_t)sample];
}

const uint8_t* ltr_hap_result_inexact(const ltr_hap_result* r) { return (r && r->failure.empty() && !r->inexact.empty()) ? r->inexact.data() : nullptr; }
int32_t ltr_hap_result_cluster_threshold(const ltr_hap_result* r, int32_t sample) {
  if (!r || sample < 0 || sample >= (int32_t)r->cluster_threshold.size()) return 0;
  return r->cluster_threshold[(size_t)sample];
}

}  // extern "C"
