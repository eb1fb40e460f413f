// ltr_cluster.cpp -- the clustering step of HaplotypeGenerator::gen_candidate_seqs (src/SeqAlignment/HaplotypeGenerator.cpp:376-472):
// the reads of a sample whose repeat sequence is no candidate allele are clustered by edit distance, the cluster centres become
// inexact alleles.  Host code on a distance matrix; the matrix comes from ltr_edit_distances (ltr_editdist.hip).
//   greedy_clustering        :237-268
//   merge_clusters           :271-293
//   the threshold ladder, refinement, acceptance   :397-470
// Documented deviation: the reference's consensus of a cluster is a partial-order alignment (spoa, un-vendored, sampling its input
// with std::random_device); here it is the cluster's MEDOID, the member with the smallest count-weighted sum of distances to the
// members, which is deterministic and one of the reads.
// needleman_wunsch(a, b, score, T) (:201-234) is not run: for T <= 700, score < T <=> d(a, b) < T, and the score is the distance
// whenever it is < T (its row test :225-230 is a lower bound of the final distance).  One exception is reproduced by argument
// position: with an empty SECOND argument and a non-empty first the inner loop never runs and the answer is T + 1 (nw_below).
#include <algorithm>
#include <climits>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ltr_internal.h"
#include "ltr_prep.h"

struct ltr_cluster_result {
  int32_t threshold = -1;
  std::vector<std::vector<int32_t>> members;                    // caller's indices, in the order the reference's vectors hold them
  std::vector<int32_t> centroid;
  std::vector<uint8_t> is_new, counted;
};

namespace {

const int kThresholds[] = {20, 50, 80, 100, 150, 200, 300, 400, 500, 600, 700};   // :405
const int kMaxCentroids = 15;                                                      // :261
const int32_t kClusterCap = 701;

struct Clusterer {
  const std::vector<std::string>& seqs;
  const int32_t* counts;
  const int32_t* dist;
  const int32_t U;
  std::vector<int32_t> lex_rank, ls_rank, by_lex;               // rank of each sequence in std::map order / in length-then-sequence order
  typedef std::map<int32_t, std::vector<int32_t>> Clusters;     // key: lex_rank of the centroid (the std::map<std::string, ..> order)

  Clusterer(const std::vector<std::string>& s, const int32_t* c, const int32_t* d) : seqs(s), counts(c), dist(d), U((int32_t)s.size()) {
    std::vector<int32_t> ls((size_t)U);
    by_lex.resize((size_t)U);
    for (int32_t i = 0; i < U; ++i) by_lex[(size_t)i] = ls[(size_t)i] = i;
    std::sort(by_lex.begin(), by_lex.end(), [&](int32_t x, int32_t y) { return seqs[(size_t)x] < seqs[(size_t)y]; });
    std::sort(ls.begin(), ls.end(), [&](int32_t x, int32_t y) { return ltr::by_len_seq(seqs[(size_t)x], seqs[(size_t)y]); });
    lex_rank.resize((size_t)U); ls_rank.resize((size_t)U);
    for (int32_t r = 0; r < U; ++r) { lex_rank[(size_t)by_lex[(size_t)r]] = r; ls_rank[(size_t)ls[(size_t)r]] = r; }
  }
  // needleman_wunsch(a, b, score, T): is score < T?  (*score = the score when it is)
  bool nw_below(int32_t a, int32_t b, int T, int* score) const {
    if (seqs[(size_t)b].empty() && !seqs[(size_t)a].empty()) return false;     // min_score_per_row stays 1000: T + 1
    const int32_t d = dist[(size_t)a * (size_t)U + (size_t)b];
    *score = d;
    return d < T;
  }
  bool greedy(const std::vector<int32_t>& order, Clusters& clusters, int T) const {      // :237-268
    std::vector<int32_t> centroids{order[0]};
    clusters[lex_rank[(size_t)order[0]]].push_back(order[0]);
    for (size_t i = 1; i < order.size(); ++i) {
      int min_score = INT_MAX, min_cntr = -1;
      for (size_t j = 0; j < centroids.size(); ++j) {
        int score = -1;
        if (nw_below(order[i], centroids[j], T, &score) && score < min_score) { min_cntr = (int)j; min_score = score; }
      }
      if (min_cntr != -1) clusters[lex_rank[(size_t)centroids[(size_t)min_cntr]]].push_back(order[i]);
      else {
        centroids.push_back(order[i]);
        if ((int)centroids.size() > kMaxCentroids) return false;
        clusters[lex_rank[(size_t)order[i]]].push_back(order[i]);
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
  bool merge(const std::vector<int32_t>& cents, Clusters& clusters, int T) const {       // :271-293
    bool updated = false;
    for (size_t i = 0; i < cents.size(); ++i)
      for (size_t j = 1; j < cents.size(); ++j) {
        const int32_t ki = lex_rank[(size_t)cents[i]], kj = lex_rank[(size_t)cents[j]];
        if (i != j && clusters.count(ki) && clusters.count(kj)) {
          int score = -1;
          if (nw_below(cents[i], cents[j], T, &score)) {
            updated = true;
            std::vector<int32_t>& dst = clusters[ki];
            const std::vector<int32_t> src = clusters[kj];
            dst.insert(dst.end(), src.begin(), src.end());
            clusters.erase(kj);
          }
        }
      }
    return updated;
  }
  template <class IsCandidate> void run(const IsCandidate& is_candidate, ltr_cluster_result* out) const {
    out->threshold = -1;
    if (U == 0) return;
    std::vector<int32_t> order = by_lex;                         // :399-403: the first std::map key stays first
    std::sort(order.begin() + 1, order.end(), [&](int32_t x, int32_t y) { return ls_rank[(size_t)x] < ls_rank[(size_t)y]; });
    int64_t ignored = 0;
    for (int32_t i = 0; i < U; ++i) ignored += counts[i];
    for (int T : kThresholds) {
      Clusters clusters;
      if (!greedy(order, clusters, T)) continue;
      for (bool not_converged = true; not_converged;) {          // :418-440
        Clusters updated;
        std::vector<int32_t> cents;
        for (const auto& kv : clusters) {
          const int32_t c = medoid(kv.second);
          std::vector<int32_t>& dst = updated[lex_rank[(size_t)c]];
          if (std::find(cents.begin(), cents.end(), c) == cents.end()) { cents.push_back(c); dst = kv.second; }
          else dst.insert(dst.end(), kv.second.begin(), kv.second.end());
        }
        std::sort(cents.begin() + 1, cents.end(), [&](int32_t x, int32_t y) { return ls_rank[(size_t)x] < ls_rank[(size_t)y]; });
        not_converged = merge(cents, updated, T);
        clusters.swap(updated);
      }
      int64_t covered = 0;                                       // :446-469
      std::vector<uint8_t> counted, is_new;
      for (const auto& kv : clusters) {
        int64_t sum = 0;
        for (int32_t y : kv.second) sum += counts[y];
        const bool big = sum > std::min<int64_t>((int)((double)ignored * 0.10), 10);
        if (big) covered += sum;
        counted.push_back(big ? 1 : 0);
        is_new.push_back(big && !is_candidate(seqs[(size_t)by_lex[(size_t)kv.first]]) ? 1 : 0);
      }
      if (covered >= (int)(0.80 * (double)ignored)) {
        out->threshold = T;
        for (const auto& kv : clusters) { out->centroid.push_back(by_lex[(size_t)kv.first]); out->members.push_back(kv.second); }
        out->counted = counted; out->is_new = is_new;
        return;
      }
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

int ltr_build_haplotypes_clustered(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len, ltr_hap_result** out) {
  if (!out || n_loci < 0 || (n_loci > 0 && !loci) || indel_flank_len < 0) return LTR_ERR_INVALID;
  for (int64_t l = 0; l < n_loci; ++l) out[l] = nullptr;
  if (!ctx) return LTR_ERR_NO_DEVICE;
  for (int64_t l = 0; l < n_loci; ++l)
    if (!loci[l].rs || loci[l].n_samples <= 0 || !loci[l].chrom_seq || loci[l].period < 1) { ltr::set_error(ctx, "ltr_build_haplotypes_clustered: bad locus " + std::to_string(l)); return LTR_ERR_INVALID; }
  ltr::TimedCall timed(ctx, ltr::kTimerHapBuild);
  LTR_GUARD_BEGIN
  struct Group { std::vector<std::string> seqs; std::vector<int32_t> counts; int32_t sample; int64_t dist_off; };
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
    if (work[(size_t)l].rc != LTR_OK) { ltr::set_error(ctx, "ltr_build_haplotypes_clustered: locus " + std::to_string(l) + " could not be prepared"); return work[(size_t)l].rc; }
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
  // phase C: per locus the samples in order (:398), each against the candidates so far (:457-458); then sort, trim, fuse
  ltr::parallel_for(n_loci, 1, [&](int64_t l) {
    Work& w = work[(size_t)l];
    const ltr_hap_build_locus& L = loci[l];
    std::vector<std::string> seqs = w.d.seqs;
    std::vector<uint8_t> inexact(seqs.size(), 0);
    std::vector<int32_t> thr((size_t)L.n_samples, 0);
    for (const Group& g : w.groups) {
      ltr_cluster_result cr;
      Clusterer(g.seqs, g.counts.data(), dist.data() + g.dist_off).run([&](const std::string& s) { return std::find(seqs.begin(), seqs.end(), s) != seqs.end(); }, &cr);
      thr[(size_t)g.sample] = cr.threshold;
      for (size_t c = 0; c < cr.centroid.size(); ++c) if (cr.is_new[c]) { seqs.push_back(g.seqs[(size_t)cr.centroid[c]]); inexact.push_back(1); }
    }
    w.rc = ltr::hap_finish(w.d, std::move(seqs), std::move(inexact), L.chrom_seq, L.chrom_seq_start, L.chrom_seq_len, L.chrom_len, &w.res);
    if (w.rc == LTR_OK && w.res) w.res->cluster_threshold = thr;
  }, 1);
  for (int64_t l = 0; l < n_loci; ++l) if (work[(size_t)l].rc != LTR_OK) return work[(size_t)l].rc;
  for (int64_t l = 0; l < n_loci; ++l) out[l] = work[(size_t)l].res;
  owner.keep = true;
  return LTR_OK;
  LTR_GUARD_END(ctx)
}

const uint8_t* ltr_hap_result_inexact(const ltr_hap_result* r) { return (r && r->failure.empty() && !r->inexact.empty()) ? r->inexact.data() : nullptr; }
int32_t ltr_hap_result_cluster_threshold(const ltr_hap_result* r, int32_t sample) {
  if (!r || sample < 0 || sample >= (int32_t)r->cluster_threshold.size()) return 0;
  return r->cluster_threshold[(size_t)sample];
}

}  // extern "C"
