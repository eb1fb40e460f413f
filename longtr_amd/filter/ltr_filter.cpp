// The reference's read filter for one region: BamProcessor::read_and_filter_reads (src/bam_processor.cpp:188-487) for reads
// without mates.  The contract, with the reference's line numbers, is in include/ltr_filter.h.  Host code only.
#include "../../include/ltr_filter.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

struct ltr_filter_result {
  std::vector<uint8_t> verdict;
  std::vector<int32_t> pass_record, pass_sample;
  std::vector<uint8_t> pass_pf;
  std::vector<std::string> sample_names;
  int32_t counters[LTR_FILTER_N_COUNTERS];
  int32_t too_many_reads;
};

namespace {

struct Held { int32_t record; uint8_t pf; };

int fail(char* err, int err_cap, const std::string& msg) {
  if (err != nullptr && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", msg.c_str());
  return LTR_FILTER_ERR_INVALID;
}

// trim_alignment_name (:163-170)
std::string trimmed_name(const char* name) {
  std::string s(name != nullptr ? name : "");
  if (s.size() > 2 && s[s.size() - 2] == '/') s.resize(s.size() - 2);
  return s;
}

// BaseQuality::sum_log_prob_correct (base_quality.h:77-84): the MEAN of qual - '!'
double mean_qual(const char* quals, int32_t length) {
  double sum = 0.0;
  for (int32_t i = 0; i < length; i++) sum += double(quals[i] - '!');
  return sum / length;
}

}  // namespace

extern "C" {

void ltr_filter_default_options(ltr_filter_options* opt) {
  if (opt == nullptr) return;
  opt->min_mapq = 20;
  opt->min_mean_qual = 30;
  opt->require_spanning = 1;
  opt->min_flank = 5;
  opt->max_total_reads = 1000000;
  opt->base_qual_trim = '5';
}

int ltr_filter_reads(const ltr_filter_record* recs, int32_t n_recs, int32_t region_start, int32_t region_stop,
                     const ltr_filter_options* opt_in, const ltr_filter_samples* samples, ltr_filter_result** out, char* err, int err_cap) {
  if (out == nullptr) return fail(err, err_cap, "ltr_filter_reads: out is NULL");
  *out = nullptr;
  if (n_recs < 0 || (n_recs > 0 && recs == nullptr)) return fail(err, err_cap, "ltr_filter_reads: no records");
  if (samples == nullptr) return fail(err, err_cap, "ltr_filter_reads: samples is NULL");
  if (samples->use_rgs ? (samples->n_rg < 0 || (samples->n_rg > 0 && (!samples->rg_id || !samples->rg_sample || !samples->rg_file)))
                       : (samples->n_files < 0 || (samples->n_files > 0 && !samples->file_sample)))
    return fail(err, err_cap, "ltr_filter_reads: malformed sample tables");
  ltr_filter_options opt;
  ltr_filter_default_options(&opt);
  if (opt_in != nullptr) opt = *opt_in;
  for (int32_t i = 0; i < n_recs; i++) {
    const ltr_filter_record& r = recs[i];
    if (r.length < 0 || r.n_cigar < 0 || (r.length > 0 && (!r.bases || !r.quals)) || (r.n_cigar > 0 && !r.cigar_type) || r.file_index < 0)
      return fail(err, err_cap, "ltr_filter_reads: malformed record " + std::to_string(i));
  }

  ltr_filter_result* res = new ltr_filter_result();
  res->verdict.assign((size_t)n_recs, LTR_FILTER_NOT_SCANNED);
  memset(res->counters, 0, sizeof(res->counters));
  res->too_many_reads = 0;
  int32_t* cnt = res->counters;

  std::map<std::string, Held> potential_strs;
  std::set<std::string> potential_mates;
  int32_t prev_file = -1, file_index = 0;
  std::string file_label = "0_";

  for (int32_t i = 0; i < n_recs; i++) {
    const ltr_filter_record& r = recs[i];
    if (r.pos > region_stop || r.end_pos < region_start) { res->verdict[i] = LTR_FILTER_OUTSIDE; continue; }                 // :208-215
    if (r.flag & 0x1) { res->verdict[i] = LTR_FILTER_PAIRED_UNSUPPORTED; cnt[LTR_FILTER_N_PAIRED]++; continue; }
    if ((int64_t)potential_strs.size() > (int64_t)opt.max_total_reads) { res->too_many_reads = 1; break; }                  // :217-220
    if ((r.flag & 0x4) || r.pos == 0 || r.n_cigar == 0 || r.length == 0) { res->verdict[i] = LTR_FILTER_SKIPPED; continue; }  // :222
    const bool overlaps = r.pos < region_stop && r.end_pos >= region_start;
    if (overlaps && opt.base_qual_trim > ' ' && (r.cigar_type[0] == 'H' || r.cigar_type[r.n_cigar - 1] == 'H')) {          // :227-235
      cnt[LTR_FILTER_N_OVERLAPPED]++; cnt[LTR_FILTER_N_HARD_CLIPPED]++;
      res->verdict[i] = LTR_FILTER_HARD_CLIPPED;
      continue;
    }
    if (prev_file != r.file_index) {                                                                                        // :247-254
      prev_file = r.file_index;
      potential_mates.clear();
      file_label = std::to_string(++file_index) + "_";
    }
    const std::string key = file_label + trimmed_name(r.name);
    if (!overlaps) {                                                                                                        // :385-417
      res->verdict[i] = LTR_FILTER_OUTSIDE;
      if (potential_strs.find(key) == potential_strs.end()) potential_mates.insert(key);     // (found in either map: IsFirstMate() is equal, continue)
      continue;
    }
    cnt[LTR_FILTER_N_OVERLAPPED]++;                                                                                         // :262
    uint8_t v = LTR_FILTER_PASS;
    if (memchr(r.bases, 'N', (size_t)r.length) != nullptr) { v = LTR_FILTER_HAS_N_BASES; cnt[LTR_FILTER_N_HAS_N]++; }        // :265-284
    else if (mean_qual(r.quals, r.length) < opt.min_mean_qual) { v = LTR_FILTER_LOW_BASE_QUALS; cnt[LTR_FILTER_N_LOW_QUAL]++; }
    else if (r.mapq < opt.min_mapq) { v = LTR_FILTER_LOW_MAPQ; cnt[LTR_FILTER_N_LOW_MAPQ]++; }
    else if (opt.require_spanning == 1 && !(r.pos <= region_start && r.end_pos >= region_stop)) { v = LTR_FILTER_NOT_SPANNING; cnt[LTR_FILTER_N_NOT_SPANNING]++; }
    if (v != LTR_FILTER_PASS) {                                                                                             // :379-383
      res->verdict[i] = v;
      potential_mates.insert(key);
      continue;
    }
    const bool no_pf = opt.min_flank > 0 && (r.pos > region_start - opt.min_flank || r.end_pos < region_stop + opt.min_flank);   // :290
    potential_mates.erase(key);                                                                                             // :324-329
    const bool first = potential_strs.insert(std::make_pair(key, Held{i, (uint8_t)(no_pf ? 0 : 1)})).second;                 // :328, :376
    res->verdict[i] = first ? LTR_FILTER_PASS : LTR_FILTER_DUPLICATE_NAME;
  }

  // :420-437: the held reads in key order; an XA tag = no unique mapping
  std::vector<Held> unpaired;
  for (const auto& kv : potential_strs) {
    if (recs[kv.second.record].has_xa) {
      cnt[LTR_FILTER_N_NOT_UNIQUE]++;
      res->verdict[kv.second.record] = LTR_FILTER_NO_UNIQUE_MAPPING;
    } else
      unpaired.push_back(kv.second);
  }
  cnt[LTR_FILTER_N_PASSED] = (int32_t)unpaired.size();

  // :452-483: from the back, samples in order of first appearance
  std::map<std::string, int32_t> rg_indices;
  std::vector<std::vector<Held>> by_rg;
  for (size_t k = unpaired.size(); k-- > 0;) {
    const ltr_filter_record& r = recs[unpaired[k].record];
    std::string sample;
    if (samples->use_rgs) {                                                                                                 // get_read_group :153-161
      if (r.rg == nullptr) { delete res; return fail(err, err_cap, "Failed to retrieve BAM alignment's RG tag"); }
      bool found = false;
      for (int32_t g = 0; g < samples->n_rg && !found; g++)
        if (samples->rg_file[g] == r.file_index && strcmp(samples->rg_id[g], r.rg) == 0) { sample = samples->rg_sample[g]; found = true; }
      if (!found) { delete res; return fail(err, err_cap, std::string("No sample found for read group ") + r.rg + " in BAM file headers"); }
    } else {
      if (r.file_index >= samples->n_files) { delete res; return fail(err, err_cap, "ltr_filter_reads: no sample given for file " + std::to_string(r.file_index)); }
      sample = samples->file_sample[r.file_index];
    }
    auto it = rg_indices.find(sample);
    int32_t idx;
    if (it == rg_indices.end()) {
      idx = (int32_t)rg_indices.size();
      rg_indices[sample] = idx;
      res->sample_names.push_back(sample);
      by_rg.emplace_back();
    } else
      idx = it->second;
    by_rg[(size_t)idx].push_back(unpaired[k]);
  }
  for (size_t s = 0; s < by_rg.size(); s++)
    for (const Held& h : by_rg[s]) {
      res->pass_record.push_back(h.record);
      res->pass_sample.push_back((int32_t)s);
      res->pass_pf.push_back(h.pf);
    }
  *out = res;
  return LTR_FILTER_OK;
}

void ltr_filter_result_free(ltr_filter_result* r) { delete r; }
int32_t ltr_filter_result_n_records(const ltr_filter_result* r) { return r ? (int32_t)r->verdict.size() : 0; }
const uint8_t* ltr_filter_result_verdicts(const ltr_filter_result* r) { return r ? r->verdict.data() : nullptr; }
int32_t ltr_filter_result_n_passing(const ltr_filter_result* r) { return r ? (int32_t)r->pass_record.size() : 0; }
const int32_t* ltr_filter_result_pass_record(const ltr_filter_result* r) { return r ? r->pass_record.data() : nullptr; }
const int32_t* ltr_filter_result_pass_sample(const ltr_filter_result* r) { return r ? r->pass_sample.data() : nullptr; }
const uint8_t* ltr_filter_result_pass_pf(const ltr_filter_result* r) { return r ? r->pass_pf.data() : nullptr; }
int32_t ltr_filter_result_n_samples(const ltr_filter_result* r) { return r ? (int32_t)r->sample_names.size() : 0; }
const char* ltr_filter_result_sample_name(const ltr_filter_result* r, int32_t i) {
  return (r && i >= 0 && (size_t)i < r->sample_names.size()) ? r->sample_names[(size_t)i].c_str() : "";
}
const int32_t* ltr_filter_result_counters(const ltr_filter_result* r) { return r ? r->counters : nullptr; }
int32_t ltr_filter_result_too_many_reads(const ltr_filter_result* r) { return r ? r->too_many_reads : 0; }
const char* ltr_filter_verdict_name(int32_t v) {
  static const char* const names[] = {"PASS", "OUTSIDE", "NOT_SCANNED", "SKIPPED", "HARD_CLIPPED", "HAS_N_BASES", "LOW_BASE_QUALS", "LOW_MAPQ",
                                      "NOT_SPANNING", "NO_UNIQUE_MAPPING", "DUPLICATE_NAME", "PAIRED_UNSUPPORTED"};
  return (v >= 0 && v < (int32_t)(sizeof(names) / sizeof(names[0]))) ? names[v] : "";
}

}  // extern "C"
