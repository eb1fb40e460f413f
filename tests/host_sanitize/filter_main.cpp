// Stand-alone runner of ltr_filter_reads for tests/test_read_filter_standalone.py (built with -fsanitize=address,undefined on the CPU).
// It reads the hand-made cases the test writes as tab-separated lines and prints one result line per case:
//   CASE <name> <min_mapq> <min_mean_qual> <require_spanning> <min_flank> <max_total_reads> <base_qual_trim code> <use_rgs> <start> <stop>
//   RG <id> <sample> <file>            FS <sample>
//   REC <name> <file> <pos> <end_pos> <mapq> <flag> <bases|*> <quals|*> <cigar types|*> <rg|*> <has_xa>
//   END
// ->  <name> <rc> <verdict names ,> <record:sample:pf ,> <sample names ,> <counters ,> <too_many_reads> <error text>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ltr_filter.h"

static std::vector<std::string> split_tabs(const std::string& line) {
  std::vector<std::string> out;
  std::string tok;
  std::stringstream ss(line);
  while (std::getline(ss, tok, '\t')) out.push_back(tok);
  return out;
}

struct Rec { std::string name, bases, quals, cigar, rg; bool has_rg; int file, pos, end_pos, mapq, flag, has_xa; };

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: filter_main cases.tsv\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line, case_name;
  ltr_filter_options opt;
  int use_rgs = 1, start = 0, stop = 0, n_cases = 0;
  std::vector<Rec> recs;
  std::vector<std::string> rg_id, rg_sample, file_sample;
  std::vector<int32_t> rg_file;
  while (std::getline(in, line)) {
    std::vector<std::string> t = split_tabs(line);
    if (t.empty()) continue;
    if (t[0] == "CASE" && t.size() == 11) {
      case_name = t[1];
      opt.min_mapq = atoi(t[2].c_str()); opt.min_mean_qual = atof(t[3].c_str()); opt.require_spanning = atoi(t[4].c_str());
      opt.min_flank = atoi(t[5].c_str()); opt.max_total_reads = atoi(t[6].c_str()); opt.base_qual_trim = atoi(t[7].c_str());
      use_rgs = atoi(t[8].c_str()); start = atoi(t[9].c_str()); stop = atoi(t[10].c_str());
      recs.clear(); rg_id.clear(); rg_sample.clear(); rg_file.clear(); file_sample.clear();
    } else if (t[0] == "RG" && t.size() == 4) {
      rg_id.push_back(t[1]); rg_sample.push_back(t[2]); rg_file.push_back(atoi(t[3].c_str()));
    } else if (t[0] == "FS" && t.size() == 2) {
      file_sample.push_back(t[1]);
    } else if (t[0] == "REC" && t.size() == 12) {
      Rec r;
      r.name = t[1]; r.file = atoi(t[2].c_str()); r.pos = atoi(t[3].c_str()); r.end_pos = atoi(t[4].c_str()); r.mapq = atoi(t[5].c_str());
      r.flag = atoi(t[6].c_str()); r.bases = t[7] == "*" ? "" : t[7]; r.quals = t[8] == "*" ? "" : t[8]; r.cigar = t[9] == "*" ? "" : t[9];
      r.has_rg = t[10] != "*"; r.rg = t[10]; r.has_xa = atoi(t[11].c_str());
      recs.push_back(r);
    } else if (t[0] == "END") {
      std::vector<ltr_filter_record> fr(recs.size());
      for (size_t i = 0; i < recs.size(); i++) {
        const Rec& r = recs[i];
        fr[i].name = r.name.c_str(); fr[i].file_index = r.file; fr[i].pos = r.pos; fr[i].end_pos = r.end_pos; fr[i].mapq = r.mapq; fr[i].flag = r.flag;
        fr[i].length = (int32_t)r.bases.size(); fr[i].bases = r.bases.c_str(); fr[i].quals = r.quals.c_str();
        fr[i].n_cigar = (int32_t)r.cigar.size(); fr[i].cigar_type = r.cigar.c_str(); fr[i].rg = r.has_rg ? r.rg.c_str() : nullptr; fr[i].has_xa = r.has_xa;
      }
      std::vector<const char*> ids, sms, fss;
      for (auto& s : rg_id) ids.push_back(s.c_str());
      for (auto& s : rg_sample) sms.push_back(s.c_str());
      for (auto& s : file_sample) fss.push_back(s.c_str());
      ltr_filter_samples sm;
      sm.use_rgs = use_rgs; sm.n_rg = (int32_t)ids.size(); sm.rg_id = ids.data(); sm.rg_sample = sms.data(); sm.rg_file = rg_file.data();
      sm.n_files = (int32_t)fss.size(); sm.file_sample = fss.data();
      char err[256] = "";
      ltr_filter_result* res = nullptr;
      int rc = ltr_filter_reads(fr.data(), (int32_t)fr.size(), start, stop, &opt, &sm, &res, err, (int)sizeof(err));
      std::cout << case_name << '\t' << rc << '\t';
      if (rc == 0) {
        const uint8_t* v = ltr_filter_result_verdicts(res);
        for (int32_t i = 0; i < ltr_filter_result_n_records(res); i++) std::cout << (i ? "," : "") << ltr_filter_verdict_name(v[i]);
        std::cout << '\t';
        const int32_t *pr = ltr_filter_result_pass_record(res), *ps = ltr_filter_result_pass_sample(res);
        const uint8_t* pf = ltr_filter_result_pass_pf(res);
        for (int32_t i = 0; i < ltr_filter_result_n_passing(res); i++) std::cout << (i ? "," : "") << pr[i] << ':' << ps[i] << ':' << (int)pf[i];
        std::cout << '\t';
        for (int32_t i = 0; i < ltr_filter_result_n_samples(res); i++) std::cout << (i ? "," : "") << ltr_filter_result_sample_name(res, i);
        std::cout << '\t';
        const int32_t* c = ltr_filter_result_counters(res);
        for (int i = 0; i < LTR_FILTER_N_COUNTERS; i++) std::cout << (i ? "," : "") << c[i];
        std::cout << '\t' << ltr_filter_result_too_many_reads(res) << '\t';
        ltr_filter_result_free(res);
      } else
        std::cout << "\t\t\t\t\t";
      std::cout << err << '\n';
      n_cases++;
    } else {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  // the argument checks: each must refuse, none may read through a NULL
  ltr_filter_result* res = nullptr;
  ltr_filter_samples none = {1, 0, nullptr, nullptr, nullptr, 0, nullptr};
  if (ltr_filter_reads(nullptr, 1, 0, 1, nullptr, &none, &res, nullptr, 0) != LTR_FILTER_ERR_INVALID || res != nullptr) return 3;
  if (ltr_filter_reads(nullptr, 0, 0, 1, nullptr, nullptr, &res, nullptr, 0) != LTR_FILTER_ERR_INVALID) return 3;
  if (ltr_filter_reads(nullptr, 0, 0, 1, nullptr, &none, nullptr, nullptr, 0) != LTR_FILTER_ERR_INVALID) return 3;
  if (ltr_filter_reads(nullptr, 0, 0, 1, nullptr, &none, &res, nullptr, 0) != 0 || ltr_filter_result_n_passing(res) != 0) return 3;
  ltr_filter_result_free(res);
  ltr_filter_result_free(nullptr);
  std::cout << "filter cases run: " << n_cases << '\n';
  return 0;
}
