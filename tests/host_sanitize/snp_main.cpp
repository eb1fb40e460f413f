// Stand-alone runner of libltr_snp's entry points for tests/test_snp_phasing_standalone.py (built with -fsanitize=address,undefined on the
// CPU).  It reads the hand-made cases the test writes and prints one result line per SET and per READS block:
//   SET <name> <skip padding> <skip regions start:stop,...|-> <number of record lines>
//   <the #CHROM line>
//   <record line> ...
//   READS <column> <number of reads>
//   <pos> <end_pos> <bases hex|*> <quals hex|*> <cigar 10M2D...|*> ...
// ->  SET <name> <rc> <n_samples> <n_valid_snps> <pos:base_one:base_two,... per column, ';' between columns> <column of each sample name ,>
//     SET <name> <rc> <error text>                      when rc != 0
//     READS <rc> <log_p1 bits hex ,> <log_p2 bits hex ,> <counts ,>        (READS <rc> <error text> when rc != 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ltr_snp.h"

static std::vector<std::string> split(const std::string& line, char sep) {
  std::vector<std::string> out;
  std::string tok;
  std::stringstream ss(line);
  while (std::getline(ss, tok, sep)) out.push_back(tok);
  return out;
}

static std::string unhex(const std::string& h) {
  std::string out;
  if (h == "*") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::strtol(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static void print_bits(const std::vector<double>& v) {
  for (size_t i = 0; i < v.size(); i++) {
    unsigned long long b;
    std::memcpy(&b, &v[i], sizeof(b));
    std::printf("%s%016llx", i ? "," : "", b);
  }
}

struct Read { int32_t pos, end_pos; std::string bases, quals, types; std::vector<int32_t> nums; };

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: snp_main cases.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  ltr_snp_set* set = nullptr;
  int n_sets = 0, n_blocks = 0;
  while (std::getline(in, line)) {
    std::vector<std::string> t = split(line, '\t');
    if (t.empty()) continue;
    if (t[0] == "SET" && t.size() == 5) {
      ltr_snp_set_free(set);
      set = nullptr;
      std::vector<int32_t> a, b;
      if (t[3] != "-")
        for (const std::string& r : split(t[3], ',')) { a.push_back(atoi(split(r, ':')[0].c_str())); b.push_back(atoi(split(r, ':')[1].c_str())); }
      std::string header, text;
      std::getline(in, header);
      for (int i = 0, n = atoi(t[4].c_str()); i < n; i++) { std::getline(in, line); text += line + "\n"; }
      char err[256] = "";
      const int rc = ltr_snp_set_create(header.c_str(), text.data(), (int64_t)text.size(), a.data(), b.data(), (int32_t)a.size(), atoi(t[2].c_str()),
                                        &set, err, (int)sizeof(err));
      std::printf("SET\t%s\t%d\t", t[1].c_str(), rc);
      if (rc != 0) {
        if (set != nullptr) return 3;
        std::printf("%s\n", err);
      } else {
        const int32_t S = ltr_snp_set_n_samples(set);
        std::printf("%d\t%d\t", S, ltr_snp_set_n_valid_snps(set));
        for (int32_t c = 0; c < S; c++) {
          const int32_t n = ltr_snp_set_n_snps(set, c);
          std::vector<int32_t> pos((size_t)n + 1);
          std::vector<char> b1((size_t)n + 1), b2((size_t)n + 1);
          if (ltr_snp_set_snps(set, c, pos.data(), b1.data(), b2.data(), n) != n) return 3;
          if (c) std::printf(";");
          for (int32_t i = 0; i < n; i++) std::printf("%s%d:%c:%c", i ? "," : "", pos[(size_t)i], b1[(size_t)i], b2[(size_t)i]);
        }
        std::printf("\t");
        for (int32_t c = 0; c < S; c++) std::printf("%s%d", c ? "," : "", ltr_snp_set_sample_index(set, ltr_snp_set_sample_name(set, c)));
        std::printf("\n");
        if (ltr_snp_set_sample_index(set, "no such sample") != -1 || ltr_snp_set_n_snps(set, S) != -1 || ltr_snp_set_sample_name(set, S)[0]) return 3;
      }
      n_sets++;
    } else if (t[0] == "READS" && t.size() == 3) {
      const int n = atoi(t[2].c_str());
      std::vector<Read> rd((size_t)n);
      for (Read& r : rd) {
        std::getline(in, line);
        std::vector<std::string> f = split(line, '\t');
        if (f.size() != 5) { fprintf(stderr, "bad read line: %s\n", line.c_str()); return 2; }
        r.pos = atoi(f[0].c_str()); r.end_pos = atoi(f[1].c_str()); r.bases = unhex(f[2]); r.quals = unhex(f[3]);
        for (const char* p = f[4] == "*" ? "" : f[4].c_str(); *p;) {
          char* e = nullptr;
          r.nums.push_back((int32_t)std::strtol(p, &e, 10));
          r.types.push_back(*e);
          p = e + 1;
        }
      }
      std::vector<ltr_snp_read> reads((size_t)n);
      for (int i = 0; i < n; i++) {
        const Read& r = rd[(size_t)i];
        reads[(size_t)i] = ltr_snp_read{r.pos, r.end_pos, (int32_t)r.bases.size(), r.bases.data(), r.quals.data(), (int32_t)r.types.size(),
                                        r.types.data(), r.nums.data()};
      }
      std::vector<double> p1((size_t)n, 9.0), p2((size_t)n, 9.0);
      int32_t counts[3] = {5, 6, 7};
      char err[256] = "";
      const int rc = ltr_snp_phasing_priors(set, atoi(t[1].c_str()), reads.data(), n, p1.data(), p2.data(), counts, err, (int)sizeof(err));
      std::printf("READS\t%d\t", rc);
      if (rc != 0) {
        if (counts[0] != 5 || counts[1] != 6 || counts[2] != 7) return 3;          // nothing is added on an error
        std::printf("%s\n", err);
      } else {
        print_bits(p1);
        std::printf("\t");
        print_bits(p2);
        std::printf("\t%d,%d,%d\n", counts[0] - 5, counts[1] - 6, counts[2] - 7);
      }
      n_blocks++;
    } else {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  ltr_snp_set_free(set);
  // the argument checks: each must refuse, none may read through a NULL
  set = nullptr;
  const char* head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS";
  if (ltr_snp_set_create(nullptr, "", 0, nullptr, nullptr, 0, 15, &set, nullptr, 0) != LTR_SNP_ERR_INVALID || set) return 3;
  if (ltr_snp_set_create(head, nullptr, 5, nullptr, nullptr, 0, 15, &set, nullptr, 0) != LTR_SNP_ERR_INVALID || set) return 3;
  if (ltr_snp_set_create(head, "", 0, nullptr, nullptr, 1, 15, &set, nullptr, 0) != LTR_SNP_ERR_INVALID || set) return 3;
  if (ltr_snp_set_create(head, "", 0, nullptr, nullptr, 0, 15, nullptr, nullptr, 0) != LTR_SNP_ERR_INVALID) return 3;
  if (ltr_snp_set_create("chr1\t5", "", 0, nullptr, nullptr, 0, 15, &set, nullptr, 0) != LTR_SNP_ERR_INVALID || set) return 3;
  if (ltr_snp_set_create(head, "", 0, nullptr, nullptr, 0, 15, &set, nullptr, 0) != LTR_SNP_OK || !set) return 3;
  double p = 1.0;
  ltr_snp_read none = {0, 10, 0, nullptr, nullptr, 0, nullptr, nullptr};
  if (ltr_snp_phasing_priors(nullptr, 0, &none, 1, &p, &p, nullptr, nullptr, 0) != LTR_SNP_ERR_INVALID) return 3;
  if (ltr_snp_phasing_priors(set, 1, &none, 1, &p, &p, nullptr, nullptr, 0) != LTR_SNP_ERR_INVALID) return 3;
  if (ltr_snp_phasing_priors(set, 0, nullptr, 1, &p, &p, nullptr, nullptr, 0) != LTR_SNP_ERR_INVALID) return 3;
  if (ltr_snp_phasing_priors(set, 0, &none, 1, &p, &p, nullptr, nullptr, 0) != LTR_SNP_OK || p != 0.0) return 3;   // no SNP: no array is read
  ltr_snp_set_free(set);
  ltr_snp_set_free(nullptr);
  if (ltr_snp_set_n_samples(nullptr) != 0 || ltr_snp_set_n_valid_snps(nullptr) != 0 || ltr_snp_set_snps(nullptr, 0, nullptr, nullptr, nullptr, 4) != 0) return 3;
  double correct[LTR_SNP_N_QUALITIES], error[LTR_SNP_N_QUALITIES];
  ltr_snp_debug_quality_tables(correct, error);
  ltr_snp_debug_quality_tables(nullptr, nullptr);
  if (correct[0] != -100.0 || error[0] != 0.0 || !(correct[LTR_SNP_N_QUALITIES - 1] < 0.0) || !(error[LTR_SNP_N_QUALITIES - 1] < 0.0)) return 3;
  std::printf("snp sets run: %d, read blocks run: %d\n", n_sets, n_blocks);
  return 0;
}
