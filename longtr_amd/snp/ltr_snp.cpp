// ltr_snp.cpp -- create_snp_trees (src/snp_tree.cpp:25-113) without a tracker and calc_het_snp_factors for reads without
// mates (src/snp_phasing_quality.cpp:4-120).  The contract, with the reference's line numbers, is in include/ltr_snp.h.
// Host code only; reads no file.
#include "../../include/ltr_snp.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

struct Snp { int32_t pos; char base_one, base_two; };

void put_error(char* err, int err_cap, const std::string& text) {
  if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", text.c_str());
}

std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t k = 0;
  for (;;) {
    const size_t e = s.find(sep, k);
    out.push_back(s.substr(k, e == std::string::npos ? std::string::npos : e - k));
    if (e == std::string::npos) return out;
    k = e + 1;
  }
}

// BaseQuality (base_quality.h:29-75)
struct QualityTables {
  double log_correct[LTR_SNP_N_QUALITIES], log_error[LTR_SNP_N_QUALITIES];
  QualityTables() {
    log_correct[0] = -100;
    log_error[0] = 0;
    for (int i = 1; i < LTR_SNP_N_QUALITIES; ++i) {
      log_correct[i] = std::log(1.0 - std::pow(10.0, i / (-10.0)));
      log_error[i] = std::log(std::pow(10.0, i / (-10.0) / 5.0));
    }
  }
  static int index(char quality) {
    const int q = (signed char)quality;            // `char` as the reference's compiler has it
    return q < '!' ? 0 : q > 'J' ? 'J' - '!' : q - '!';
  }
};

const QualityTables& tables() {
  static const QualityTables t;
  return t;
}

}  // namespace

struct ltr_snp_set {
  std::vector<std::string> samples;                // the columns after FORMAT
  std::map<std::string, int32_t> index;            // name -> column, the last of several
  std::vector<std::vector<Snp>> snps;              // per column, sorted by position, stable in file order
  int32_t n_valid = 0;
};

namespace {

// One GT subfield: the allele indices (-1 = '.') and whether the separator before the second one is '|'.  false = unreadable.
bool parse_gt(const std::string& gt, std::vector<int32_t>* alleles, bool* phased) {
  alleles->clear();
  *phased = false;
  size_t k = 0;
  for (;;) {
    const size_t e = gt.find_first_of("/|", k);
    const std::string a = gt.substr(k, e == std::string::npos ? std::string::npos : e - k);
    if (a == ".") {
      alleles->push_back(-1);
    } else {
      if (a.empty() || a.size() > 6 || a.find_first_not_of("0123456789") != std::string::npos) return false;
      alleles->push_back((int32_t)std::atoi(a.c_str()));
    }
    if (e == std::string::npos) return true;
    if (alleles->size() == 1) *phased = gt[e] == '|';
    k = e + 1;
  }
}

int add_record(ltr_snp_set* s, const std::string& line, const int32_t* skip_start, const int32_t* skip_stop, int32_t n_skip,
               int32_t padding, std::string* why) {
  const std::vector<std::string> col = split(line, '\t');
  if (col.size() < 8) { *why = "a record with fewer than 8 columns: " + line.substr(0, 60); return LTR_SNP_ERR_INVALID; }
  char* endp = nullptr;
  const long long pos = std::strtoll(col[1].c_str(), &endp, 10);
  if (col[1].empty() || *endp || pos < 1 || pos > (1ll << 31) - 1) { *why = "a record with the unreadable POS " + col[1]; return LTR_SNP_ERR_INVALID; }
  const std::string at = " in the record at POS " + col[1];
  std::vector<std::string> allele{col[3]};
  if (col[4] != ".") for (const std::string& a : split(col[4], ',')) allele.push_back(a);
  const size_t S = s->samples.size();
  std::vector<int32_t> gt_a(S, -1), gt_b(S, -1);
  std::vector<char> usable(S, 0);                  // a phased call of exactly two alleles, neither missing
  if (S > 0) {
    if (col.size() < 9) { *why = "no FORMAT column" + at; return LTR_SNP_ERR_INVALID; }
    const std::vector<std::string> keys = split(col[8], ':');
    const size_t gt_key = (size_t)(std::find(keys.begin(), keys.end(), "GT") - keys.begin());
    if (gt_key == keys.size()) { *why = "no GT in FORMAT" + at; return LTR_SNP_ERR_INVALID; }
    if (col.size() < 9 + S) { *why = "fewer sample columns than the header has" + at; return LTR_SNP_ERR_INVALID; }
    std::vector<int32_t> a;
    bool phased = false;
    for (size_t i = 0; i < S; ++i) {
      const std::vector<std::string> f = split(col[9 + i], ':');
      if (gt_key >= f.size()) continue;            // the field ends before GT: a missing call
      if (!parse_gt(f[gt_key], &a, &phased)) { *why = "unreadable GT " + f[gt_key] + at; return LTR_SNP_ERR_INVALID; }
      for (int32_t x : a)
        if (x >= (int32_t)allele.size()) { *why = "allele index " + std::to_string(x) + " names no allele" + at; return LTR_SNP_ERR_INVALID; }
      if (a.size() != 2 || a[0] < 0 || a[1] < 0 || !phased) continue;
      gt_a[i] = a[0]; gt_b[i] = a[1]; usable[i] = 1;
    }
  }
  // is_biallelic_snp; '*' and symbolic ALTs are no SNPs (ours, see the header)
  if (allele.size() != 2 || allele[0].size() != 1 || allele[1].size() != 1) return LTR_SNP_OK;
  for (const std::string& x : allele) if (x == "*" || x == ".") return LTR_SNP_OK;
  for (int32_t r = 0; r < n_skip; ++r)             // in_any_region (snp_tree.cpp:9-15)
    if (pos >= (long long)skip_start[r] - padding && pos <= (long long)skip_stop[r] + padding) return LTR_SNP_OK;
  ++s->n_valid;
  for (size_t i = 0; i < S; ++i)
    if (usable[i] && gt_a[i] != gt_b[i]) s->snps[i].push_back(Snp{(int32_t)(pos - 1), allele[(size_t)gt_a[i]][0], allele[(size_t)gt_b[i]][0]});
  return LTR_SNP_OK;
}

// add_log_phasing_probs (snp_phasing_quality.cpp:63-93) for one read; n_match[3] += p1 matches, p2 matches, mismatches
int read_priors(const std::vector<Snp>& all, const ltr_snp_read& r, double* log_p1, double* log_p2, int32_t* n_match, std::string* why) {
  *log_p1 = 0.0; *log_p2 = 0.0;
  // findContained(Position(), GetEndPosition() - 1)
  const auto lo = std::lower_bound(all.begin(), all.end(), r.pos, [](const Snp& s, int32_t p) { return s.pos < p; });
  const auto hi = std::upper_bound(lo, all.end(), (int64_t)r.end_pos - 1, [](int64_t p, const Snp& s) { return p < s.pos; });
  const size_t n = (size_t)(hi - lo);
  if (n == 0) return LTR_SNP_OK;
  if (r.n_cigar < 0 || r.length < 0 || (r.n_cigar > 0 && (!r.cigar_type || !r.cigar_num)) || (r.length > 0 && (!r.bases || !r.quals))) {
    *why = "missing arrays";
    return LTR_SNP_ERR_INVALID;
  }
  std::vector<char> bases, quals;
  bases.reserve(n); quals.reserve(n);
  int64_t pos = r.pos, base_index = 0;
  size_t snp_index = 0;
  int32_t cigar_index = 0;
  while (snp_index < n && cigar_index < r.n_cigar) {
    const int64_t len = r.cigar_num[cigar_index], snp_pos = lo[snp_index].pos;
    switch (r.cigar_type[cigar_index]) {
      case 'M': case '=': case 'X':
        if (snp_pos < pos + len) {
          const int64_t at = snp_pos - pos + base_index;
          if (at < 0 || at >= r.length) { *why = "a SNP's base lies outside the read's bases"; return LTR_SNP_ERR_INVALID; }
          bases.push_back(r.bases[at]);
          quals.push_back(r.quals[at]);
          snp_index++;
        } else {
          pos += len;
          base_index += len;
          cigar_index++;
        }
        break;
      case 'D':
        if (snp_pos < pos + len) {
          bases.push_back('-');
          quals.push_back('-');
          snp_index++;
        } else {
          pos += len;
          cigar_index++;
        }
        break;
      case 'I':
        base_index += len;
        cigar_index++;
        break;
      case 'S':
        if (snp_pos < pos) {
          bases.push_back('-');                    // bases in soft clips count as deletions
          quals.push_back('-');
          snp_index++;
        } else {
          base_index += len;
          cigar_index++;
        }
        break;
      case 'H':
        cigar_index++;
        break;
      default:
        *why = "Invalid CIGAR option encountered";
        return LTR_SNP_ERR_CIGAR;
    }
  }
  if (snp_index != n) { *why = "the CIGAR ends before the read's last SNP"; return LTR_SNP_ERR_INVALID; }
  const QualityTables& t = tables();
  for (size_t i = 0; i < n; ++i) {
    if (bases[i] == '-') continue;
    const int q = QualityTables::index(quals[i]);
    if (bases[i] == lo[i].base_one) {
      *log_p1 += t.log_correct[q];
      *log_p2 += t.log_error[q];
      n_match[0]++;
    } else if (bases[i] == lo[i].base_two) {
      *log_p1 += t.log_error[q];
      *log_p2 += t.log_correct[q];
      n_match[1]++;
    } else {
      *log_p1 += t.log_error[q];
      *log_p2 += t.log_error[q];
      n_match[2]++;
    }
  }
  return LTR_SNP_OK;
}

}  // namespace

extern "C" {

int ltr_snp_set_create(const char* header_line, const char* record_lines, int64_t len, const int32_t* skip_start,
                       const int32_t* skip_stop, int32_t n_skip, int32_t skip_padding, ltr_snp_set** out, char* err, int err_cap) {
  if (out) *out = nullptr;
  if (!out || !header_line || len < 0 || (len > 0 && !record_lines) || n_skip < 0 || (n_skip > 0 && (!skip_start || !skip_stop))) {
    put_error(err, err_cap, "ltr_snp_set_create: bad argument");
    return LTR_SNP_ERR_INVALID;
  }
  try {
    std::string head(header_line);
    while (!head.empty() && (head.back() == '\n' || head.back() == '\r')) head.pop_back();
    const std::vector<std::string> hc = split(head, '\t');
    if (hc.size() < 8 || hc[0] != "#CHROM" || (hc.size() > 8 && hc[8] != "FORMAT")) {
      put_error(err, err_cap, "the header line is not a VCF's #CHROM line");
      return LTR_SNP_ERR_INVALID;
    }
    std::unique_ptr<ltr_snp_set> s(new ltr_snp_set());
    for (size_t i = 9; i < hc.size(); ++i) {
      s->index[hc[i]] = (int32_t)s->samples.size();
      s->samples.push_back(hc[i]);
    }
    s->snps.resize(s->samples.size());
    std::string why;
    for (int64_t k = 0; k < len;) {
      const char* nl = (const char*)std::memchr(record_lines + k, '\n', (size_t)(len - k));
      const int64_t e = nl ? nl - record_lines : len;
      std::string line(record_lines + k, (size_t)(e - k));
      k = e + 1;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      const int rc = add_record(s.get(), line, skip_start, skip_stop, n_skip, skip_padding, &why);
      if (rc != LTR_SNP_OK) {
        put_error(err, err_cap, why);
        return rc;
      }
    }
    for (std::vector<Snp>& v : s->snps) std::stable_sort(v.begin(), v.end(), [](const Snp& a, const Snp& b) { return a.pos < b.pos; });
    *out = s.release();
    return LTR_SNP_OK;
  } catch (const std::bad_alloc&) { put_error(err, err_cap, "out of host memory"); return LTR_SNP_ERR_NOMEM; }
  catch (const std::exception& e) { put_error(err, err_cap, std::string("internal error: ") + e.what()); return LTR_SNP_ERR_INVALID; }
}

void ltr_snp_set_free(ltr_snp_set* s) { delete s; }

int32_t ltr_snp_set_n_samples(const ltr_snp_set* s) { return s ? (int32_t)s->samples.size() : 0; }

const char* ltr_snp_set_sample_name(const ltr_snp_set* s, int32_t column) {
  return s && column >= 0 && (size_t)column < s->samples.size() ? s->samples[(size_t)column].c_str() : "";
}

int32_t ltr_snp_set_sample_index(const ltr_snp_set* s, const char* name) {
  if (!s || !name) return -1;
  try {
    const auto it = s->index.find(name);
    return it == s->index.end() ? -1 : it->second;
  } catch (...) { return -1; }
}

int32_t ltr_snp_set_n_valid_snps(const ltr_snp_set* s) { return s ? s->n_valid : 0; }

int32_t ltr_snp_set_n_snps(const ltr_snp_set* s, int32_t column) {
  return s && column >= 0 && (size_t)column < s->snps.size() ? (int32_t)s->snps[(size_t)column].size() : -1;
}

int32_t ltr_snp_set_snps(const ltr_snp_set* s, int32_t column, int32_t* pos, char* base_one, char* base_two, int32_t cap) {
  if (!s || column < 0 || (size_t)column >= s->snps.size() || cap <= 0 || !pos || !base_one || !base_two) return 0;
  const std::vector<Snp>& v = s->snps[(size_t)column];
  const int32_t n = (int32_t)std::min<size_t>(v.size(), (size_t)cap);
  for (int32_t i = 0; i < n; ++i) { pos[i] = v[(size_t)i].pos; base_one[i] = v[(size_t)i].base_one; base_two[i] = v[(size_t)i].base_two; }
  return n;
}

int ltr_snp_phasing_priors(const ltr_snp_set* s, int32_t vcf_sample, const ltr_snp_read* reads, int32_t n_reads, double* log_p1,
                           double* log_p2, int32_t* counts, char* err, int err_cap) {
  if (!s || n_reads < 0 || (n_reads > 0 && (!reads || !log_p1 || !log_p2)) || (vcf_sample >= 0 && (size_t)vcf_sample >= s->snps.size())) {
    put_error(err, err_cap, "ltr_snp_phasing_priors: bad argument");
    return LTR_SNP_ERR_INVALID;
  }
  if (vcf_sample < 0) {                            // no SNP info for the sample: equal phasing LLs
    for (int32_t i = 0; i < n_reads; ++i) log_p1[i] = log_p2[i] = 0.0;
    return LTR_SNP_OK;
  }
  try {
    int32_t n_match[3] = {0, 0, 0};
    std::string why;
    for (int32_t i = 0; i < n_reads; ++i) {
      const int rc = read_priors(s->snps[(size_t)vcf_sample], reads[i], &log_p1[i], &log_p2[i], n_match, &why);
      if (rc != LTR_SNP_OK) {
        put_error(err, err_cap, "read " + std::to_string(i) + ": " + why);
        return rc;
      }
    }
    if (counts) for (int k = 0; k < 3; ++k) counts[k] += n_match[k];
    return LTR_SNP_OK;
  } catch (const std::bad_alloc&) { put_error(err, err_cap, "out of host memory"); return LTR_SNP_ERR_NOMEM; }
  catch (const std::exception& e) { put_error(err, err_cap, std::string("internal error: ") + e.what()); return LTR_SNP_ERR_INVALID; }
}

void ltr_snp_debug_quality_tables(double* log_correct, double* log_error) {
  const QualityTables& t = tables();
  if (log_correct) std::memcpy(log_correct, t.log_correct, sizeof(t.log_correct));
  if (log_error) std::memcpy(log_error, t.log_error, sizeof(t.log_error));
}

}  // extern "C"
