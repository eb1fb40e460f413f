// Stand-alone host program: ltrp::describe_batch with haplotype families of the narrow band (form_families, csrc/ltr_plan_families.cpp: reads
// of 321 .. 640 columns) by rule (knob 0) and on request (knob 2), on batches large enough to pack -- C = 321 and C = 640, a fork at
// n - 1, a locus of 64 haplotypes, 33 candidates (one more than a family holds) -- for a run under AddressSanitizer / UBSan.
// No GPU, no HIP runtime call.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -I include tests/manual/asan_form_families_narrow.cpp \
//         longtr_amd/csrc/ltr_plan_*.cpp -o asan_form_families_narrow && ./asan_form_families_narrow
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../longtr_amd/csrc/ltr_internal.h"
#include "../../longtr_amd/csrc/ltr_plan.h"

// what the planning units (ltr_plan_*.cpp) take from the library's other units
namespace ltrp {
void* pinned_alloc(size_t) { return nullptr; }
void pinned_free(void*) {}
}
namespace ltr {
std::atomic<int> g_trace{0};
double dbg_ms() { return 0.0; }
}

namespace {
std::mt19937 rng(11);
std::string seq(size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rng() & 3]; return s; }

struct Case { const char* name; int m, p, n_reads, n_haps; int n_first, n_step; int want_fams[2], want_count, want_p, want_w; };   // want_fams: knob 0, knob 2

// One locus: n_reads random reads of m bases against n_haps windows that share p rows (window h: n_first + h * n_step rows; a
// window of exactly p rows is a prefix of the others).
int run(const Case& c) {
  const ltr_align_params prm = {-1.0f, -0.458675f, -1.0f, -0.458675f, -0.00005800168f, -10.448214728f, -10.448214728f, 5, 0};      // HapAligner.h:118
  const std::string x = seq((size_t)c.p);
  std::string rb, hb;
  std::vector<int64_t> ro(1, 0), ho(1, 0);
  for (int r = 0; r < c.n_reads; ++r) { rb += seq((size_t)c.m); ro.push_back((int64_t)rb.size()); }
  for (int h = 0; h < c.n_haps; ++h) {
    const int n = c.n_first + h * c.n_step;
    std::string w = x;
    if (n > c.p) { w += "ACGT"[h & 3]; w += seq((size_t)(n - c.p - 1)); }
    hb += seq(30) + w + seq(30); ho.push_back((int64_t)hb.size());
  }
  int64_t lro[2] = {0, c.n_reads}, lho[2] = {0, c.n_haps};
  ltr_locus_batch b{};
  b.n_loci = 1; b.locus_read_off = lro; b.locus_hap_off = lho; b.n_reads = c.n_reads; b.read_bytes = (const uint8_t*)rb.data(); b.read_off = ro.data();
  b.n_haps = c.n_haps; b.hap_bytes = (const uint8_t*)hb.data(); b.hap_off = ho.data();
  const int cap = c.n_reads * c.n_haps;
  int bad = 0;
  for (int k = 0; k < 2; ++k) {
    const int32_t knobs[2] = {k == 0 ? 0 : 2, 0};
    int64_t out[4] = {0};
    std::vector<int32_t> fam((size_t)cap * 6, 0), mn((size_t)cap, 0);
    std::vector<int64_t> mo((size_t)cap, 0);
    std::vector<double> U((size_t)cap, 0.0);
    const int rc = ltr_debug_plan_families(&prm, -1, 1, &b, knobs, out, cap, fam.data(), U.data(), cap, mn.data(), mo.data());
    std::printf("%s, knob %d: rc %d families %lld members %lld (count %d p %d W %d)\n", c.name, knobs[0], rc, (long long)out[0], (long long)out[1], fam[1], fam[2], fam[3]);
    if (rc != 0 || out[0] != c.want_fams[k]) bad = 1;
    for (int64_t i = 0; i < out[0]; ++i)
      if (fam[(size_t)i * 6 + 1] != c.want_count || fam[(size_t)i * 6 + 2] != c.want_p || fam[(size_t)i * 6 + 3] != c.want_w) bad = 1;
  }
  return bad;
}
}  // namespace

int main() {
  // (a one-CU device packs from 32 pairs up and launches families from twelve up)
  const Case cases[] = {
      {"C = 321", 322, 200, 16, 3, 300, 20, {16, 16}, 3, 200, 6},
      {"C = 640", 641, 300, 16, 3, 620, 20, {16, 16}, 3, 300, 10},
      // the shortest window IS the shared prefix: p = n_min - 1
      {"fork at n - 1", 501, 480, 16, 3, 480, 15, {16, 16}, 3, 479, 8},
      // 64 haplotypes, windows of 470 .. 533 rows: every one a candidate, more than a family holds -- refused
      {"H = 64", 501, 300, 16, 64, 470, 1, {0, 0}, 0, 0, 0},
      // 33 candidates: one more than kFamilyMaxMembers -- refused; 32: formed
      {"33 candidates", 501, 300, 16, 33, 480, 1, {0, 0}, 0, 0, 0},
      {"32 candidates", 501, 300, 16, 32, 480, 1, {16, 16}, 32, 300, 8},
  };
  int bad = 0;
  for (const Case& c : cases) bad |= run(c);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
