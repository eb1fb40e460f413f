// Stand-alone host program: ltrp::describe_batch with haplotype families (form_families, csrc/ltr_plan_families.cpp) on loci whose fork row lies
// beyond the read -- p up to m + 599 -- for a run under AddressSanitizer / UBSan.  No GPU, no HIP runtime call.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -I include tests/manual/asan_form_families.cpp \
//         longtr_amd/csrc/ltr_plan_*.cpp -o asan_form_families && ./asan_form_families
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

int main() {
  std::mt19937 rng(7);
  auto seq = [&](size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rng() & 3]; return s; };
  ltr_align_params prm = {-1.0f, -0.458675f, -1.0f, -0.458675f, -0.00005800168f, -10.448214728f, -10.448214728f, 5, 0};      // HapAligner.h:118
  int bad = 0;
  // (read length, shared rows, the two windows' lengths): forks at 1400 and at the furthest possible row, 1879
  const int cases[3][4] = {{1281, 1400, 1500, 1550}, {1281, 1879, 1880, 1881}, {701, 200, 650, 700}};
  for (int k = 0; k < 3; ++k) {
    if (k == 1) { prm.log_ins_to_ins = -0.25f; prm.log_del_to_del = -0.25f; }      // (n - m = 600 is a member only under a gentle extension)
    const std::string x = seq(2000), read = seq((size_t)cases[k][0]);
    std::vector<std::string> haps;
    for (int h = 0; h < 2; ++h) {
      std::string w = x.substr(0, (size_t)cases[k][1]);
      if ((int)w.size() < cases[k][2 + h]) { w += "AC"[h]; w += seq((size_t)cases[k][2 + h] - w.size()); }
      haps.push_back(seq(30) + w + seq(30));
    }
    std::string rb = read, hb = haps[0] + haps[1];
    int64_t lro[2] = {0, 1}, lho[2] = {0, 2}, ro[2] = {0, (int64_t)read.size()}, ho[3] = {0, (int64_t)haps[0].size(), (int64_t)hb.size()};
    ltr_locus_batch b{};
    b.n_loci = 1; b.locus_read_off = lro; b.locus_hap_off = lho; b.n_reads = 1; b.read_bytes = (const uint8_t*)rb.data(); b.read_off = ro;
    b.n_haps = 2; b.hap_bytes = (const uint8_t*)hb.data(); b.hap_off = ho;
    const int32_t knobs[2] = {1, 0};
    int64_t out[4] = {0}; int32_t fam[6] = {0}, mn[4] = {0}; int64_t mo[4] = {0}; double U = 0.0;
    const int rc = ltr_debug_plan_families(&prm, -1, 1, &b, knobs, out, 1, fam, &U, 4, mn, mo);
    std::printf("case %d: rc %d families %lld p %d U %.6f\n", k, rc, (long long)out[0], fam[2], U);
    const int want_p = k == 1 ? 1879 : cases[k][1];
    if (rc != 0 || out[0] != 1 || fam[2] != want_p) bad = 1;
  }
  return bad;
}
