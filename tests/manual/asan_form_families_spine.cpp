// Stand-alone host program: ltrp::describe_batch with haplotype families and their spines (choose_spine, csrc/ltr_plan_families.cpp)
// through ltr_debug_plan_family_forks, on request (knob 1) and with the knob at -1 -- tandem-repeat windows of 3, 12 and 32 alleles (31 distinct
// fork rows against the park slots), a window that is a prefix of another, windows that fork at one row only -- for a run under
// AddressSanitizer / UBSan.  No GPU, no HIP runtime call.
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -I include tests/manual/asan_form_families_spine.cpp \
//         longtr_amd/csrc/ltr_plan_*.cpp -o asan_form_families_spine && ./asan_form_families_spine
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
std::mt19937 rng(12);
std::string seq(size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rng() & 3]; return s; }
char other(char c) { return c == 'A' ? 'C' : 'A'; }

struct Case { const char* name; int m, n_reads; std::vector<std::string> wins; int want_fams, want_spines, want_spine, want_slots; };

int run(const Case& c) {
  const ltr_align_params prm = {-1.0f, -0.458675f, -1.0f, -0.458675f, -0.00005800168f, -10.448214728f, -10.448214728f, 5, 0};      // HapAligner.h:118
  std::string rb, hb;
  std::vector<int64_t> ro(1, 0), ho(1, 0);
  for (int r = 0; r < c.n_reads; ++r) { rb += seq((size_t)c.m); ro.push_back((int64_t)rb.size()); }
  for (const std::string& w : c.wins) { hb += seq(30) + w + seq(30); ho.push_back((int64_t)hb.size()); }
  const int n_haps = (int)c.wins.size();
  int64_t lro[2] = {0, c.n_reads}, lho[2] = {0, n_haps};
  ltr_locus_batch b{};
  b.n_loci = 1; b.locus_read_off = lro; b.locus_hap_off = lho; b.n_reads = c.n_reads; b.read_bytes = (const uint8_t*)rb.data(); b.read_off = ro.data();
  b.n_haps = n_haps; b.hap_bytes = (const uint8_t*)hb.data(); b.hap_off = ho.data();
  const int cap = c.n_reads * n_haps;
  int bad = 0;
  for (int k = 0; k < 2; ++k) {
    const int32_t knobs[3] = {2, 0, k == 0 ? 1 : -1};
    int64_t out[4] = {0};
    std::vector<int32_t> fam((size_t)cap * 10, 0), rows((size_t)cap * kFamilyParkSlots, 0), fork((size_t)cap, 0), slot((size_t)cap, 0);
    std::vector<int64_t> mo((size_t)cap, 0);
    const int rc = ltr_debug_plan_family_forks(&prm, -1, 1, &b, knobs, out, cap, fam.data(), rows.data(), cap, fork.data(), slot.data(), mo.data());
    std::printf("%s, family_spine %d: rc %d families %lld with a spine %lld steps saved %lld (spine %d slots %d)\n", c.name, knobs[2], rc, (long long)out[0],
                (long long)out[2], (long long)out[3], fam[0], fam[1]);
    if (rc != 0 || out[0] != c.want_fams || out[2] != (k == 0 ? c.want_spines : 0)) bad = 1;
    for (int64_t i = 0; i < out[0]; ++i) {
      const int32_t* f = fam.data() + (size_t)i * 10;
      if (f[0] != (k == 0 ? c.want_spine : -1) || f[1] != (k == 0 ? c.want_slots : 0) || f[3] != kFamilyParkSlots) bad = 1;
      for (int s = 1; s < f[1]; ++s) if (rows[(size_t)i * kFamilyParkSlots + s] <= rows[(size_t)i * kFamilyParkSlots + s - 1]) bad = 1;
    }
    for (int i = 0; i < (int)out[1]; ++i) if (slot[(size_t)i] < 0 || slot[(size_t)i] >= kFamilyParkSlots) bad = 1;
  }
  return bad;
}

std::vector<std::string> repeats(int prefix, int unit_len, int first, int n, int suffix) {
  const std::string p = seq((size_t)prefix), u = seq((size_t)unit_len);
  std::string s = seq((size_t)suffix);
  s[0] = other(u[0]);
  std::vector<std::string> w;
  for (int k = 0; k < n; ++k) { std::string x = p; for (int r = 0; r < first + k; ++r) x += u; w.push_back(x + s); }
  return w;
}
}  // namespace

int main() {
  const int S = kFamilyParkSlots;
  const std::string y = seq(720), x = seq(300);
  std::string a = y.substr(0, 600) + seq(81); a[600] = other(y[600]);
  const Case cases[] = {
      // (the two longest alleles of a pure repeat tie: the first of them in haplotype order is the spine)
      {"3 alleles", 701, 4, repeats(150, 9, 20, 3, 300), 4, 4, 1, 2},
      {"12 alleles", 701, 2, repeats(120, 6, 60, 12, 200), 2, 2, 10, S},
      {"32 alleles, 31 fork rows", 701, 2, repeats(100, 2, 200, 32, 150), 2, 2, 30, S},
      {"narrow band", 401, 3, repeats(80, 7, 20, 5, 150), 3, 3, 3, std::min(S, 4)},
      {"the spine is a prefix", 701, 2, {a, y, y.substr(0, 690)}, 2, 2, 2, 2},
      {"one fork row", 701, 2, {x + "A" + seq(380), x + "C" + seq(390), x + "G" + seq(400)}, 2, 0, -1, 0},
  };
  int bad = 0;
  for (const Case& c : cases) bad |= run(c);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
