// ltr_plan_families.cpp -- haplotype families (ltr_plan.h, FamilyRec): formed on the host between the class rule and the class
// sort, read by read: a read's candidates, their fork row and bound, the cost rule; then the count rule over the whole batch.

#include <cstring>

#include "ltr_internal.h"
#include "ltr_plan.h"

namespace ltrp {
namespace {

constexpr int kMaxH = 64;                    // haplotypes of a locus that forms families (FamilyRec::members is one word)

int32_t common_prefix(const uint8_t* a, const uint8_t* b2, int32_t len) {
  int32_t k = 0;
  for (; k + 8 <= len; k += 8) {
    uint64_t x, y;
    std::memcpy(&x, a + k, 8); std::memcpy(&y, b2 + k, 8);
    if (x != y) return k + (__builtin_ctzll(x ^ y) >> 3);
  }
  for (; k < len && a[k] == b2[k]; ++k) {}
  return k;
}

// What every read of one form_families call is held against.
struct FamilyCall {
  const ltr_locus_batch* b; int F, knob, min_rows;
  const BatchScratch& w;
  double cg, cd, ca, cc, cf, MATCH;
  std::vector<double> lpc;                   // as the device table holds it (ltr_ctx.hip, build_tables): lpc[1] = 0, lpc[j+1] = lpc[j] + c
};

// The haplotype windows of one locus and the longest common prefix of any two, formed when its first read with candidates asks.
struct LocusWindows {
  const uint8_t* win[kMaxH]; int32_t wn[kMaxH];
  int32_t lcp[kMaxH][kMaxH];                 // -1: not formed yet
  bool formed = false;
  void form(const FamilyCall& fc, const int64_t h0, const int64_t h1) {
    const ltr_locus_batch* b = fc.b;
    for (int64_t h = h0; h < h1; ++h) {
      const int64_t hl = b->hap_off[h + 1] - b->hap_off[h];
      int64_t pos = 0;
      const int64_t n = hl > 60 ? ltr::hap_window(hl, fc.F, &pos) : 0;
      win[h - h0] = b->hap_bytes + b->hap_off[h] + pos; wn[h - h0] = (int32_t)std::max<int64_t>(n, 0);
      for (int64_t h2 = h0; h2 < h1; ++h2) lcp[h - h0][h2 - h0] = -1;
    }
    formed = true;
  }
  int32_t lcp_of(const int x, const int y) {
    if (lcp[x][y] < 0) lcp[x][y] = lcp[y][x] = common_prefix(win[x], win[y], std::min(wn[x], wn[y]));
    return lcp[x][y];
  }
};

// A read of either band: its family geometry (strips of W on L lanes of one wavefront) and the class its pairs are members from.
struct ReadGeom { int64_t m; bool narrow; int W, L, Wp, Lp, own_cls; };
bool read_geometry(const FamilyCall& fc, const int64_t m, ReadGeom* g) {
  const int C = (int)m - 1;
  // the narrow band: by rule and on request 2 (knob 1 keeps to the wide band)
  g->m = m; g->narrow = C >= kFamilyNarrowMinC && C <= kFamilyNarrowMaxC && (fc.knob == 0 || fc.knob >= 2);
  if (!g->narrow && (C < kFamilyMinC || C > kFamilyMaxC)) return false;
  g->W = (C + 63) / 64; g->L = (C + g->W - 1) / g->W;
  // (the narrow band's pairs as the class rule packs them: two to a wavefront, 32 lanes of Wp columns)
  g->Wp = (C + (1 << kPackMaxShift) - 1) >> kPackMaxShift; g->Lp = (C + g->Wp - 1) / g->Wp;
  g->own_cls = g->narrow ? pack_class(kPackMaxShift, g->Wp) : g->W - 1;
  return true;
}

// A read's candidates: what the class rule left in the one-wave class of the read's own strip width -- the narrow band: in the packed
// class of 32 lanes; on request 2 also in the one-wave class, where a batch too small to pack leaves them --, with a DP to run
struct Candidates { int h[kMaxH]; int64_t i[kMaxH]; int n = 0; };   // haplotype within the locus, pair in batch order
void read_candidates(const FamilyCall& fc, const ReadGeom& g, const int64_t h0, const int64_t h1, const int64_t row_at, Candidates* c) {
  const ltr_locus_batch* b = fc.b;
  const RawBuf<PairDesc>& pairs = fc.w.pairs; const RawBuf<int16_t>& key = fc.w.key; const RawBuf<int16_t>& bin = fc.w.bin;
  int64_t i = row_at;
  for (int64_t h = h0; h < h1; ++h) {
    if (b->realign_hap && !b->realign_hap[h]) continue;
    if ((bin[(size_t)i] == g.own_cls || (g.narrow && fc.knob >= 2 && bin[(size_t)i] == g.W - 1)) && key[(size_t)i] > 0 && pairs[(size_t)i].generic == 0 && pairs[(size_t)i].n >= 2) { c->h[c->n] = (int)(h - h0); c->i[c->n] = i; ++c->n; }
    ++i;
  }
}

// The fork row p of the candidates and its bound U, then -- once -- of those whose score has a chance against that bound (fewer
// members: p can only grow and U only fall, so whoever passes the first bound passes the second).  False: no family here.
bool fork_and_bound(const FamilyCall& fc, const ReadGeom& g, LocusWindows* lw, Candidates* c, int* p_out, double* U_out) {
  int p = 0; double U = 0.0;
  for (int pass = 0; pass < 2 && c->n >= 2; ++pass) {
    p = 0x7fffffff;
    for (int k = 0; k < c->n; ++k) p = std::min(p, std::min(k ? lw->lcp_of(c->h[0], c->h[k]) : 0x7fffffff, lw->wn[c->h[k]] - 1));
    if (p < fc.min_rows) return false;
    if ((size_t)p >= fc.lpc.size()) return false;                  // (cannot happen: see the table's size)
    U = ((fc.cg + fc.lpc[(size_t)p - 1]) + fc.cd) + fc.MATCH;
    if (pass) break;
    int kept = 0;
    for (int k = 0; k < c->n; ++k) {
      const int dd = lw->wn[c->h[k]] - (int)g.m;
      // (the haplotype window longer than the read is the insertion state, the read longer the deletion state: make_rules)
      const double gap = dd > 0 ? fc.cf + (double)(dd - 1) * fc.ca : (dd < 0 ? fc.cg + (double)(-dd - 1) * fc.cc : 0.0);
      if (gap > U) { c->h[kept] = c->h[k]; c->i[kept] = c->i[k]; ++kept; }
    }
    if (kept == c->n) break;
    c->n = kept;
  }
  *p_out = p; *U_out = U;
  return c->n >= 2 && c->n <= kFamilyMaxMembers;
}

// The cost rule: the family's modelled steps against its members' own (f->count, p, W, dd_min, dd_max and *fam_steps out).
bool family_pays(const FamilyCall& fc, const ReadGeom& g, const LocusWindows& lw, const Candidates& c, const int p, FamilyDesc* f, int64_t* fam_steps_out) {
  int64_t fam_steps = (p - 1) + (g.L - 1), own_steps = 0;
  int dd_min = 0x7fffffff, dd_max = -0x7fffffff;
  for (int k = 0; k < c.n; ++k) {
    const int n = lw.wn[c.h[k]];
    fam_steps += (n - p) + (g.L - 1); own_steps += (n - 1) + (g.L - 1);
    dd_min = std::min(dd_min, n - (int)g.m); dd_max = std::max(dd_max, n - (int)g.m);
  }
  if (!g.narrow) {
    if (fc.knob <= 0 && fam_steps >= own_steps) return false;
  } else if (fc.knob <= 0) {
    // the geometries differ, so modelled WORK is compared, not steps: the family's steps on a whole wavefront of strips of W
    // against the members' own steps on half a wavefront of strips of Wp (formed here rather than read back from the pairs'
    // launch-order keys, which hold the packed cost only to 1/16 octave)
    double own_work = 0.0;
    for (int k = 0; k < c.n; ++k) own_work += (double)((lw.wn[c.h[k]] - 1) + (g.Lp - 1)) * ((double)g.Wp + kStepOverhead) * (double)(1 << kPackMaxShift) / 64.0;
    if ((double)fam_steps * ((double)g.W + kStepOverhead) >= own_work) return false;
  }
  f->first = 0; f->count = c.n; f->p = p; f->W = g.W; f->dd_min = dd_min; f->dd_max = dd_max;
  *fam_steps_out = fam_steps;
  return true;
}

// The spine (FamilySpine): which member the stream follows beyond p, where the others leave it, which of those rows are parked.
// Forming is settled before this is asked: a spine only removes rows and one fill/drain, so a family that pays keeps paying.
// Member k leaves spine s at f_k = max(p, min(lcp(s, k), n_k - 1)); s minimises (n_s - p) + sum(n_k - f_k), the first such member.
// Of the distinct f_k beyond p at most kFamilyParkSlots - 1 are kept, the subset that saves most rows: with v_0 = p < v_1 < .. the
// kept rows and N(v) the members with f_k >= v, sum (v_i - v_(i-1)) N(v_i); a member whose own row is not kept starts from the
// nearest kept row below it (exact all the same: it runs those rows again).
// In two parts.  spine_of_members: what the members and p alone decide -- the spine member, the fork rows, the park rows, every member's
// slot; the reads of a locus mostly meet the same candidates at the same p, so the locus keeps the last answer (SpineMemo).
// spine_for_read: what the read adds -- the certificate ranges n - m and the modelled steps (L lanes).
// *sp and fork[] are written only for a family with a spine (sp->spine >= 0).
struct SpineMemo { uint64_t members = 0; int p = -1; FamilySpine sp; int16_t fork[kFamilyMaxMembers]; };
void spine_of_members(LocusWindows* lw, const Candidates& c, const int p, FamilySpine* sp, int16_t* fork) {
  sp->spine = -1;
  // (park rows, ranges and fork rows are 16-bit: a member's n is bounded by the one-wave class, n <= m + 600 <= kFamilyMaxC + 601 -- checked all the same)
  for (int k = 0; k < c.n; ++k) if (lw->wn[c.h[k]] > 0x7fff) return;
  const auto fork_of = [&](const int s, const int k) { return std::max(p, std::min(lw->lcp_of(c.h[s], c.h[k]), lw->wn[c.h[k]] - 1)); };
  int best = -1; int64_t best_rows = 0; bool forks = false;
  for (int s = 0; s < c.n; ++s) {
    int64_t rows = lw->wn[c.h[s]] - p; bool any = false;
    for (int k = 0; k < c.n; ++k) if (k != s) { const int f = fork_of(s, k); rows += lw->wn[c.h[k]] - f; any = any || f > p; }
    if (best < 0 || rows < best_rows) { best = s; best_rows = rows; forks = any; }
  }
  if (!forks) return;                                              // nothing beyond p for the best member: nothing for any
  std::memset(sp, 0, sizeof(*sp)); std::memset(fork, 0, sizeof(int16_t) * kFamilyMaxMembers);
  // the distinct fork rows beyond p, ascending, and the members at or beyond each
  int v[kFamilyMaxMembers + 1], N[kFamilyMaxMembers + 1], nv = 1;
  v[0] = p; N[0] = 0;
  for (int k = 0; k < c.n; ++k) { fork[k] = (int16_t)(k == best ? lw->wn[c.h[k]] : fork_of(best, k)); }
  for (int k = 0; k < c.n; ++k) if (k != best && fork[k] > p) {
    int at = 1;
    while (at < nv && v[at] < fork[k]) ++at;
    if (at == nv || v[at] != fork[k]) { for (int j = nv; j > at; --j) v[j] = v[j - 1]; v[at] = fork[k]; ++nv; }
  }
  sp->spine = (int8_t)best;
  sp->slot_row[0] = (int16_t)p;
  if (nv <= kFamilyParkSlots) {
    // every fork row has a slot (the common case; each kept row saves rows, so this is also what the search below would find)
    sp->n_slots = (int8_t)nv;
    for (int j = 1; j < nv; ++j) sp->slot_row[j] = (int16_t)v[j];
  } else {
    for (int i = 1; i < nv; ++i) { N[i] = 0; for (int k = 0; k < c.n; ++k) if (k != best && fork[k] >= v[i]) ++N[i]; }
    // the best kept subset of at most kFamilyParkSlots - 1 of them: gain[j][i] = most rows saved with j kept rows, v[i] the last
    int64_t gain[kFamilyParkSlots][kFamilyMaxMembers + 1]; int from[kFamilyParkSlots][kFamilyMaxMembers + 1];
    gain[0][0] = 0;
    int bj = 0, bi = 0; int64_t bg = 0;
    for (int j = 1; j < kFamilyParkSlots; ++j)
      for (int i = j; i < nv; ++i) {
        gain[j][i] = -1;
        for (int i2 = j - 1; i2 < i; ++i2) {
          if (j == 1 && i2 != 0) break;
          const int64_t ga = gain[j - 1][i2] + (int64_t)(v[i] - v[i2]) * N[i];
          if (ga > gain[j][i]) { gain[j][i] = ga; from[j][i] = i2; }
        }
        if (gain[j][i] > bg) { bg = gain[j][i]; bj = j; bi = i; }
      }
    sp->n_slots = (int8_t)(bj + 1);
    for (int j = bj, i = bi; j >= 1; i = from[j][i], --j) sp->slot_row[j] = (int16_t)v[i];
  }
  for (int k = 0; k < c.n; ++k) if (k != best) {
    int s = 0;
    while (s + 1 < sp->n_slots && sp->slot_row[s + 1] <= fork[k]) ++s;
    sp->slot_of[k] = (uint8_t)s;
  }
}
// Returns the family's modelled steps as it is run.
int64_t spine_for_read(const ReadGeom& g, const LocusWindows& lw, const Candidates& c, FamilySpine* sp) {
  const int best = sp->spine;
  int64_t steps = (lw.wn[c.h[best]] - 1) + (g.L - 1);
  for (int k = 0; k < c.n; ++k) if (k != best) steps += (lw.wn[c.h[k]] - sp->slot_row[sp->slot_of[k]]) + (g.L - 1);
  // the certificate's range from each park row on: the members of later slots and the spine member
  for (int s = 0; s < sp->n_slots; ++s) {
    int lo = lw.wn[c.h[best]] - (int)g.m, hi = lo;
    for (int k = 0; k < c.n; ++k) if (k != best && sp->slot_of[k] > s) { const int dd = lw.wn[c.h[k]] - (int)g.m; lo = std::min(lo, dd); hi = std::max(hi, dd); }
    sp->slot_dd_min[s] = (int16_t)lo; sp->slot_dd_max[s] = (int16_t)hi;
  }
  return steps;
}

// The count rule.
// A launch of its own pays once the batch fills the GPU: one wavefront runs a family's stem and all its tails one after the other, so
// a family lasts as long as ~H pairs on one wave slot, and the families are dealt out statically.  Measured on MI355X (config-3 loci,
// families on request against none, kernel ms per pass): 16 families 1.52 against 0.38, 272 families 2.37 against 1.07, 533 families
// (4311 pairs) 2.04 against 1.40 -- the pass stays one family long while the plan kernel spreads the same pairs over idle wave slots.
// By rule: from a family for every wavefront of a full grid up (kFamPerCu per CU: three workgroups of four); knobs 1 and 2: whenever
// one can be formed.  The narrow band by rule only when its families ALONE are a full grid's worth: below that a plan keeps the
// launches it had -- its packed pairs stay with the plan kernel, its wide families are counted as before -- so that a plan of a few
// hundred loci runs exactly as it did without the band (a 300-locus plain run of config 3 on 256 CUs: 2271 narrow families, not
// formed; 625 loci: 4571, formed).  Then both bands together against the same count.
void count_rule(const int n_cu, std::vector<FamilyRec>* out) {
  const int64_t want = (int64_t)kFamPerCu * std::max(n_cu, 1);
  const auto is_narrow = [](const FamilyRec& r) { return r.f.W * 64 <= kFamilyNarrowMaxC; };
  if ((int64_t)std::count_if(out->begin(), out->end(), is_narrow) < want) out->erase(std::remove_if(out->begin(), out->end(), is_narrow), out->end());
  if ((int64_t)out->size() < want) out->clear();
}

// The members leave their classes for the family class, under their family's key.
void mark_members(const std::vector<FamilyRec>& fams, const BatchScratch& w) {
  ltr::parallel_for((int64_t)fams.size(), 256, [&](int64_t i) {
    const FamilyRec& r = fams[(size_t)i];
    for (uint64_t rest = r.members; rest; rest &= rest - 1) {
      const size_t at = (size_t)(r.row_at + __builtin_ctzll(rest));
      w.bin[at] = (int16_t)kFamClass; w.key[at] = r.key;
    }
  });
}

}  // namespace

void form_families(const ltr_locus_batch* b, const ModelConsts& mc, const int F, const int n_cu, const int knob, const int min_rows_in, const int spine_knob,
                   const std::vector<int64_t>& pair_base, const BatchScratch& w, std::vector<FamilyRec>* out, FamilySide* side) {
  FamilyCall fc{b, F, knob, std::max(min_rows_in, 2) /* (the stem has a row of its own) */, w,
                (double)mc.g, (double)mc.d, (double)mc.a, (double)mc.c, (double)mc.f, (double)mc.match, {}};
  // (as far as a fork row can reach: p <= n - 1 and a member's n <= m + 600 <= kFamilyMaxC + 601)
  fc.lpc.assign((size_t)kFamilyMaxC + 600 + 4, 0.0);
  for (size_t j = 1; j + 1 < fc.lpc.size(); ++j) fc.lpc[j + 1] = fc.lpc[j] + (double)mc.c;
  std::vector<std::vector<FamilyRec>> per_locus((size_t)b->n_loci);
  side->sp.assign((size_t)b->n_loci, {}); side->fork.assign((size_t)b->n_loci, {});
  ltr::parallel_for(b->n_loci, 64, [&](int64_t l) {
    const int64_t r0 = b->locus_read_off[l], r1 = b->locus_read_off[l + 1];
    const int64_t h0 = b->locus_hap_off[l], h1 = b->locus_hap_off[l + 1];
    if (h1 - h0 < 2 || h1 - h0 > kMaxH) return;
    LocusWindows lw;
    SpineMemo memo;
    int64_t at = pair_base[(size_t)l];
    for (int64_t r = r0; r < r1; ++r) {
      if (b->realign_read && !b->realign_read[r]) continue;
      const int64_t row_at = at;
      for (int64_t h = h0; h < h1; ++h) if (!b->realign_hap || b->realign_hap[h]) ++at;
      ReadGeom g;
      if (!read_geometry(fc, b->read_off[r + 1] - b->read_off[r], &g)) continue;
      Candidates c;
      read_candidates(fc, g, h0, h1, row_at, &c);
      if (c.n < 2) continue;
      if (!lw.formed) lw.form(fc, h0, h1);
      FamilyRec rec;
      int p = 0; int64_t fam_steps = 0;
      if (!fork_and_bound(fc, g, &lw, &c, &p, &rec.U) || !family_pays(fc, g, lw, c, p, &rec.f, &fam_steps)) continue;
      rec.first_pair = c.i[0]; rec.row_at = row_at; rec.members = 0;
      rec.steps = rec.plain_steps = (int32_t)fam_steps; rec.locus = (int32_t)l; rec.spine_at = -1;
      rec.key = rec.plain_key = launch_key((double)fam_steps * (g.W + kStepOverhead));
      if (spine_knob >= 0) {
        // the spine records of a locus sit in lists of their own: the family list, which is joined, filtered and searched, stays lean
        uint64_t haps = 0;
        for (int k = 0; k < c.n; ++k) haps |= 1ull << c.h[k];
        if (memo.p != p || memo.members != haps) { spine_of_members(&lw, c, p, &memo.sp, memo.fork); memo.p = p; memo.members = haps; }
        if (memo.sp.spine >= 0) {
          FamilySpine sp = memo.sp;
          const int16_t* fork = memo.fork;
          const int64_t steps = spine_for_read(g, lw, c, &sp);
          std::vector<FamilySpine>& sps = side->sp[(size_t)l];
          if (sps.empty()) sps.reserve((size_t)(r1 - r));             // (at most one per remaining read)
          rec.spine_at = (int32_t)sps.size(); rec.steps = (int32_t)steps;
          rec.key = launch_key((double)steps * (g.W + kStepOverhead));
          sps.push_back(sp);
          if (side->keep_forks) side->fork[(size_t)l].insert(side->fork[(size_t)l].end(), fork, fork + kFamilyMaxMembers);
        }
      }
      for (int k = 0; k < c.n; ++k) rec.members |= 1ull << (c.i[k] - row_at);
      per_locus[(size_t)l].push_back(rec);
    }
  });
  out->clear();
  { size_t total = 0; for (const std::vector<FamilyRec>& v : per_locus) total += v.size(); out->reserve(total); }
  for (const std::vector<FamilyRec>& v : per_locus) out->insert(out->end(), v.begin(), v.end());     // (ascending first_pair: loci, then reads, in batch order)
  if (knob <= 0) count_rule(n_cu, out);
  // The spine's own count rule: by rule (knob 0) a plan runs its families along spines only when it forms at least kSpinePerCu of them
  // per CU; a smaller plan keeps plain families and the launch it had (knob 1: whenever a member forks beyond p).
  if (spine_knob == 0 && (int64_t)out->size() < (int64_t)kSpinePerCu * std::max(n_cu, 1))
    for (FamilyRec& r : *out) { r.spine_at = -1; r.steps = r.plain_steps; r.key = r.plain_key; }
  mark_members(*out, w);
}

}  // namespace ltrp
