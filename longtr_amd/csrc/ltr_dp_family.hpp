// ltr_dp_family.hpp -- HAPLOTYPE FAMILIES: the pairs of one pooled read against several haplotypes of its locus, the rows their
// haplotype windows share scored ONCE (included after ltr_dp_kernel.hpp and ltr_dp_redo.hpp by ltr_k_family.hip).
//
// Replaces HapAligner::align_seq_to_hap (reference src/SeqAlignment/HapAligner.cpp:236-343) for those pairs: the reference scores a
// read against every candidate haplotype of its locus (:840-852), and the windows of a locus are the same bytes from their first
// base -- left flank, pad, the repeat up to the shortest allele -- to the row where the alleles fork.
//
// Geometry.  A family (FamilyDesc, built on the host: ltrp::form_families) is one read of 321 .. 1280 columns -- ONE column block
// of one wavefront, strips of W = ceil(C / 64) columns on L = ceil(C / W) <= 64 lanes -- and its member pairs, contiguous in the
// sorted pair list, with the fork row p <= every member's n - 1.  Two bands of read length, one geometry: 641 .. 1280 columns
// (W 11 .. 20: pairs that were one-wave pairs of the same strips) and 321 .. 640 columns (W 6 .. 10: pairs that were packed two to a
// wavefront on strips of 11 .. 20, which as a family trade half a wavefront each for the shared rows).
// The wavefront runs the STEM, rows 1 .. p-1, once; parks the carried state of row p-1 (X and Y of every column: 2W doubles a
// lane) in a block of its own; and runs one TAIL per member, rows p .. n_h - 1, from that state.
// The body is column_block<W, true, kModeCert, true, true> (ltr_dp_kernel.hpp) with a row base: same cell, same operation order.
//
// Exactness.  Row 0 is NOT shared: the reference indexes the haplotype with the READ index there (:268), so M(0, j) for j >= p
// depends on haplotype bytes beyond the common prefix and on n.  The stem takes those cells as MISMATCH, which is <= what any
// member holds there.  Every cell is the maximum over DP paths of the path's left-to-right rounded sum, x -> fl(x + k) is
// monotone, and every emission and transition is <= 0 (a path's running value never rises), so
//   * every stem and tail value is a lower bound of the member's true value, bit-identical whenever its best path avoids the
//     lowered cells; a certificate that passes on a lower bound proves the true row passes;
//   * U = ((g + lpc[p-1]) + d) + MATCH, formed as row 0 forms it, is the largest value a lowered cell can hold for any member
//     (lpc decreases), and any path through one ends <= U.
// A member whose shared score S > U (strictly), with every certificate passed, therefore has the reference's score bit for bit;
// any other member is scored again, unshared, by the exact body (redo_dispatch, from the kernel).
// Nothing in this argument depends on W: the narrow band (W 6 .. 10) is exact by the same three facts -- the lowered row-0 cells,
// the acceptance rule S > U, the stem certificate against the member furthest from the diagonal -- and redo_dispatch takes every
// C <= 1280.
//
// The stem's certificate must hold for every member: thr(k) grows with |k|, k = dd - i + j, and |k| over dd_min .. dd_max is
// largest at an end, so the stem tests against max(|k(dd_min)|, |k(dd_max)|).
//
// A family whose members fork from EACH OTHER beyond p runs along a spine instead (spine_walk, below family_walk: one stream along
// one member's window, the others leaving it at park rows of their own); family_walk is the plain family, unchanged.

// One family.  Returns the number of members noted for the exact body (note[0 ..]).
template <int W>
__device__ __forceinline__ int family_walk(const KernelArgs& A, const FamilyArgs& F, const int fi, const int lane,
                                           const double* emit_tab, int* note, double* park) {
  const FamilyDesc* __restrict__ fd = F.fams + fi;
  const int first = uni(fd->first), count = uni(fd->count), p = uni(fd->p);
  const int dd_lo = uni(fd->dd_min), dd_hi = uni(fd->dd_max);
  const PairDesc* pp0 = A.pairs + first;
  const int m = uni(pp0->m);
  const uint8_t* __restrict__ read = A.read_bytes + uni64(pp0->read_off);
  const double ca = A.mc.a, cc = A.mc.c, cd = A.mc.d, ce = A.mc.e, cf = A.mc.f, cg = A.mc.g, cb = A.mc.b;
  const double MATCH = A.mc.match, MISMATCH = A.mc.mismatch;
  const float c32 = A.mc.c;
  const double IMP = kImp;
  const double* __restrict__ lpc = A.lpc;
  const int C = m - 1;
  const int L = (C + W - 1) / W;                               // active lanes (one column block)
  const int Wl = C - (L - 1) * W;                              // real columns of the last lane, 1..W
  const int j0 = 1 + lane * W;
  const int rb = p - 1;                                        // the tails' row base: the row whose state is parked

  // ---- row 0 of the stem (HapAligner.cpp:263-272): columns below the fork as every member has them, the others lowered ----
  double Xp[W], Yp[W];
  constexpr int NQ = (W + 3) / 4;
  uint32_t rc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) rc[q] = 0;
  int e01;
  double emit00;
  {
    const uint8_t* __restrict__ hap = A.hap_bytes + uni64(pp0->hap_off);
    const uint32_t r0 = (uint32_t)uni((int)read[0]);
    const int h0 = uni((int)hap[0]);
    emit00 = (h0 == (int)r0) ? MATCH : MISMATCH;               // match_matrix[0], :265
    e01 = (h0 == uni((int)read[1])) ? 1 : 0;                   // emission of the whole first column, :276
#pragma unroll
    for (int s = 0; s < W; ++s) {
      const int jc = min(j0 + s, m - 1);
      const double lp1 = lpc[max(jc - 1, 0)], lp = lpc[jc];
      const uint32_t hb = (uint32_t)hap[min(jc, p - 1)];
      const double D0jm1 = (jc == 1) ? IMP : (cg + lp1);
      const double D0j = cg + lp;
      const bool eq = (jc < p) & (hb == r0);                   // (columns from the fork on: MISMATCH, <= every member's cell)
      const double M0 = (D0jm1 + cd) + (eq ? MATCH : MISMATCH);
      Xp[s] = dmax(M0 + ce, dmax(D0j + cd, IMP + cb));
      Yp[s] = dmax(M0 + cf, IMP + ca);
      rc[s / 4] |= (((uint32_t)read[jc] >> 1) & 3u) << (2 * (s % 4) + 4);
      if ((s % 4) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the largest value a lowered cell can hold for any member (row 0's own expression at column p)
  const double U = ((cg + lpc[p - 1]) + cd) + MATCH;

  double outX = Xp[W - 1];
  double leftX = wave_shr1(outX, dmax(emit00 + ce, dmax(IMP + cd, IMP + cb)));
  double outZ = IMP;
  uint64_t fmask = ~0ull;
  const uint64_t lastbit = 1ull << (L - 1);
  double certM = 0.0;
  double res_cap = 0.0;
  // per-phase state of the step (the stem: member 0's window, rows 1 .. p-1; a tail: the member's window, rows p .. n-1)
  int nr = p;                                                  // rows of the phase counted from its base: lane l is active on steps l .. l + nr - 2
  const uint16_t* hs = A.hap_codes + uni64(pp0->hap_off) - 63;
  const uint32_t hoff = 64u - (uint32_t)lane;                  // (hs + t)[hoff] = row base + t + 1 - lane
  __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)hs), 0, 0x7fffffff, 0x00020000);
  const int hvo = (int)(hoff * (uint32_t)sizeof(uint16_t));
  auto hrow_at = [&](const int t) __attribute__((always_inline)) -> uint32_t {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(hrs, hvo, t * 2, 0);
  };
  typedef double d2v_t __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)((const double2*)A.colXZ + e01)), 0, 0x7fffffff, 0x00020000);
  uint32_t h_next = hrow_at(0);
  double bX_next, bZ_next;
  int bso = 2 * 2 * (int)sizeof(double2);                      // -> record 2: lane 0's row at step 1
  { const double2 b1 = ((const double2*)A.colXZ)[e01 + 2 * 1]; bX_next = b1.x; bZ_next = b1.y; }
  // band offset k of (my row, j0) for the smallest and the largest n - m of the family; -1 per step
  double kd = (double)(dd_lo - (1 - lane) + j0), kd2 = (double)(dd_hi - (1 - lane) + j0);
  const double cabs_up = fabs((double)c32) * (1.0 + 0x1p-22);
  const double thr0 = -600.0 + 1e-6;

  // One wavefront step of column_block's certificate body (FIRST, final block, SYM, LUT).  STEM: the threshold of the member
  // furthest from the diagonal; FIN: the last step of a tail, which captures the member's result.
  auto step = [&](auto fin_tag, auto stem_tag, const int t) __attribute__((always_inline)) {
    constexpr bool FIN = decltype(fin_tag)::value;
    constexpr bool STEM = decltype(stem_tag)::value;
    const uint32_t h = h_next;
    const double bX = bX_next, bZ = bZ_next;
    h_next = hrow_at(t + 1);
    {
      const d2v_t bn = __builtin_bit_cast(d2v_t, __builtin_amdgcn_raw_buffer_load_b128(brs, 0, bso, 0));
      bso += 2 * (int)sizeof(double2); bX_next = bn.x; bZ_next = bn.y;
    }
    const double mX = wave_shr1(outX, bX);
    const double mZ = wave_shr1(outZ, bZ);
    const double kcur = kd, kcur2 = kd2;
    kd = kcur - 1.0;
    if (STEM) kd2 = kcur2 - 1.0;
    const int a_hi = min(t, L - 1), a_lo = max(t - (nr - 2), 0);
    const uint64_t active_mask = (~0ull >> (63 - a_hi)) & (~0ull << a_lo);
    const bool active = __builtin_amdgcn_inverse_ballot_w64(active_mask);
    if (active) {
      double diag = leftX;
      leftX = mX;
      double zleft = mZ;
      double Iv = 0.0, Dv = 0.0;
      double em[W];
      auto fetch_quad = [&](const int q) __attribute__((always_inline)) {
        const double2* row = (const double2*)((const char*)emit_tab + (h + rc[q < NQ ? q : 0]));
        const double2 lo = row[0];
        em[4 * q] = lo.x;
        if (4 * q + 1 < W) em[(4 * q + 1) < W ? (4 * q + 1) : 0] = lo.y;
        if (4 * q + 2 < W) {
          const double2 hi = row[kEmitTabDoubles / 4];
          em[(4 * q + 2) < W ? (4 * q + 2) : 0] = hi.x;
          if (4 * q + 3 < W) em[(4 * q + 3) < W ? (4 * q + 3) : 0] = hi.y;
        }
      };
      fetch_quad(0);
      if (NQ > 1) fetch_quad(1 < NQ ? 1 : 0);
      certM = em[0] + diag;
      double Mv = certM;
#pragma unroll
      for (int s = 0; s < W; ++s) {
        double Mnext = 0.0;
        if ((s % 4) == 2 && (s / 4 + 2) < NQ) fetch_quad((s / 4 + 2) < NQ ? (s / 4 + 2) : 0);
        if (s + 1 < W) Mnext = em[(s + 1) < W ? (s + 1) : 0] + Xp[s];
        Iv = MATCH + Yp[s];
        Dv = zleft;
        const double di = dmax(Dv, Iv);
        if (FIN) { if (Wl == s + 1) res_cap = dmax(di, Mv); }
        const double t2 = di + cd;
        const double mf = Mv + cf;
        Xp[s] = dmax(Mv + ce, t2);
        Yp[s] = dmax(mf, Iv + ca);
        zleft = dmax(mf, Dv + cc);
        if (s + 1 < W) asm volatile("" : "+v"(Xp[s]), "+v"(Yp[s]), "+v"(zleft), "+v"(Mnext));
        else asm volatile("" : "+v"(Xp[s]), "+v"(Yp[s]), "+v"(zleft));
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < W) Mv = Mnext;
      }
      outX = Xp[W - 1];
      outZ = zleft;
    }
    const double kabs = STEM ? fmax(__builtin_fabs(kcur), __builtin_fabs(kcur2)) : __builtin_fabs(kcur);
    const uint64_t cert = __builtin_amdgcn_ballot_w64(certM >= __builtin_fma(kabs, cabs_up, thr0)) & active_mask;
    fmask = cert | (fmask << 1);
    return (~fmask & lastbit) != 0 ? 1 : 0;                    // every row of the last lane is watched
  };

  // ---- the stem: rows 1 .. p-1 ----
  {
    const int T = (nr - 1) + (L - 1);
    for (int t = 0; t < T; ++t) {
      if (step(BoolTag<false>{}, BoolTag<true>{}, t)) {
        // a row no lane certifies for every member: all of them take the exact body
        if (lane < count) note[lane] = first + lane;
        if (lane == 0) atomicAdd(F.stats + 0, 1u);
        return count;
      }
    }
  }
  // ---- park row p-1 once: X, Y of my columns; my X(p-1, j0-1) stays in a register ----
  const double leftX_fork = leftX;
#pragma unroll
  for (int s = 0; s < W; ++s) { park[s * 64 + lane] = Xp[s]; park[(W + s) * 64 + lane] = Yp[s]; }
  asm volatile("" ::: "memory");                               // (the tails LOAD the state: no forwarding of 2W live doubles across the member loop)

  // ---- one tail per member: rows p .. n_h - 1 ----
  int noted = 0;
  for (int k = 0; k < count; ++k) {
    const PairDesc* pp = A.pairs + first + k;
    const int n = uni(pp->n);
    const int64_t out_idx = uni64(pp->out_idx);
    nr = n - rb;                                               // >= 2: the host keeps p <= n - 1
    hs = A.hap_codes + uni64(pp->hap_off) - 63 + rb;
    hrs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)hs), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int s = 0; s < W; ++s) { Xp[s] = park[s * 64 + lane]; Yp[s] = park[(W + s) * 64 + lane]; }
    leftX = leftX_fork;
    outX = Xp[W - 1];
    outZ = IMP;
    fmask = ~0ull;
    h_next = hrow_at(0);
    { const double2 b1 = ((const double2*)A.colXZ)[e01 + 2 * (rb + 1)]; bX_next = b1.x; bZ_next = b1.y; }
    bso = 2 * (rb + 2) * (int)sizeof(double2);
    kd = (double)((n - m) - (rb + 1 - lane) + j0);
    const int T = (nr - 1) + (L - 1);
    int bad = 0;
    for (int t = 0; t < T - 1 && !bad; ++t) bad = step(BoolTag<false>{}, BoolTag<false>{}, t);
    if (!bad) bad = step(BoolTag<true>{}, BoolTag<false>{}, T - 1);
    int why = bad ? 2 : 0;
    double S = 0.0;
    if (!bad) {
      S = lane_bcast(res_cap, L - 1);
      if (!(S > U)) why = 1;                                   // the acceptance rule: a path through a lowered cell could be the best one
    }
    if (why) {
      if (lane == 0) { note[noted] = first + k; atomicAdd(F.stats + why, 1u); }
      ++noted;
    } else if (lane == 0) A.out_ll[out_idx] = S;
  }
  return noted;
}

// A real call per family (class_walk_call's reasons: every strip width keeps its own register allocation, the kernel arguments
// come from the kernel's own argument segment, the LDS tables travel as LDS addresses); a leaf: the exact bodies of the members
// it notes are called from the kernel (ltr_dp_plan.hpp's reasons).
template <int W>
__device__ __forceinline__ int family_walk_from_kernarg(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v) {
  const KernelArgs& A = *(const KernelArgs*)(KernArgPtr)(uintptr_t)uni64(kernarg_v);
  const FamilyArgs& F = *(const FamilyArgs*)(FamArgPtr)(uintptr_t)(uni64(kernarg_v) + (int64_t)kFamilyArgsOffset);
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const double* emit_tab = (const double*)(LdsDoubles)(uintptr_t)(unsigned)uni((int)emit_lds_v);
  int* note = (int*)(LdsInts)(uintptr_t)(unsigned)uni((int)note_lds_v);
  double* park = F.park + ((size_t)blockIdx.x * kBlockWaves + wave) * (size_t)kFamilyParkDoubles;
  return family_walk<W>(A, F, uni(fi_v), lane, emit_tab, note, park);
}
template <int W>                                               // the wide band: W 11 .. 20
__device__ __attribute__((noinline)) int family_walk_call(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v) {
  return family_walk_from_kernarg<W>(kernarg_v, fi_v, emit_lds_v, note_lds_v);
}
template <int W>                                               // the narrow band: W 6 .. 10, the same walk ([2W][64] of the same park block)
__device__ __attribute__((noinline)) int family_narrow_call(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v) {
  return family_walk_from_kernarg<W>(kernarg_v, fi_v, emit_lds_v, note_lds_v);
}

// ---- A family along a SPINE ------------------------------------------------------------------------------------------------------
// A plain family shares rows 0 .. p-1, p the smallest pairwise common prefix.  The windows of a tandem-repeat locus are flank + unit
// x k + flank: an allele of 27 copies and one of 23 share three more units with each other than with the 20-copy allele that fixes
// p, and every plain tail scores those rows again.  A family with a spine (FamilySpine, chosen on the host: ltrp choose_spine) runs
// ONE stream along the window of one member, rows 1 .. n_s - 1, and every other member k leaves it at a park row R_k <= f_k =
// max(p, min(lcp(spine, k), n_k - 1)): its tail is rows R_k .. n_k - 1 from the parked state of row R_k - 1.  At most
// kFamilyParkSlots rows are parked per family (slot 0: p); a slot is X, Y of every column and X(row - 1, j0 - 1) of every lane.
// Why it stays bit-exact.  The lowered cells are still exactly row 0, columns >= p.  Rows p .. R_k - 1 of the spine member are
// member k's own rows -- its window is the spine member's up to f_k >= R_k -- so every value of the stream is still a lower bound
// of member k's value there, bit-identical whenever the best path avoids the lowered cells, and U still bounds every path through
// one: the acceptance rule S > U and redo_dispatch carry over unchanged.  The certificate: up to row p - 1 the family's range
// dd_min .. dd_max as the stem's; from a park row on the range of the members that still use the stream's rows -- those of later
// slots and the spine member -- which covers every member the row belongs to.  A row of the stream that fails: below p every member
// takes the exact body (a stem failure); from p on the members whose park row lies at or below it run their tails as usual -- their
// slot was complete and every row under it certified -- and the others, the spine member among them, take the exact body (tail
// failures).  The spine member's score is the stream's last step.
template <int W>
__device__ __forceinline__ int spine_walk(const KernelArgs& A, const FamilyArgs& F, const int fi, const int lane,
                                           const double* emit_tab, int* note, int* spl, double* park) {
  const FamilyDesc* __restrict__ fd = F.fams + fi;
  const FamilySpine* __restrict__ sp = F.spines + fi;
  const int first = uni(fd->first), count = uni(fd->count), p = uni(fd->p);
  const int dd_lo = uni(fd->dd_min), dd_hi = uni(fd->dd_max);
  const PairDesc* pp0 = A.pairs + first;
  const int spine = uni((int)sp->spine), n_slots = uni((int)sp->n_slots);
  const PairDesc* pps = pp0 + spine;                           // the member the stream follows
  // ---- the spine record, once per family, to this wavefront's LDS words (kSpineLds*): inside the stream's loop a lane reads its
  // slot's row and range with an index of its own, and an LDS read waits on lgkmcnt -- no vector-memory counter, so nothing there
  // waits for the park stores.  (Written and read by this wavefront alone, in its program order: LDS serves a wavefront in order.)
  if (lane <= 16) spl[kSpineLdsRow + lane] = lane < n_slots ? (int)sp->slot_row[min(lane, kFamilyParkSlots - 1)] : kSpineNoRow;
  if (lane < kFamilyParkSlots) { spl[kSpineLdsDdMin + lane] = (int)sp->slot_dd_min[lane]; spl[kSpineLdsDdMax + lane] = (int)sp->slot_dd_max[lane]; }
  if (lane < kFamilyMaxMembers) spl[kSpineLdsSlotOf + lane] = (int)sp->slot_of[lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int m = uni(pp0->m);
  const uint8_t* __restrict__ read = A.read_bytes + uni64(pp0->read_off);
  const double ca = A.mc.a, cc = A.mc.c, cd = A.mc.d, ce = A.mc.e, cf = A.mc.f, cg = A.mc.g, cb = A.mc.b;
  const double MATCH = A.mc.match, MISMATCH = A.mc.mismatch;
  const float c32 = A.mc.c;
  const double IMP = kImp;
  const double* __restrict__ lpc = A.lpc;
  const int C = m - 1;
  const int L = (C + W - 1) / W;                               // active lanes (one column block)
  const int Wl = C - (L - 1) * W;                              // real columns of the last lane, 1..W
  const int j0 = 1 + lane * W;
  int rb = 0;                                                  // a tail's row base: the row whose state its slot holds

  // ---- row 0 of the stream (HapAligner.cpp:263-272): columns below the fork as every member has them, the others lowered ----
  double Xp[W], Yp[W];
  constexpr int NQ = (W + 3) / 4;
  uint32_t rc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) rc[q] = 0;
  int e01;
  double emit00;
  {
    const uint8_t* __restrict__ hap = A.hap_bytes + uni64(pps->hap_off);
    const uint32_t r0 = (uint32_t)uni((int)read[0]);
    const int h0 = uni((int)hap[0]);
    emit00 = (h0 == (int)r0) ? MATCH : MISMATCH;               // match_matrix[0], :265
    e01 = (h0 == uni((int)read[1])) ? 1 : 0;                   // emission of the whole first column, :276
#pragma unroll
    for (int s = 0; s < W; ++s) {
      const int jc = min(j0 + s, m - 1);
      const double lp1 = lpc[max(jc - 1, 0)], lp = lpc[jc];
      const uint32_t hb = (uint32_t)hap[min(jc, p - 1)];
      const double D0jm1 = (jc == 1) ? IMP : (cg + lp1);
      const double D0j = cg + lp;
      const bool eq = (jc < p) & (hb == r0);                   // (columns from the fork on: MISMATCH, <= every member's cell)
      const double M0 = (D0jm1 + cd) + (eq ? MATCH : MISMATCH);
      Xp[s] = dmax(M0 + ce, dmax(D0j + cd, IMP + cb));
      Yp[s] = dmax(M0 + cf, IMP + ca);
      rc[s / 4] |= (((uint32_t)read[jc] >> 1) & 3u) << (2 * (s % 4) + 4);
      if ((s % 4) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the largest value a lowered cell can hold for any member (row 0's own expression at column p)
  const double U = ((cg + lpc[p - 1]) + cd) + MATCH;

  double outX = Xp[W - 1];
  double leftX = wave_shr1(outX, dmax(emit00 + ce, dmax(IMP + cd, IMP + cb)));
  double outZ = IMP;
  uint64_t fmask = ~0ull;
  const uint64_t lastbit = 1ull << (L - 1);
  double certM = 0.0;
  double res_cap = 0.0;
  // per-phase state of the step (the stream: the spine member's window, rows 1 .. n_s-1; a tail: the member's window from its park row)
  int nr = uni(pps->n);                                        // rows of the phase counted from its base: lane l is active on steps l .. l + nr - 2
  const uint16_t* hs = A.hap_codes + uni64(pps->hap_off) - 63;
  const uint32_t hoff = 64u - (uint32_t)lane;                  // (hs + t)[hoff] = row base + t + 1 - lane
  __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)hs), 0, 0x7fffffff, 0x00020000);
  const int hvo = (int)(hoff * (uint32_t)sizeof(uint16_t));
  auto hrow_at = [&](const int t) __attribute__((always_inline)) -> uint32_t {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(hrs, hvo, t * 2, 0);
  };
  typedef double d2v_t __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)((const double2*)A.colXZ + e01)), 0, 0x7fffffff, 0x00020000);
  uint32_t h_next = hrow_at(0);
  double bX_next, bZ_next;
  int bso = 2 * 2 * (int)sizeof(double2);                      // -> record 2: lane 0's row at step 1
  { const double2 b1 = ((const double2*)A.colXZ)[e01 + 2 * 1]; bX_next = b1.x; bZ_next = b1.y; }
  // band offset k of (my row, j0) for the smallest and the largest n - m of the family; -1 per step
  double kd = (double)(dd_lo - (1 - lane) + j0), kd2 = (double)(dd_hi - (1 - lane) + j0);
  const double cabs_up = fabs((double)c32) * (1.0 + 0x1p-22);
  const double thr0 = -600.0 + 1e-6;

  // One wavefront step of column_block's certificate body (FIRST, final block, SYM, LUT), as family_walk's.  STEM: the stream -- the
  // threshold of the member furthest from the diagonal among those the lane's row belongs to (kd, kd2: the ends of their range);
  // FIN: the last step of the stream or of a tail, which captures the member's result.
  auto step = [&](auto fin_tag, auto stem_tag, const int t) __attribute__((always_inline)) {
    constexpr bool FIN = decltype(fin_tag)::value;
    constexpr bool STEM = decltype(stem_tag)::value;
    const uint32_t h = h_next;
    const double bX = bX_next, bZ = bZ_next;
    h_next = hrow_at(t + 1);
    {
      const d2v_t bn = __builtin_bit_cast(d2v_t, __builtin_amdgcn_raw_buffer_load_b128(brs, 0, bso, 0));
      bso += 2 * (int)sizeof(double2); bX_next = bn.x; bZ_next = bn.y;
    }
    const double mX = wave_shr1(outX, bX);
    const double mZ = wave_shr1(outZ, bZ);
    const double kcur = kd, kcur2 = kd2;
    kd = kcur - 1.0;
    if (STEM) kd2 = kcur2 - 1.0;
    const int a_hi = min(t, L - 1), a_lo = max(t - (nr - 2), 0);
    const uint64_t active_mask = (~0ull >> (63 - a_hi)) & (~0ull << a_lo);
    const bool active = __builtin_amdgcn_inverse_ballot_w64(active_mask);
    if (active) {
      double diag = leftX;
      leftX = mX;
      double zleft = mZ;
      double Iv = 0.0, Dv = 0.0;
      double em[W];
      auto fetch_quad = [&](const int q) __attribute__((always_inline)) {
        const double2* row = (const double2*)((const char*)emit_tab + (h + rc[q < NQ ? q : 0]));
        const double2 lo = row[0];
        em[4 * q] = lo.x;
        if (4 * q + 1 < W) em[(4 * q + 1) < W ? (4 * q + 1) : 0] = lo.y;
        if (4 * q + 2 < W) {
          const double2 hi = row[kEmitTabDoubles / 4];
          em[(4 * q + 2) < W ? (4 * q + 2) : 0] = hi.x;
          if (4 * q + 3 < W) em[(4 * q + 3) < W ? (4 * q + 3) : 0] = hi.y;
        }
      };
      fetch_quad(0);
      if (NQ > 1) fetch_quad(1 < NQ ? 1 : 0);
      certM = em[0] + diag;
      double Mv = certM;
#pragma unroll
      for (int s = 0; s < W; ++s) {
        double Mnext = 0.0;
        if ((s % 4) == 2 && (s / 4 + 2) < NQ) fetch_quad((s / 4 + 2) < NQ ? (s / 4 + 2) : 0);
        if (s + 1 < W) Mnext = em[(s + 1) < W ? (s + 1) : 0] + Xp[s];
        Iv = MATCH + Yp[s];
        Dv = zleft;
        const double di = dmax(Dv, Iv);
        if (FIN) { if (Wl == s + 1) res_cap = dmax(di, Mv); }
        const double t2 = di + cd;
        const double mf = Mv + cf;
        Xp[s] = dmax(Mv + ce, t2);
        Yp[s] = dmax(mf, Iv + ca);
        zleft = dmax(mf, Dv + cc);
        if (s + 1 < W) asm volatile("" : "+v"(Xp[s]), "+v"(Yp[s]), "+v"(zleft), "+v"(Mnext));
        else asm volatile("" : "+v"(Xp[s]), "+v"(Yp[s]), "+v"(zleft));
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < W) Mv = Mnext;
      }
      outX = Xp[W - 1];
      outZ = zleft;
    }
    const double kabs = STEM ? fmax(__builtin_fabs(kcur), __builtin_fabs(kcur2)) : __builtin_fabs(kcur);
    const uint64_t cert = __builtin_amdgcn_ballot_w64(certM >= __builtin_fma(kabs, cabs_up, thr0)) & active_mask;
    fmask = cert | (fmask << 1);
    return (~fmask & lastbit) != 0 ? 1 : 0;                    // every row of the last lane is watched
  };

  // ---- the stream: rows 1 .. n_s - 1 of the spine member, no drain at p.  A lane parks a park row's state -- X, Y of its columns
  // and X(row - 1, j0 - 1) -- when its own row reaches row - 1 (step row - 2 + lane: the lanes reach a row on different steps, and
  // park rows closer than L rows are in flight together), and from that row on tests against the members still on the spine.
  // A parking step does not wait for memory: the lane's chunk of the slot is 2W+2 consecutive doubles (ltr_dp_types.h: lane-major),
  // W+1 16-byte stores from one address; the slot's row and range come from the LDS copy; and the step's two prefetches (the next
  // haplotype row code, the next column-0 record) are waited for BEFORE the branch, a step after they were issued, so that the
  // stores are the youngest vector-memory operations in flight and no wait of that step covers them ----
  constexpr int CH = 2 * W + 2;                                // doubles of a lane's chunk
  constexpr int SLOT = 64 * CH;                                // ... of a slot at this width
  double* const chunk0 = park + lane * CH;                     // my chunk of slot 0
  int pk = p - 2 + lane;                                       // the step after which I park my next slot
  int psl = 0;                                                 // ... which slot that is
  auto park_if = [&](const int t) __attribute__((always_inline)) {
    asm volatile("" : "+v"(h_next), "+v"(bX_next), "+v"(bZ_next));
    if (t == pk) {
      d2v_t* sl = (d2v_t*)(chunk0 + psl * SLOT);
#pragma unroll
      for (int i = 0; i <= W; ++i) {                           // X[0 .. W-1], Y[0 .. W-1], leftX, pad (at odd W one pair is X[W-1], Y[0])
        const int a = 2 * i, b = 2 * i + 1;
        d2v_t v;
        v.x = a < W ? Xp[a < W ? a : 0] : (a < 2 * W ? Yp[a < 2 * W ? a - W : 0] : leftX);
        v.y = b < W ? Xp[b < W ? b : 0] : (b < 2 * W ? Yp[b < 2 * W ? b - W : 0] : leftX);
        sl[i] = v;
      }
      const int R = spl[kSpineLdsRow + psl];
      kd = (double)(spl[kSpineLdsDdMin + psl] - R + j0); kd2 = (double)(spl[kSpineLdsDdMax + psl] - R + j0);   // (my next row is R)
      ++psl;
      pk = spl[kSpineLdsRow + psl] - 2 + lane;                 // (from n_slots on: kSpineNoRow, a step that never comes)
    }
  };
  int bad = 0, t_bad = 0;
  {
    const int T = (nr - 1) + (L - 1);
    // (step 0's operands are waited for here: the loop is then entered with no load pending, as it is by its back edge, and the
    // wait that a pending load at the loop's head would need -- one that also drains the stores of the step before -- is not there)
    asm volatile("" : "+v"(h_next), "+v"(bX_next), "+v"(bZ_next));
    for (int t = 0; t < T - 1; ++t) {
      if (step(BoolTag<false>{}, BoolTag<true>{}, t)) { bad = 1; t_bad = t; break; }
      park_if(t);
    }
    if (!bad) {
      bad = step(BoolTag<true>{}, BoolTag<true>{}, T - 1);
      t_bad = T - 1;
      park_if(T - 1);
    }
  }
  // (the tails LOAD the state.  A compile-only barrier is enough because every lane reloads exactly the addresses it stored itself
  // -- its own chunk of the slot --, in program order of its own wavefront: a read of another lane's doubles would need more than this)
  asm volatile("" ::: "memory");
  // the row no lane certifies (it is noticed when it reaches the last lane); every row below it passed, and a slot whose row is at
  // or below it is complete: the last lane parked it when it finished the row before
  const int r_bad = bad ? t_bad + 1 - (L - 1) : 0x7fffffff;
  if (r_bad < p) {
    // a row below the fork no lane certifies for every member: all of them take the exact body
    if (lane < count) note[lane] = first + lane;
    if (lane == 0) atomicAdd(F.stats + 0, 1u);
    return count;
  }
  int noted = 0;
  // ---- the spine member: its result is the stream's ----
  {
    int why = bad ? 2 : 0;
    double S = 0.0;
    if (!bad) {
      S = lane_bcast(res_cap, L - 1);
      if (!(S > U)) why = 1;
    }
    if (why) {
      if (lane == 0) { note[noted] = first + spine; atomicAdd(F.stats + why, 1u); }
      ++noted;
    } else if (lane == 0) A.out_ll[uni64(pps->out_idx)] = S;
  }
  // ---- one tail per other member: rows slot_row .. n_h - 1 from its slot (family_walk's tails with a row base of their own) ----
  for (int k = 0; k < count; ++k) {
    if (k == spine) continue;
    const PairDesc* pp = A.pairs + first + k;
    const int slot = uni(spl[kSpineLdsSlotOf + k]);
    const int R = uni(spl[kSpineLdsRow + slot]);
    if (R > r_bad) {                                           // its slot is not complete: the spine's certificate failed below its park row
      if (lane == 0) { note[noted] = first + k; atomicAdd(F.stats + 2, 1u); }
      ++noted;
      continue;
    }
    const int n = uni(pp->n);
    const int64_t out_idx = uni64(pp->out_idx);
    rb = R - 1;
    nr = n - rb;                                               // >= 2: the host keeps every park row <= n - 1
    hs = A.hap_codes + uni64(pp->hap_off) - 63 + rb;
    hrs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)uni64((int64_t)(uintptr_t)hs), 0, 0x7fffffff, 0x00020000);
    const d2v_t* sl = (const d2v_t*)(chunk0 + slot * SLOT);
#pragma unroll
    for (int i = 0; i <= W; ++i) {                             // my chunk as I stored it: W+1 16-byte loads
      const d2v_t v = sl[i];
      const int a = 2 * i, b = 2 * i + 1;
      if (a < W) Xp[a < W ? a : 0] = v.x; else if (a < 2 * W) Yp[a < 2 * W ? a - W : 0] = v.x; else leftX = v.x;
      if (b < W) Xp[b < W ? b : 0] = v.y; else if (b < 2 * W) Yp[b < 2 * W ? b - W : 0] = v.y;
    }
    outX = Xp[W - 1];
    outZ = IMP;
    fmask = ~0ull;
    h_next = hrow_at(0);
    { const double2 b1 = ((const double2*)A.colXZ)[e01 + 2 * (rb + 1)]; bX_next = b1.x; bZ_next = b1.y; }
    bso = 2 * (rb + 2) * (int)sizeof(double2);
    kd = (double)((n - m) - (rb + 1 - lane) + j0);
    const int T = (nr - 1) + (L - 1);
    int tbad = 0;
    for (int t = 0; t < T - 1 && !tbad; ++t) tbad = step(BoolTag<false>{}, BoolTag<false>{}, t);
    if (!tbad) tbad = step(BoolTag<true>{}, BoolTag<false>{}, T - 1);
    int why = tbad ? 2 : 0;
    double S = 0.0;
    if (!tbad) {
      S = lane_bcast(res_cap, L - 1);
      if (!(S > U)) why = 1;                                   // the acceptance rule: a path through a lowered cell could be the best one
    }
    if (why) {
      if (lane == 0) { note[noted] = first + k; atomicAdd(F.stats + why, 1u); }
      ++noted;
    } else if (lane == 0) A.out_ll[out_idx] = S;
  }
  return noted;
}

// The calls of a family with a spine (the reasons of family_walk_call; names of their own: the plain families' bodies stay what they were).
template <int W>
__device__ __forceinline__ int spine_walk_from_kernarg(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v, unsigned spine_lds_v) {
  const KernelArgs& A = *(const KernelArgs*)(KernArgPtr)(uintptr_t)uni64(kernarg_v);
  const FamilyArgs& F = *(const FamilyArgs*)(FamArgPtr)(uintptr_t)(uni64(kernarg_v) + (int64_t)kFamilyArgsOffset);
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const double* emit_tab = (const double*)(LdsDoubles)(uintptr_t)(unsigned)uni((int)emit_lds_v);
  int* note = (int*)(LdsInts)(uintptr_t)(unsigned)uni((int)note_lds_v);
  int* spl = (int*)(LdsInts)(uintptr_t)(unsigned)uni((int)spine_lds_v);
  double* park = F.park + ((size_t)blockIdx.x * kBlockWaves + wave) * (size_t)kFamilyParkDoubles;
  return spine_walk<W>(A, F, uni(fi_v), lane, emit_tab, note, spl, park);
}
template <int W>                                               // the wide band: W 11 .. 20
__device__ __attribute__((noinline)) int spine_wide_call(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v, unsigned spine_lds_v) {
  return spine_walk_from_kernarg<W>(kernarg_v, fi_v, emit_lds_v, note_lds_v, spine_lds_v);
}
template <int W>                                               // the narrow band: W 6 .. 10
__device__ __attribute__((noinline)) int spine_narrow_call(int64_t kernarg_v, int fi_v, unsigned emit_lds_v, unsigned note_lds_v, unsigned spine_lds_v) {
  return spine_walk_from_kernarg<W>(kernarg_v, fi_v, emit_lds_v, note_lds_v, spine_lds_v);
}

// Persistent: the families are dealt STATICALLY, wavefront w of G takes families w, 2G-1-w, 2G+w, .. of the list (sorted by
// modelled cost, largest first: snake order evens the waves' sums out) -- no work counter, no pop.
__global__ __launch_bounds__(64 * kBlockWaves, 3) void ltr_dp_family_kernel(KernelArgs A, FamilyArgs F) {
  __shared__ __attribute__((aligned(16))) double s_emit[kEmitTabDoubles];
  __shared__ double s_pen[kPenTabDoubles];                     // the exact thresholds of the in-line redo (kModeThr)
  __shared__ int s_note[kBlockWaves][kFamilyMaxMembers];       // per wave: members waiting for the exact body
  __shared__ int s_spine[kBlockWaves][kSpineLdsInts];          // per wave: the spine record of the family it runs (spine_walk)
  for (int idx = threadIdx.x; idx < kEmitTabDoubles; idx += 64 * kBlockWaves) {
    const int half = idx >> 11, hcode = (idx >> 9) & 3, quad = (idx >> 1) & 255, k = 2 * half + (idx & 1);
    s_emit[idx] = (hcode == ((quad >> (2 * k)) & 3)) ? (double)A.mc.match : (double)A.mc.mismatch;
  }
  if (A.thr_ok) for (int idx = threadIdx.x; idx < kPenTabDoubles; idx += 64 * kBlockWaves) s_pen[idx] = A.thr_tab[idx];
  __syncthreads();
  const int wave = uni((int)(threadIdx.x >> 6));
  const unsigned emit_lds = (unsigned)(uintptr_t)(LdsDoubles)s_emit;
  const unsigned pen_lds = (unsigned)(uintptr_t)(LdsDoubles)s_pen;
  const unsigned note_lds = (unsigned)(uintptr_t)(LdsInts)s_note[wave];
  const unsigned spine_lds = (unsigned)(uintptr_t)(LdsInts)s_spine[wave];
  const int64_t kargs = (int64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  const int G = (int)gridDim.x * kBlockWaves, my_wave = (int)blockIdx.x * kBlockWaves + wave;
  const int n_f = F.n_fams;
  const unsigned long long t_first = F.wave_clock ? wall_clock64() : 0ull;   // (measurement aid, as the plan kernel's: when this wavefront started ..)
  for (int64_t base = 0, round = 0; base < n_f; base += G, ++round) {
    const int64_t f64 = base + ((round & 1) ? (G - 1 - my_wave) : my_wave);
    if (f64 >= n_f) continue;
    const int fi = (int)f64;
    const int w = uni(F.fams[fi].W);
    int noted;
    if (uni((int)F.spines[fi].spine) >= 0) switch (w) {
      case 6: noted = spine_narrow_call<6>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 7: noted = spine_narrow_call<7>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 8: noted = spine_narrow_call<8>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 9: noted = spine_narrow_call<9>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 10: noted = spine_narrow_call<10>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 11: noted = spine_wide_call<11>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 12: noted = spine_wide_call<12>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 13: noted = spine_wide_call<13>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 14: noted = spine_wide_call<14>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 15: noted = spine_wide_call<15>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 16: noted = spine_wide_call<16>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 17: noted = spine_wide_call<17>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 18: noted = spine_wide_call<18>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      case 19: noted = spine_wide_call<19>(kargs, fi, emit_lds, note_lds, spine_lds); break;
      default: noted = spine_wide_call<20>(kargs, fi, emit_lds, note_lds, spine_lds); break;
    }
    else switch (w) {
      case 6: noted = family_narrow_call<6>(kargs, fi, emit_lds, note_lds); break;
      case 7: noted = family_narrow_call<7>(kargs, fi, emit_lds, note_lds); break;
      case 8: noted = family_narrow_call<8>(kargs, fi, emit_lds, note_lds); break;
      case 9: noted = family_narrow_call<9>(kargs, fi, emit_lds, note_lds); break;
      case 10: noted = family_narrow_call<10>(kargs, fi, emit_lds, note_lds); break;
      case 11: noted = family_walk_call<11>(kargs, fi, emit_lds, note_lds); break;
      case 12: noted = family_walk_call<12>(kargs, fi, emit_lds, note_lds); break;
      case 13: noted = family_walk_call<13>(kargs, fi, emit_lds, note_lds); break;
      case 14: noted = family_walk_call<14>(kargs, fi, emit_lds, note_lds); break;
      case 15: noted = family_walk_call<15>(kargs, fi, emit_lds, note_lds); break;
      case 16: noted = family_walk_call<16>(kargs, fi, emit_lds, note_lds); break;
      case 17: noted = family_walk_call<17>(kargs, fi, emit_lds, note_lds); break;
      case 18: noted = family_walk_call<18>(kargs, fi, emit_lds, note_lds); break;
      case 19: noted = family_walk_call<19>(kargs, fi, emit_lds, note_lds); break;
      default: noted = family_walk_call<20>(kargs, fi, emit_lds, note_lds); break;
    }
    noted = uni(noted);
    for (int k = 0; k < noted; ++k) {
      const int pi = uni(s_note[wave][k]);
      redo_dispatch<true>(A, kargs, pi, uni(A.pairs[pi].m) - 1, emit_lds, pen_lds);
    }
  }
  if (F.wave_clock && (threadIdx.x & 63) == 0) {               // (.. and when it left: the spread of the static deal)
    F.wave_clock[2 * my_wave] = t_first; F.wave_clock[2 * my_wave + 1] = wall_clock64();
  }
}
