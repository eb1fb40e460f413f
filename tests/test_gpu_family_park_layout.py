"""-m gpu: the lane-major park slots of a family along a spine (csrc/ltr_dp_family.hpp, spine_walk; csrc/ltr_dp_types.h): a lane's
chunk of a slot is 2W+2 consecutive doubles -- X and Y of its W columns, X of the column left of its strip, a pad -- written by W+1
16-byte stores when the lane parks and read back by W+1 16-byte loads when a tail starts; the slots of a family are dense at the
family's own width.  tests/test_gpu_families_spine.py and tests/test_gpu_grid_cap.py park at every strip width; here is what the
layout adds: odd and even widths (at odd W one 16-byte pair holds X[W-1] and Y[0]), all 64 lanes with a full last lane and with a
single real column in it, families of different widths one after the other on one wavefront (its park block reused with another
stride, stale doubles of the wider family between the narrower one's chunks), and twelve fork rows for the slots there are (every
slot used, members that start from the nearest kept row below their own).  One-read loci of four to twelve alleles, spines on
request; every score bit-identical to the same plan without families, with plain families and to the CPU oracle."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

import test_gpu_families_spine as sp

pytestmark = pytest.mark.gpu

WIDTHS = [6, 7, 19, 20]


def _tr_locus(rng, C, prefix_len, unit_len, copies, read_of, n_sub=3, extra=0):
    """One read of C columns against the windows prefix + unit x k + suffix, k in copies; the read is the window of copies[read_of]
    (its first C + 1 bases where the windows are `extra` bases longer than the read) with n_sub substitutions."""
    m = C + 1
    unit = sp._seq(rng, unit_len)
    prefix = sp._seq(rng, prefix_len - 1) + sp._other(unit[-1])
    suffix = sp._other(unit[0]) + sp._seq(rng, m - prefix_len - unit_len * copies[read_of] - 1 + extra)
    wins = sp._tr(prefix, unit, copies, suffix)
    assert len(wins[read_of]) == m + extra
    return [sp._mutate(rng, wins[read_of][:m], n_sub)], [sp._hap(rng, w) for w in wins]


@pytest.mark.parametrize("W", WIDTHS)
def test_odd_and_even_widths_on_64_lanes(gpu_ctx, W):
    """Read columns 64 W (64 lanes, the last one full) and 63 W + 1 (64 lanes, the last one holds a single real column); per count
    the two loci of test_gpu_families_spine.edge_loci: four alleles, three park rows, closer than a wavefront is long and further."""
    cols = [(64 * W, W), (63 * W + 1, W)]
    for C, _ in cols:
        L = -(-C // W)
        assert -(-C // 64) == W and L == 64 and C - (L - 1) * W in (W, 1)
    loci, want = sp.edge_loci(np.random.default_rng(1000 + W), cols)
    st, st_plain, formed = sp._check(gpu_ctx, loci)
    assert len(formed["families"]) == 4 == formed["with_spine"]
    for f in formed["families"]:
        assert f["W"] == W and f["count"] == 4 and f["spine"] == 2 and f["slots"] == 3
        assert (f["W"], f["p"], (f["slot_rows"][1] - f["p"], f["slot_rows"][2] - f["p"])) in want, f
    assert sp._clean(st) and sp._clean(st_plain), (st, st_plain)


@pytest.mark.parametrize("W", WIDTHS)
def test_twelve_fork_rows_for_the_slots_there_are(gpu_ctx, W):
    """Twelve alleles of 10 .. 21 copies of a 2-base unit: twelve distinct fork rows, so every slot is used and the members whose
    row was not kept start from the nearest kept row below it."""
    C = 64 * W - 3
    locus = _tr_locus(np.random.default_rng(2000 + W), C, C // 2, 2, tuple(range(10, 22)), read_of=6)
    st, st_plain, formed = sp._check(gpu_ctx, [locus])
    (f,) = formed["families"]
    assert f["W"] == W and f["count"] == 12 and f["spine"] >= 0 and len(set(f["fork"])) == 12
    assert f["slots"] == f["park_slots"] == formed["park_slots"]
    others = [k for k in range(12) if k != f["spine"]]
    assert sorted({f["slot"][k] for k in others}) == list(range(f["slots"]))                    # every slot is some member's
    assert all(f["slot_rows"][f["slot"][k]] <= f["fork"][k] for k in others)
    losers = [k for k in others if f["slot_rows"][f["slot"][k]] < f["fork"][k]]
    assert len(losers) == len({f["fork"][k] for k in others}) - f["slots"] > 0, (f, losers)     # (the others' rows are distinct: one loser per row not kept)
    assert sp._clean(st) and sp._clean(st_plain), (st, st_plain)


def _mixed_loci(rng):
    """Four families each, in the order the launch deals them (modelled cost, largest first): twelve alleles on strips of 6 with
    long tails, four alleles on strips of 20 that fork near their end, four alleles on strips of 6."""
    loci = [_tr_locus(rng, 384, 130, 2, tuple(range(10, 22)), read_of=6, n_sub=1, extra=90) for _ in range(4)]
    loci += [_tr_locus(rng, 1217, 1190, 2, (4, 6, 5, 8), read_of=2) for _ in range(4)]
    loci += [_tr_locus(rng, 379, 250, 2, (10, 11, 13, 16), read_of=1) for _ in range(4)]
    return loci


def _run_capped(ctx, batch, families):
    try:
        ctx.set_debug("families", families)
        ctx.set_debug("family_min_rows", 0)
        ctx.set_debug("family_spine", 1)
        ctx.set_debug("grid_cap", 1)
        plan = ctx.plan(batch)
        plan.execute()
        ll, _ = plan.fetch()
        st = plan.family_stats()
        st.update(plan.family_spine_stats())
        launches = _lib.debug_last_launches(plan=plan)
        plan.close()
    finally:
        ctx.set_debug("reset", 0)
    return ll, st, launches


def test_mixed_widths_on_one_wavefront(gpu_ctx):
    """One workgroup (grid_cap 1): its four wavefronts take family after family of the static deal, and each of them runs a family
    on strips of 6 (eight slots of 14 doubles a lane), then one on strips of 20 (three slots of 42 doubles a lane, over the chunks
    of the narrow one), then one on strips of 6 again (over the wide one's, whose doubles stay between its chunks)."""
    import oracle_lib as ol
    batch = _abi.PackedBatch(_mixed_loci(np.random.default_rng(77)))
    formed = _lib.debug_plan_family_forks(batch, families=2, family_min_rows=0, family_spine=1)
    fams = formed["families"]
    assert len(fams) == 12 == formed["with_spine"] and all(f["spine"] >= 0 for f in fams)
    # the static deal of ltr_dp_family_kernel over G = 4 wavefronts: wavefront w takes families w, 2G-1-w, 2G+w, ..
    G = 4
    per_wave = [[fams[base + (G - 1 - w if (base // G) & 1 else w)]["W"] for base in range(0, len(fams), G)] for w in range(G)]
    print("strip widths per wavefront, in the order it runs them:", per_wave)
    pairs = {(a, b) for ws in per_wave for a, b in zip(ws, ws[1:])}
    assert (20, 6) in pairs and (6, 20) in pairs, per_wave
    ref, _, _ = ol.oracle_align_batch(batch, gpu_ctx.params)
    off, st_off, _ = _run_capped(gpu_ctx, batch, -1)
    on, st, launches = _run_capped(gpu_ctx, batch, 2)
    assert st_off["families"] == 0 and st["families"] == 12 == st["with_spine"]
    fam_launches = [L for L in launches if L["kind"] == "family"]
    assert [L["grid"] for L in fam_launches] == [1], launches
    for got in (off, on):
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))[:8]
    assert sp._clean(st), st
