"""-m gpu: haplotype families run along a spine (csrc/ltr_dp_family.hpp, spine_walk) on small crafted batches: scores bit-identical
to the CPU oracle, to the same plan without families and to the same plan with plain families (ltr_ctx_set_debug "family_spine" -1),
and the statistics show that the branch a case is built for really ran.  Shapes: every strip width 6 .. 20 at its lane edges with
park rows closer than a wavefront is long (a period of 2) and further apart (a period of 9), the shapes of
tests/test_plan_families_spine.py, more fork rows than park slots, a stream whose certificate fails between two park rows, the
acceptance rule failing, an asymmetric model."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

pytestmark = pytest.mark.gpu
FLANK = 30


def _seq(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


def _hap(rng, window):
    return _seq(rng, FLANK) + window + _seq(rng, FLANK)


def _other(base, avoid=b""):
    return bytes([next(c for c in b"ACGT" if c != base and c not in avoid)])


def _mutate(rng, s, n_sub, lo=0, hi=None):
    r = bytearray(s)
    for p in rng.choice(np.arange(lo, len(s) if hi is None else hi), size=n_sub, replace=False):
        r[p] = _other(r[p])[0]
    return bytes(r)


def _tr(prefix, unit, copies, suffix):
    return [prefix + unit * k + suffix for k in copies]


def _run(ctx, batch, families, spine=1, min_rows=0, params=None):
    try:
        if params is not None:
            ctx.set_params(params)
        ctx.set_debug("families", families)
        ctx.set_debug("family_min_rows", min_rows)
        ctx.set_debug("family_spine", spine)
        plan = ctx.plan(batch)
        plan.execute()
        ll, _ = plan.fetch()
        st = plan.family_stats()
        st.update(plan.family_spine_stats())
        plan.close()
    finally:
        ctx.set_debug("reset", 0)
        if params is not None:
            ctx.set_params(_abi.default_params())
    return ll, st


def _check(ctx, loci, families=2, min_rows=0, params=None):
    """Families on request along their spines against plain families, against none and against the oracle; returns the statistics
    of the run with spines, of the run with plain families, and what the host formed."""
    import oracle_lib as ol
    batch = _abi.PackedBatch(loci)
    ref, _, _ = ol.oracle_align_batch(batch, params or ctx.params)
    off, st_off = _run(ctx, batch, -1, params=params)
    plain, st_plain = _run(ctx, batch, families, -1, min_rows, params=params)
    on, st = _run(ctx, batch, families, 1, min_rows, params=params)      # (on request: by rule a plan this small keeps plain families)
    assert st_off["families"] == 0 and st_off["with_spine"] == 0 and st_plain["with_spine"] == 0 and st_plain["steps_saved"] == 0
    for got in (off, plain, on):
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))[:8]
    formed = _lib.debug_plan_family_forks(batch, params=params, families=families, family_min_rows=min_rows, family_spine=1)
    assert st["families"] == st_plain["families"] == len(formed["families"]) and st["members"] == st_plain["members"] == formed["members"]
    assert (st["with_spine"], st["steps_saved"]) == (formed["with_spine"], formed["steps_saved"])
    return st, st_plain, formed


def _clean(st):
    return st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0


# read columns at the lane edges of every strip width: the first and the last count of a width (tests/test_gpu_families.py,
# tests/test_gpu_families_narrow.py)
EDGE_COLUMNS = [(321, 6), (384, 6), (385, 7), (448, 7), (449, 8), (512, 8), (513, 9), (576, 9), (577, 10), (640, 10), (641, 11), (704, 11), (705, 12), (768, 12),
                (769, 13), (832, 13), (833, 14), (896, 14), (897, 15), (960, 15), (961, 16), (1024, 16), (1025, 17), (1088, 17), (1089, 18), (1152, 18),
                (1153, 19), (1216, 19), (1217, 20), (1280, 20)]


@pytest.mark.parametrize("cols", [EDGE_COLUMNS[:10], EDGE_COLUMNS[10:20], EDGE_COLUMNS[20:]], ids=["W6-10", "W11-15", "W16-20"])
def test_every_strip_width_parks_close_and_distant_rows(gpu_ctx, cols):
    loci, want = edge_loci(np.random.default_rng(sum(c for c, _ in cols)), cols)
    st, st_plain, formed = _check(gpu_ctx, loci)
    assert len(formed["families"]) == len(want) == formed["with_spine"]
    for f in formed["families"]:
        assert f["count"] == 4 and f["spine"] == 2 and f["slots"] == 3
        assert (f["W"], f["p"], (f["slot_rows"][1] - f["p"], f["slot_rows"][2] - f["p"])) in want, f
    assert sorted(f["W"] for f in formed["families"]) == sorted(w for w, _, _ in want)
    assert _clean(st) and _clean(st_plain), (st, st_plain)        # every member accepted from the stream or its tail


def edge_loci(rng, cols):
    """Per (read columns, strip width) two one-read loci of four alleles, three park slots each; and per locus (W, p, gaps of the
    later park rows) (test_every_strip_width_parks_close_and_distant_rows; tests/test_gpu_grid_cap.py)."""
    loci, want = [], []
    for C, W in cols:
        assert W == -(-C // 64)
        m = C + 1
        # a period of 2: park rows p, p + 2, p + 6 -- all in flight at once; a period of 9: p, p + 27, p + 99 -- the last further
        # than the 64 lanes of a wavefront from the one before
        for unit_len, copies, gaps in ((2, (60, 61, 63, 66), (2, 6)), (9, (20, 23, 40, 31), (27, 99))):
            unit = _seq(rng, unit_len)
            prefix = _seq(rng, 79) + _other(unit[-1])
            suffix = _other(unit[0]) + _seq(rng, m - 80 - unit_len * copies[1] - 1)
            wins = _tr(prefix, unit, copies, suffix)
            assert len(wins[1]) == m
            loci.append(([_mutate(rng, wins[1], 3)], [_hap(rng, w) for w in wins]))
            want.append((W, 80 + unit_len * copies[0], gaps))
    return loci, want


def _cpu_shapes(rng):
    """The shapes of tests/test_plan_families_spine.py (reads of 701 bases: strips of 11)."""
    unit = _seq(rng, 9)
    suffix = _other(unit[0]) + _seq(rng, 300)
    shapes = {"spine in the middle": _tr(_seq(rng, 150), unit, (20, 23, 27, 25), suffix)}
    suf_b = _other(unit[0], avoid=suffix[:1]) + suffix[1:-10]      # (the same tail behind a base of its own)
    prefix = _seq(rng, 150)
    shapes["two members at one fork row"] = [prefix + unit * 20 + suffix, prefix + unit * 27 + suffix, prefix + unit * 23 + suffix, prefix + unit * 23 + suf_b]
    prefix, suffix = _seq(rng, 100), _other(unit[0]) + _seq(rng, 330)
    long_ = prefix + unit * 30 + suffix
    q = 100 + 9 * 22 + 4
    z1 = long_[:q] + _other(long_[q]) + long_[q + 1:]
    z2 = z1[:q + 20] + _other(z1[q + 20]) + z1[q + 21:]
    shapes["a substitution inside the repeat"] = [prefix + unit * 20 + suffix, long_, prefix + unit * 29 + suffix, prefix + unit * 28 + suffix, z1, z2]
    y = _seq(rng, 720)
    a = y[:600] + _other(y[600]) + _seq(rng, 80)
    shapes["a prefix of the spine"] = [a, y, y[:690], y[:710] + _other(y[710]) + _seq(rng, 20)]
    shapes["the spine is a prefix"] = [a, y, y[:690]]
    unit6 = _seq(rng, 6)
    shapes["more fork rows than slots"] = _tr(_seq(rng, 120), unit6, range(60, 72), _other(unit6[0]) + _seq(rng, 199))
    x, t = _seq(rng, 300), _seq(rng, 400)
    shapes["nothing beyond p"] = [x + b"ACGT"[k:k + 1] + t[:380 + 10 * k] for k in range(3)]      # (related tails: a base of its own each)
    return shapes


def cpu_shape_loci(rng):
    """Two reads per shape of _cpu_shapes (test_the_shapes_of_the_cpu_test; tests/test_gpu_grid_cap.py).  (loci, number of shapes)"""
    shapes = _cpu_shapes(rng)
    loci = []
    for wins in shapes.values():
        # two reads near the second longest window, cut or padded to 701 bases
        w = sorted(wins, key=len)[-2]
        r = w[:701] if len(w) >= 701 else w + _seq(rng, 701 - len(w))
        reads = [_mutate(rng, r, 3), _mutate(rng, r, 5)]
        loci.append((reads, [_hap(rng, w) for w in wins]))
    return loci, len(shapes)


def test_the_shapes_of_the_cpu_test(gpu_ctx):
    loci, n_shapes = cpu_shape_loci(np.random.default_rng(31))
    st, st_plain, formed = _check(gpu_ctx, loci, families=1)
    assert len(formed["families"]) == 2 * n_shapes and formed["with_spine"] == 2 * (n_shapes - 1)
    by_count = lambda n: [f for f in formed["families"] if f["count"] == n]
    assert all(f["slots"] == f["park_slots"] and len(set(f["fork"])) == 12 for f in by_count(12))      # more fork rows than slots
    assert any(f["spine"] >= 0 and f["slot_rows"][-1] == max(f["fork"][k] for k in range(f["count"]) if k != f["spine"]) == f["fork"][f["spine"]]
               for f in by_count(3))                              # a member that leaves the spine at the spine's end
    assert _clean(st) and _clean(st_plain), (st, st_plain)


def failed_stream_locus(rng):
    """(locus, p) of test_a_stream_that_fails_between_two_park_rows."""
    unit = _seq(rng, 9)
    prefix, suffix = _seq(rng, 499) + _other(unit[-1]), _other(unit[0]) + _seq(rng, 59)
    wins = _tr(prefix, unit, (20, 23, 70, 68), suffix)
    p = 500 + 9 * 20
    read = bytearray(wins[2])
    read[p + 30:p + 400] = _seq(rng, 370)
    return ([bytes(read)], [_hap(rng, w) for w in wins]), p


def spine_rule_failure_locus(rng):
    """Read 0 fails the acceptance rule for all four members of a spine family, read 1 is clean
    (test_the_acceptance_rule_fails_for_a_spine_family)."""
    unit = _seq(rng, 9)
    wins = _tr(_seq(rng, 69) + _other(unit[-1]), unit, (4, 6, 9, 8), _other(unit[0]) + _seq(rng, 560))
    base = wins[2][:701] + _seq(rng, max(0, 701 - len(wins[2])))
    reads = [_mutate(rng, base, 15), _mutate(rng, base, 2)]
    return reads, [_hap(rng, w) for w in wins]


def test_a_stream_that_fails_between_two_park_rows(gpu_ctx):
    """Alleles of 20, 23, 70 and 68 copies of a 9-base unit behind 500 shared bases: the spine is the 70-copy allele, the others leave
    it at p, p + 27 and p + 432.  The read is that allele with 370 random bases from column p + 30 on: along the spine they cost
    more than 600, so the stream's certificate fails some 300 rows into them, below the last park row -- the 68-copy allele's slot
    is never complete and it goes to the exact body with the spine member, two tail failures.  The two short alleles were parked
    below: their tails skip the noise inside the gap their length needs anyway (-460 and -433, above U(680) = -689) and are accepted."""
    locus, p = failed_stream_locus(np.random.default_rng(32))
    st, st_plain, formed = _check(gpu_ctx, [locus], families=1)
    (f,) = formed["families"]
    assert (f["p"], f["spine"], f["slot_rows"], f["slot"][:2] + f["slot"][3:]) == (p, 2, [p, p + 27, p + 432], [0, 1, 2])
    assert (st["stem_failures"], st["tail_failures"], st["rule_failures"]) == (0, 2, 0), st
    assert (st_plain["stem_failures"], st_plain["tail_failures"], st_plain["rule_failures"]) == (0, 2, 0), st_plain


def test_the_acceptance_rule_fails_for_a_spine_family(gpu_ctx):
    """p = 106 and a read with 15 substitutions: every member's score stays far above -600 but not above U(106) = -114.9; the clean
    read's members are accepted."""
    st, st_plain, formed = _check(gpu_ctx, [spine_rule_failure_locus(np.random.default_rng(33))], families=1)
    assert [(f["p"], f["spine"], f["count"]) for f in formed["families"]] == [(106, 2, 4)] * 2
    assert (st["stem_failures"], st["tail_failures"], st["rule_failures"]) == (0, 0, 4), st
    assert (st_plain["stem_failures"], st_plain["tail_failures"], st_plain["rule_failures"]) == (0, 0, 4), st_plain


def test_an_asymmetric_model_forms_none(gpu_ctx):
    rng = np.random.default_rng(34)
    unit = _seq(rng, 9)
    wins = _tr(_seq(rng, 150), unit, (20, 23, 27, 25), _other(unit[0]) + _seq(rng, 300))
    prm = _abi.make_params((-1.0, -0.458675, -1.0, -0.6, -0.00005800168, -10.448214728, -10.448214728))      # b != d
    st, st_plain, formed = _check(gpu_ctx, [([_mutate(rng, wins[1][:701], 3)], [_hap(rng, w) for w in wins])], families=1, params=prm)
    assert formed["families"] == [] and st["families"] == 0 and st["with_spine"] == 0
