"""-m gpu: haplotype families of reads of 321 .. 640 columns (csrc/ltr_dp_family.hpp, the narrow bodies: strips of 6 .. 10 on one
wavefront) on small crafted batches, families on request in both bands (knob 2): scores bit-identical to the CPU oracle and to the
same plan without families, ltr_plan_family_stats equal to what the host formed, and the statistics show that the branch a case is
built for really ran.  Shapes: every strip width 6 .. 10 with its lane and slot edges, 2 and 12 members, a fork at the minimum and
at n - 1, a tail of 600 rows with n - m = 600 next to 601, a family of each band in one launch, config-3 loci."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

pytestmark = pytest.mark.gpu
FLANK = 30
GENTLE = (-0.25, -0.458675, -0.25, -0.458675, -0.00005800168, -10.448214728, -10.448214728)      # a = c = -0.25: test_gpu_families.py, test_length_differences_of_600_next_to_601


def _seq(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


def _hap(rng, window):
    return _seq(rng, FLANK) + window + _seq(rng, FLANK)


def _other(base):
    return b"C" if base == b"A"[0] else b"A"


def _mutate(rng, s, n_sub, lo=0):
    r = bytearray(s)
    for p in rng.choice(np.arange(lo, len(s)), size=n_sub, replace=False):
        r[p] = _other(r[p])[0]
    return bytes(r)


def _alleles(prefix, unit, copies, suffix):
    """TR-like windows: prefix + unit x k + suffix; they fork where the shortest allele's suffix meets the others' repeat."""
    return [prefix + unit * k + suffix for k in copies]


def _run(ctx, batch, families, min_rows=0, params=None):
    try:
        if params is not None:
            ctx.set_params(params)
        ctx.set_debug("families", families)
        ctx.set_debug("family_min_rows", min_rows)
        plan = ctx.plan(batch)
        plan.execute()
        ll, _ = plan.fetch()
        st = plan.family_stats()
        plan.close()
    finally:
        ctx.set_debug("reset", 0)
        if params is not None:
            ctx.set_params(_abi.default_params())
    return ll, st


def _check(ctx, loci, min_rows=0, params=None):
    """Families on request in both bands against none and against the oracle; returns (statistics, what the host formed)."""
    import oracle_lib as ol
    batch = _abi.PackedBatch(loci)
    ref, _, _ = ol.oracle_align_batch(batch, params or ctx.params)
    off, st_off = _run(ctx, batch, -1, params=params)
    on, st = _run(ctx, batch, 2, min_rows, params=params)
    assert st_off["families"] == 0 and st_off["members"] == 0
    assert np.array_equal(off.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(on.view(np.uint64), ref.view(np.uint64)), np.flatnonzero(on.view(np.uint64) != ref.view(np.uint64))[:8]
    formed = _lib.debug_plan_families(batch, params=params, families=2, family_min_rows=min_rows)
    assert st["families"] == len(formed["families"]) and st["members"] == formed["members"]
    return st, formed


def _clean(st):
    return st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0


# read columns, strip width, lanes, columns in the last lane
WIDTH_COLUMNS = [(321, 6, 54, 3), (384, 6, 64, 6), (385, 7, 55, 7), (448, 7, 64, 7), (449, 8, 57, 1), (512, 8, 64, 8), (513, 9, 57, 9), (576, 9, 64, 9),
                 (577, 10, 58, 7), (640, 10, 64, 10)]


@pytest.mark.parametrize("cols", [WIDTH_COLUMNS[:4], WIDTH_COLUMNS[4:7], WIDTH_COLUMNS[7:]], ids=["W6-7", "W8-9", "W9-10"])
def test_every_strip_width_accepts_its_tails(gpu_ctx, cols):
    rng = np.random.default_rng(sum(c[0] for c in cols))
    loci, want_w = [], []
    for C, W, lanes, last in cols:
        assert W == -(-C // 64) and lanes == -(-C // W) and last == C - (lanes - 1) * W
        m = C + 1
        unit = _seq(rng, 7)
        wins = _alleles(_seq(rng, 80), unit, (20, 22, 25), _seq(rng, m - 80 - 7 * 22))      # windows of m - 14, m, m + 21 rows
        reads = [_mutate(rng, wins[1], 3), _mutate(rng, wins[2][:m], 4)]
        assert all(len(r) == m for r in reads)
        loci.append((reads, [_hap(rng, w) for w in wins]))
        want_w += [W, W]
    st, formed = _check(gpu_ctx, loci)
    assert sorted(f["W"] for f in formed["families"]) == sorted(want_w) and all(f["count"] == 3 and f["p"] >= 80 + 7 * 20 for f in formed["families"])
    assert (st["families"], st["members"]) == (2 * len(cols), 6 * len(cols))
    assert _clean(st), st                                         # every tail accepted: nothing went to the exact body


def test_two_and_twelve_members(gpu_ctx):
    rng = np.random.default_rng(22)
    unit = _seq(rng, 6)
    prefix, suffix = _seq(rng, 60), _seq(rng, 120)
    twelve = _alleles(prefix, unit, range(30, 42), suffix)        # windows of 360 .. 426 rows, fork after 30 copies
    two = _alleles(prefix, unit, (34, 36), suffix)
    reads12 = [_mutate(rng, twelve[5], 3), _mutate(rng, twelve[9], 3)]
    reads2 = [_mutate(rng, two[0], 2), _mutate(rng, two[1], 2), _mutate(rng, two[1], 5)]
    st, formed = _check(gpu_ctx, [(reads12, [_hap(rng, w) for w in twelve]), (reads2, [_hap(rng, w) for w in two])])
    assert sorted(f["count"] for f in formed["families"]) == [2, 2, 2, 12, 12] and all(6 <= f["W"] <= 7 for f in formed["families"])
    assert _clean(st), st


def test_fork_at_the_minimum_and_one_row_tails(gpu_ctx):
    rng = np.random.default_rng(23)
    x = _seq(rng, 400)
    # p = family_min_rows: the windows fork after 64 rows and stay related (the second is the first with a few substitutions)
    a = x
    b = x[:64] + _other(x[64]) + _mutate(rng, x[65:], 4)
    # p = n_min - 1: one window is a prefix of the other -- the shorter member's tail is ONE row
    c, d = x[:390], x[:390] + _seq(rng, 25)
    loci = [([_mutate(rng, a, 2), _mutate(rng, b, 2, lo=70)], [_hap(rng, a), _hap(rng, b)]), ([_mutate(rng, c, 2), _mutate(rng, d, 3)], [_hap(rng, c), _hap(rng, d)])]
    st, formed = _check(gpu_ctx, loci, min_rows=64)
    assert sorted(f["p"] for f in formed["families"]) == [64, 64, 389, 389] and all(6 <= f["W"] <= 7 for f in formed["families"])
    assert _clean(st), st


def test_a_tail_of_600_rows_and_length_differences_of_600_next_to_601(gpu_ctx):
    """Under the gentler gap extension (a = c = -0.25: risky from 2038).  Longer windows: 640 columns against windows of 1240 rows
    (n - m = +600: a member, its tail the 600 rows behind the fork at row 640), 1241 rows (+601: the reference's constant -700, no
    member) and 1100 rows.  A gap of 600 scores about -160.7, above U(641) = -170.7: accepted from the tail.
    Shorter windows: n - m = -600 leaves a window of at most 41 rows, and the gap alone, g + 599 c = -160.2, is below every bound
    a fork at p <= 40 can have (U >= -20.4): the host's filter keeps such a pair out of any narrow family -- it and its neighbour
    at -601 are scored as before, bit for bit."""
    prm = _abi.make_params(GENTLE)
    rng = np.random.default_rng(25)
    x = _seq(rng, 1300)
    longer = ([x[:641]], [_hap(rng, x[:1241]), _hap(rng, x[:1242]), _hap(rng, x[:641] + _other(x[641]) + x[642:1100])])
    shorter = ([x[:641]], [_hap(rng, x[:41]), _hap(rng, x[:40]), _hap(rng, x[:30] + _other(x[30]) + x[31:60])])
    st, formed = _check(gpu_ctx, [longer, shorter], min_rows=16, params=prm)
    assert [(f["W"], f["p"], f["dd_min"], f["dd_max"], sorted(f["n"])) for f in formed["families"]] == [(10, 641, 459, 600, [1100, 1241])]
    assert max(formed["families"][0]["n"]) - formed["families"][0]["p"] == 600
    assert st["members"] == 2 and _clean(st), st


def test_the_acceptance_rule_fails_on_the_device(gpu_ctx):
    """A read with p / 9 + 4 substitutions at p = 100: its score stays far above -600 but not above U(100) = -108.9 -- the host cannot
    know, the device's rule sends the member to the exact body."""
    rng = np.random.default_rng(26)
    x = _seq(rng, 400)
    b = x[:100] + _other(x[100]) + x[101:]
    reads = [_mutate(rng, x, 100 // 9 + 4), _mutate(rng, x, 2)]
    st, formed = _check(gpu_ctx, [(reads, [_hap(rng, x), _hap(rng, b)])])
    assert [(f["p"], f["W"]) for f in formed["families"]] == [(100, 7), (100, 7)]
    assert st["rule_failures"] == 2 and st["stem_failures"] == 0 and st["tail_failures"] == 0, st


def test_a_random_read_fails_the_stem_certificate(gpu_ctx):
    rng = np.random.default_rng(27)
    x = _seq(rng, 640)
    b = x[:500] + _other(x[500]) + x[501:]
    st, formed = _check(gpu_ctx, [([_seq(rng, 641), _mutate(rng, x + b"A", 2)], [_hap(rng, x), _hap(rng, b)])])
    assert [(f["p"], f["W"]) for f in formed["families"]] == [(500, 10), (500, 10)]
    assert st["stem_failures"] == 1 and st["tail_failures"] == 0 and st["rule_failures"] == 0, st


def test_random_tails_fail_the_tail_certificate_under_a_clean_stem(gpu_ctx):
    rng = np.random.default_rng(28)
    x = _seq(rng, 640)
    wins = [x, x[:150] + _other(x[150]) + _seq(rng, 489), x[:150] + (b"G" if x[150] not in b"G" else b"T") + _seq(rng, 500)]
    st, formed = _check(gpu_ctx, [([_mutate(rng, x + b"A", 2)], [_hap(rng, w) for w in wins])])
    assert [(f["count"], f["p"], f["W"]) for f in formed["families"]] == [(3, 150, 10)]
    assert st["stem_failures"] == 0 and st["tail_failures"] == 2 and st["rule_failures"] == 0, st


def test_a_family_of_each_band_in_one_launch(gpu_ctx):
    rng = np.random.default_rng(29)
    loci = []
    for m in (701, 501):
        unit = _seq(rng, 7)
        wins = _alleles(_seq(rng, 80), unit, (20, 22, 25), _seq(rng, m - 80 - 7 * 22))
        loci.append(([_mutate(rng, wins[1], 3), _mutate(rng, wins[0] + _seq(rng, m - len(wins[0])), 3)], [_hap(rng, w) for w in wins]))
    st, formed = _check(gpu_ctx, loci)
    assert sorted(f["W"] for f in formed["families"]) == [8, 8, 11, 11] and st["members"] == 12
    assert _clean(st), st


def test_config3_loci_on_request_and_by_rule(gpu_ctx):
    """The first 24 loci of BASELINE config 3 with a repeat of 250 .. 500 bases: none, by rule and on request bit for bit, a stratified
    sample against the oracle, and at most 5 % of the members sent to the exact body.  (By rule a plan this small keeps the plan
    kernel -- fewer than twelve families per CU --; on request is the pass the 5 % is asserted on.)"""
    import parity_util
    from longtr_amd import synth
    hdr = synth.config_headers("config3", n_loci=400)
    ids = [i for i in range(len(hdr)) if 250 <= hdr[i, 0] <= 500][:24]
    assert len(ids) == 24
    loci, _ = synth.config_loci("config3", n_loci=400, ids=ids)
    batch, _ = synth.pack_loci(loci)
    formed = _lib.debug_plan_families(batch, families=2)
    narrow = [f for f in formed["families"] if f["W"] <= 10]
    assert len(narrow) > 256 and sum(f["count"] for f in narrow) > 2 * len(narrow)      # (the selection does form narrow families)
    off, _ = _run(gpu_ctx, batch, -1)
    by_rule, st0 = _run(gpu_ctx, batch, 0)
    on, st = _run(gpu_ctx, batch, 2)
    assert np.array_equal(by_rule.view(np.uint64), off.view(np.uint64)) and np.array_equal(on.view(np.uint64), off.view(np.uint64))
    assert st["families"] == len(formed["families"]) and st["members"] == formed["members"]
    chk = parity_util.stratified_oracle_check(batch, on, gpu_ctx.params, n_loci_target=6, reads_per_locus=2)
    assert chk["mismatches"] == 0 and chk["checked_pairs"] > 0
    # (a failed stem sends every member of its family: counted at the largest family of the batch)
    biggest = max(f["count"] for f in formed["families"])
    for s in (st0, st):
        failed = s["rule_failures"] + s["tail_failures"] + biggest * s["stem_failures"]
        print("config3 narrow families:", s)
        assert failed <= 0.05 * s["members"], s
