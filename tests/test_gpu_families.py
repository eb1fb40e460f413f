"""-m gpu: haplotype families (csrc/ltr_dp_family.hpp) -- the rows a read's haplotypes share scored once, a tail per haplotype -- on
small crafted batches: scores bit-identical to the CPU oracle and to the same plan without families, and ltr_plan_family_stats shows
that the branch a case is built for really ran (accepted tails; the acceptance rule, a stem certificate, a tail certificate sending
members to the exact body).  Shapes: every strip width 11 .. 20 with its lane and slot edges, 2 and 12 members, a fork at the
minimum and at n - 1, a tail of 600 rows, length differences of +-600."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

pytestmark = pytest.mark.gpu
FLANK = 30


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


def _alleles(rng, prefix, unit, copies, suffix):
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
    """Families on request against none and against the oracle; returns (statistics, what the host formed)."""
    import oracle_lib as ol
    batch = _abi.PackedBatch(loci)
    ref, _, _ = ol.oracle_align_batch(batch, params or ctx.params)
    off, st_off = _run(ctx, batch, -1, params=params)
    on, st = _run(ctx, batch, 1, min_rows, params=params)
    assert st_off["families"] == 0 and st_off["members"] == 0
    assert np.array_equal(off.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(on.view(np.uint64), ref.view(np.uint64)), np.flatnonzero(on.view(np.uint64) != ref.view(np.uint64))[:8]
    formed = _lib.debug_plan_families(batch, params=params, families=1, family_min_rows=min_rows)
    assert st["families"] == len(formed["families"]) and st["members"] == formed["members"]
    return st, formed


# read columns: 641 (59 lanes, 3 columns in the last), 704 (64 full lanes of 11), 705 (59 x 12, 9 in the last), one per width up to
# 1217 (61 x 20, 17 in the last) and 1280 (64 full lanes of 20)
WIDTH_COLUMNS = [(641, 11), (704, 11), (705, 12), (800, 13), (890, 14), (950, 15), (1010, 16), (1080, 17), (1150, 18), (1216, 19), (1217, 20), (1280, 20)]


@pytest.mark.parametrize("cols", [WIDTH_COLUMNS[:4], WIDTH_COLUMNS[4:8], WIDTH_COLUMNS[8:]], ids=["W11-13", "W14-17", "W18-20"])
def test_every_strip_width_accepts_its_tails(gpu_ctx, cols):
    rng = np.random.default_rng(sum(c for c, _ in cols))
    loci, want_w = [], []
    for C, W in cols:
        m = C + 1
        unit = _seq(rng, 9)
        wins = _alleles(rng, _seq(rng, 150), unit, (20, 23, 27), _seq(rng, m - 150 - 9 * 23))
        reads = [_mutate(rng, wins[1], 3), _mutate(rng, wins[2][:m] if len(wins[2]) >= m else wins[2] + _seq(rng, m - len(wins[2])), 4)]
        assert all(len(r) == m for r in reads)
        loci.append((reads, [_hap(rng, w) for w in wins]))
        want_w += [W, W]
    st, formed = _check(gpu_ctx, loci)
    assert sorted(f["W"] for f in formed["families"]) == sorted(want_w) and all(f["count"] == 3 and f["p"] >= 150 + 9 * 20 for f in formed["families"])
    assert (st["families"], st["members"]) == (2 * len(cols), 6 * len(cols))
    assert st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0       # every tail accepted: nothing went to the exact body


def two_and_twelve_loci(rng):
    """A locus of twelve alleles and one of two (test_two_and_twelve_members; tests/test_gpu_grid_cap.py)."""
    unit = _seq(rng, 6)
    prefix, suffix = _seq(rng, 120), _seq(rng, 200)
    twelve = _alleles(rng, prefix, unit, range(60, 72), suffix)                # windows of 680 .. 746 rows, fork after 60 copies
    two = _alleles(rng, prefix, unit, (64, 66), suffix)
    reads12 = [_mutate(rng, twelve[5], 3), _mutate(rng, twelve[9], 3)]
    reads2 = [_mutate(rng, two[0], 2), _mutate(rng, two[1], 2), _mutate(rng, two[1], 5)]
    return [(reads12, [_hap(rng, w) for w in twelve]), (reads2, [_hap(rng, w) for w in two])]


def test_two_and_twelve_members(gpu_ctx):
    st, formed = _check(gpu_ctx, two_and_twelve_loci(np.random.default_rng(12)))
    assert sorted(f["count"] for f in formed["families"]) == [2, 2, 2, 12, 12]
    assert st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0


def test_fork_at_the_minimum_and_one_row_tails(gpu_ctx):
    rng = np.random.default_rng(13)
    x = _seq(rng, 700)
    # p = family_min_rows: the windows fork after 64 rows and stay related (the second is the first with a few substitutions)
    a = x
    b = x[:64] + _other(x[64]) + _mutate(rng, x[65:], 4)
    # p = n_min - 1: one window is a prefix of the other -- the shorter member's tail is ONE row
    c, d = x[:690], x[:690] + _seq(rng, 25)
    loci = [([_mutate(rng, a, 2), _mutate(rng, b, 2, lo=70)], [_hap(rng, a), _hap(rng, b)]), ([_mutate(rng, c, 2), _mutate(rng, d, 3)], [_hap(rng, c), _hap(rng, d)])]
    st, formed = _check(gpu_ctx, loci, min_rows=64)
    assert sorted(f["p"] for f in formed["families"]) == [64, 64, 689, 689]
    assert st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0


def test_a_tail_of_600_rows(gpu_ctx):
    rng = np.random.default_rng(14)
    x = _seq(rng, 700)
    a = x
    b = x[:100] + _other(x[100]) + _mutate(rng, x[101:], 2)                      # forks at row 100
    reads = [_mutate(rng, a, 3), _mutate(rng, b, 3, lo=110), _mutate(rng, a, 1)]
    st, formed = _check(gpu_ctx, [(reads, [_hap(rng, a), _hap(rng, b)])])
    assert [f["p"] for f in formed["families"]] == [100] * 3 and all(max(f["n"]) - f["p"] == 600 for f in formed["families"])
    assert st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0


def test_length_differences_of_600_next_to_601(gpu_ctx):
    """|n - m| = 600 is still scored, 601 is the reference's constant -700.  Under the default model such a pair is on a risky list (it
    starts with the exact body); a gentler gap extension (a = c = -0.25: risky from 2038) makes it a member."""
    prm = _abi.make_params((-0.25, -0.458675, -0.25, -0.458675, -0.00005800168, -10.448214728, -10.448214728))
    rng = np.random.default_rng(15)
    x = _seq(rng, 1300)
    longer = ([x[:642]], [_hap(rng, x[:1242]), _hap(rng, x[:1243]), _hap(rng, x[:1100] + _seq(rng, 20))])         # n - m = +600, +601 (no member), +478
    shorter = ([x[:1281]], [_hap(rng, x[:681]), _hap(rng, x[:680]), _hap(rng, x[:675] + _other(x[675]) + x[676:705])])     # n - m = -600, -601 (no member), -576 (forks at row 675, one substitution: above U(675) = -179.2)
    st, formed = _check(gpu_ctx, [longer, shorter], params=prm)
    assert sorted((f["dd_min"], f["dd_max"]) for f in formed["families"]) == [(-600, -576), (478, 600)]
    # all four accepted from their tails (gaps of 600 at -0.25 a base: scores near -160, far above both bounds and the -600 line)
    assert st["members"] == 4 and st["stem_failures"] == 0 and st["tail_failures"] == 0 and st["rule_failures"] == 0, st


def rule_failure_locus(rng):
    """Read 0 fails the acceptance rule for both members, read 1 is clean (test_the_acceptance_rule_fails_on_the_device)."""
    x = _seq(rng, 700)
    b = x[:100] + _other(x[100]) + x[101:]
    reads = [_mutate(rng, x, 100 // 9 + 4), _mutate(rng, x, 2)]
    return reads, [_hap(rng, x), _hap(rng, b)]


def stem_failure_locus(rng):
    """Read 0 is random: its family's stem certificate fails; read 1 is clean (test_a_random_read_fails_the_stem_certificate)."""
    x = _seq(rng, 700)
    b = x[:300] + _other(x[300]) + x[301:]
    return [_seq(rng, 701), _mutate(rng, x, 2)], [_hap(rng, x), _hap(rng, b)]


def tail_failure_locus(rng):
    """One read, a clean stem of 300 rows and two random tails (test_random_tails_fail_the_tail_certificate_under_a_clean_stem)."""
    x = _seq(rng, 700)
    wins = [x, x[:300] + _other(x[300]) + _seq(rng, 399), x[:300] + (b"G" if x[300] not in b"G" else b"T") + _seq(rng, 420)]
    return [_mutate(rng, x, 2)], [_hap(rng, w) for w in wins]


def test_the_acceptance_rule_fails_on_the_device(gpu_ctx):
    """A read with p / 9 + 4 substitutions at p = 100: its score stays far above -600 but not above U(100) = -108.9 -- the host cannot
    know, the device's rule sends the member to the exact body."""
    st, formed = _check(gpu_ctx, [rule_failure_locus(np.random.default_rng(16))])
    assert [f["p"] for f in formed["families"]] == [100, 100]
    assert st["rule_failures"] == 2 and st["stem_failures"] == 0 and st["tail_failures"] == 0      # both members of the noisy read; the clean read's are accepted


def test_a_random_read_fails_the_stem_certificate(gpu_ctx):
    st, formed = _check(gpu_ctx, [stem_failure_locus(np.random.default_rng(17))])
    assert len(formed["families"]) == 2
    assert st["stem_failures"] == 1 and st["tail_failures"] == 0 and st["rule_failures"] == 0


def test_random_tails_fail_the_tail_certificate_under_a_clean_stem(gpu_ctx):
    st, formed = _check(gpu_ctx, [tail_failure_locus(np.random.default_rng(18))])
    assert [(f["count"], f["p"]) for f in formed["families"]] == [(3, 300)]
    assert st["stem_failures"] == 0 and st["tail_failures"] == 2 and st["rule_failures"] == 0


def test_bytes_outside_acgt_form_no_family(gpu_ctx):
    rng = np.random.default_rng(19)
    x = _seq(rng, 700)
    b = x[:300] + _other(x[300]) + x[301:]
    n_read = _mutate(rng, x, 2)
    n_read = n_read[:350] + b"N" + n_read[351:]
    masked = _hap(rng, b)
    masked = masked[:500] + masked[500:520].lower() + masked[520:]
    st, formed = _check(gpu_ctx, [([n_read], [_hap(rng, x), _hap(rng, b)]), ([_mutate(rng, x, 2)], [_hap(rng, x), masked])])
    assert formed["families"] == [] and st["families"] == 0


def test_config3_loci_by_rule(gpu_ctx):
    """The first 24 loci of BASELINE config 3 with a repeat of 600 bases or more: families by rule against none, bit for bit, a
    stratified sample against the oracle, and at most 5 % of the members sent to the exact body.  (By rule a plan this small keeps
    the plan kernel -- fewer than twelve families per CU --, so the same loci run with families on request as well: that is the
    pass the 5 % is asserted on.)"""
    import parity_util
    from longtr_amd import synth
    hdr = synth.config_headers("config3", n_loci=400)
    ids = [i for i in range(len(hdr)) if hdr[i, 0] >= 600][:24]
    assert len(ids) == 24
    loci, _ = synth.config_loci("config3", n_loci=400, ids=ids)
    batch, _ = synth.pack_loci(loci)
    off, _ = _run(gpu_ctx, batch, -1)
    by_rule, st0 = _run(gpu_ctx, batch, 0)
    on, st = _run(gpu_ctx, batch, 1)
    assert np.array_equal(by_rule.view(np.uint64), off.view(np.uint64)) and np.array_equal(on.view(np.uint64), off.view(np.uint64))
    assert st0["families"] in (0, st["families"]) and st["families"] > 256 and st["members"] > 2 * st["families"]
    chk = parity_util.stratified_oracle_check(batch, on, gpu_ctx.params, n_loci_target=6, reads_per_locus=2)
    assert chk["mismatches"] == 0 and chk["checked_pairs"] > 0
    # (a failed stem sends every member of its family: counted at the largest family of the batch)
    biggest = max(f["count"] for f in _lib.debug_plan_families(batch, families=1)["families"])
    for s in (st0, st):
        failed = s["rule_failures"] + s["tail_failures"] + biggest * s["stem_failures"]
        print("config3 families:", s)
        assert failed <= 0.05 * s["members"], s
