"""CPU: haplotype families (csrc/ltr_plan_families.cpp, form_families) on hand-built loci, through ltr_debug_plan_families -- which pairs
of a read become members, the fork row p, the acceptance bound U the host filters with.  What a family decides is HOW its members
are scored (shared rows once, ltr_dp_family.hpp), never the score: tests/test_gpu_families.py pins that to the oracle."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

RNG = np.random.default_rng(77)
FLANK = 30                                                        # window = hap[35 - F : len - (35 - F)], F = indel_flank_len = 5


def seq(n, rng=RNG):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


def hap(window):
    return seq(FLANK) + window + seq(FLANK)


def forked(prefix, tails):
    """Windows that share `prefix` exactly: tail k starts with a base of its own."""
    assert len(tails) <= 4
    return [hap(prefix + b"ACGT"[k:k + 1] + t) for k, t in enumerate(tails)]


_FILLER = None


def families(loci, **kw):
    """By rule (families = 0) a batch forms families from twelve per CU up (a full grid of wavefronts): the hand-built loci count as a
    one-CU device's and travel with a filler locus of twelve more families, which is taken out of what is returned."""
    global _FILLER
    kw.setdefault("n_cu", 1)
    if _FILLER is None:
        _FILLER = ([seq(901) for _ in range(12)], forked(seq(300), [seq(599), seq(600)]))
    main = _abi.PackedBatch(loci)
    f = _lib.debug_plan_families(_abi.PackedBatch(list(loci) + [_FILLER]), **kw)
    mine = [fam for fam in f["families"] if min(fam["out_idx"]) < main.ll_size]
    assert all(max(fam["out_idx"]) < main.ll_size for fam in mine)
    filler = len(f["families"]) - len(mine)
    assert filler in (0, 12)
    return dict(families=mine, members=f["members"] - 2 * filler, n_pairs=f["n_pairs"] - 24)


def test_fork_row_members_and_geometry():
    read = seq(701)                                               # 700 columns: strips of 11, 64 lanes
    f = families([([read, seq(702)], forked(seq(200), [seq(449), seq(499), seq(559)]))])
    assert len(f["families"]) == 2 and f["members"] == 6 and f["n_pairs"] == 6
    for fam in f["families"]:
        assert (fam["count"], fam["p"], fam["W"]) == (3, 200, 11) and sorted(fam["n"]) == [650, 700, 760]
    m = {len(r) for r in (read, seq(702))}
    assert {(fam["dd_min"], fam["dd_max"]) for fam in f["families"]} == {(650 - k, 760 - k) for k in m}
    # members of a family are one run of the sorted pair list, the two families side by side, the costlier read first
    a, b = f["families"]
    assert b["first"] == a["first"] + a["count"] and sorted(a["out_idx"] + b["out_idx"]) == list(range(6))
    assert sorted(a["out_idx"]) in ([0, 1, 2], [3, 4, 5])


def test_a_haplotype_that_is_a_prefix_of_another_leaves_a_tail_of_one_row():
    x = seq(650)
    f = families([([seq(701)], [hap(x), hap(x + seq(50))])])
    assert [(fam["count"], fam["p"]) for fam in f["families"]] == [(2, 649)]          # common prefix 650, but p <= n_min - 1


def test_a_fork_beyond_the_read():
    """p is bounded by the windows, not by the read: 1280 columns against windows of 1500 and 1550 rows that share 1400 (the bound's
    table reaches that far: lpc[p - 1] with p up to m + 599)."""
    f = families([([seq(1281)], forked(seq(1400), [seq(99), seq(149)]))])
    (fam,) = f["families"]
    assert (fam["count"], fam["p"], fam["W"], fam["dd_min"], fam["dd_max"]) == (2, 1400, 20, 219, 269)
    f32 = lambda v: np.float64(np.float32(v))
    assert fam["U"] == ((f32(-10.448214728) + 1398 * f32(-1.0)) + f32(-0.458675)) + f32(-0.000100005)
    # the furthest a fork can be: m = 1281, n = 1881 and 1880 (n - m = 600 is risky under the default model: a gentler extension)
    prm = _abi.make_params((-0.25, -0.458675, -0.25, -0.458675, -0.00005800168, -10.448214728, -10.448214728))
    x = seq(1881)
    f = families([([seq(1281)], [hap(x), hap(x[:1880])])], params=prm)
    assert [(fam["count"], fam["p"]) for fam in f["families"]] == [(2, 1879)]


def test_the_bound_is_row_zeros_own_expression():
    f = families([([seq(701)], forked(seq(100), [seq(599), seq(649)]))])
    (fam,) = f["families"]
    assert fam["p"] == 100
    f32 = lambda v: np.float64(np.float32(v))
    # ((g + lpc[p-1]) + d) + MATCH, lpc[p-1] = (p - 2) x c: the float-typed defaults of the reference promoted to double
    want = ((f32(-10.448214728) + 98 * f32(-1.0)) + f32(-0.458675)) + f32(-0.000100005)
    assert fam["U"] == want and abs(fam["U"] - (-108.9069897)) < 1e-5


@pytest.mark.parametrize("what", ["short haplotype", "far haplotype", "N in the read", "masked haplotype", "640 columns", "1281 columns",
                                  "risky length difference", "no chance against the bound", "asymmetric model", "explicit mode"])
def test_exclusions(what):
    prefix, read, kw = seq(200), seq(701), {}
    haps = forked(prefix, [seq(449), seq(499), seq(559)])
    want = [(3, 200)]
    if what == "short haplotype":
        haps.append(seq(50)); want = [(3, 200)]                                       # hap_full_len <= 60: constant score
    elif what == "far haplotype":
        haps = forked(prefix, [seq(449), seq(499), seq(1200)]); want = [(2, 200)]     # |n - m| > 600: constant score
    elif what == "N in the read":
        read = read[:300] + b"N" + read[301:]; want = []
    elif what == "masked haplotype":
        haps[1] = haps[1][:400] + b"acgtn" + haps[1][405:]; want = [(2, 200)]         # bytes outside ACGT behind the fork
    elif what == "640 columns":
        read = seq(641); want = []                                                    # a packed class takes it
    elif what == "1281 columns":
        read = seq(1282); haps = forked(prefix, [seq(1049), seq(1099), seq(1159)]); want = []       # two column blocks
    elif what == "risky length difference":
        haps = forked(seq(600), [seq(99), seq(149), seq(620)]); want = [(2, 600)]      # n - m = 520: straight to the exact body
    elif what == "no chance against the bound":
        haps = forked(seq(100), [seq(599), seq(649), seq(720)]); want = [(2, 100)]     # n - m = 120: g + 119 c < U(p = 100) = -108.9
    elif what == "asymmetric model":
        kw["params"] = _abi.make_params((-1.0, -0.45, -1.0, -0.5, -0.0001, -10.0, -9.0)); want = []
    elif what == "explicit mode":
        kw["mode"] = 0; want = []
    f = families([([read], haps)], **kw)
    assert [(fam["count"], fam["p"]) for fam in f["families"]] == want
    assert f["members"] == sum(c for c, _ in want)


def test_minimum_rows_and_the_cost_rule():
    read = seq(705)                                               # 704 columns: 64 lanes of 11
    short = [([read], forked(seq(40), [seq(659), seq(669), seq(679)]))]
    assert families(short)["families"] == [] and [fam["p"] for fam in families(short, family_min_rows=32)["families"]] == [40]
    assert families(short, families=1)["families"] == []          # (the knob lifts the cost rule, not the minimum)
    # two members at p = 64 on 64 lanes: the stem's skew costs what it saves -- not by rule, only on request
    even = [([read], forked(seq(64), [seq(635), seq(685)]))]
    assert families(even)["families"] == [] and [fam["p"] for fam in families(even, families=1)["families"]] == [64]
    assert [fam["p"] for fam in families([([read], forked(seq(65), [seq(634), seq(684)]))])["families"]] == [65]
    assert families([([read], forked(seq(200), [seq(449), seq(499)]))], families=-1)["families"] == []
    # one haplotype in reach: nothing to share
    assert families([([read], forked(seq(200), [seq(449), seq(1300)]))])["families"] == []
    # fewer than twelve families per CU: not a launch of their own by rule
    raw = lambda n_reads, **kw: len(_lib.debug_plan_families(_abi.PackedBatch([([seq(706) for _ in range(n_reads)], forked(seq(200), [seq(449), seq(499)]))]), **kw)["families"])
    assert raw(12, n_cu=1) == 12 and raw(11, n_cu=1) == 0 and raw(11, n_cu=1, families=1) == 11
    assert raw(24, n_cu=2) == 24 and raw(23, n_cu=2) == 0


def test_the_schedule_batches_form_no_family():
    """The schedules tests/test_plan_units.py and tests/test_gpu_plan_schedule.py pin stay as they are: random windows share no rows,
    and the handful of reads whose two haplotypes do (test_gpu_plan_schedule: an insertion half way) are far fewer than twelve families per CU."""
    import test_gpu_plan_schedule as tgs
    import test_plan_units as tpu
    rng = np.random.default_rng(5)
    for batch, n_cu in ((tgs.schedule_batch(256), 256), (tpu._mixed_batch(rng), 1), (tpu._random_batch(rng), 256)):
        f = _lib.debug_plan_families(batch, n_cu=n_cu)
        assert f["families"] == [] and f["members"] == 0
    # (on request they are there: two reads of 1201 bases, two and a stranger of 801)
    assert [fam["p"] for fam in _lib.debug_plan_families(tgs.schedule_batch(256), families=1)["families"]] == [600, 600, 400, 400, 400]


def test_a_family_is_its_own_launch_ahead_of_the_plan_kernel():
    L = _lib.lib()
    nk = L.ltr_debug_num_classes()
    loci = [([seq(701) for _ in range(6)] + [seq(801) for _ in range(6)], forked(seq(200), [seq(449), seq(499), seq(559)])), ([seq(301)] * 3, [hap(seq(300)), hap(seq(310))])]
    s = _lib.debug_plan_schedule(_abi.PackedBatch(loci), np.full(nk + 3, 512, dtype=np.int32), n_cu=1)
    assert s["use_plan"] and [l["kind"] for l in s["launches"]] == ["family", "plan"]
    fam = s["launches"][0]
    assert fam["pairs"] == 36 and fam["grid"] == 3 and fam["small"] and fam["cmax"] == 800 and L.ltr_kernel_family(fam["cls"]) == 2
    assert s["launches"][1]["pairs"] == 6 and all(e["kind"] != 0 or e["W"] < 11 for e in s["entries"])      # the plan kernel never sees the members
