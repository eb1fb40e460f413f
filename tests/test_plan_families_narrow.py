"""CPU: haplotype families of reads of 321 .. 640 columns (csrc/ltr_plan_families.cpp, form_families: the narrow band, strips of 6 .. 10 on one
wavefront) on hand-built loci, through ltr_debug_plan_families.  By rule only pairs a 32-lane packed class holds become members, and
a family is formed when its modelled work, steps x (W + 1.5), is less than its members' packed work, and when the batch holds twelve
narrow families per CU; knob 2 forms them on request,
knob 1 keeps to the wide band.  tests/test_gpu_families_narrow.py pins the scores."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

RNG = np.random.default_rng(78)
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
N_FILLER = 16


def families(loci, **kw):
    """By rule a batch forms families from twelve per CU up and narrow ones only from pairs that are packed (a one-CU device packs from
    32 pairs up): the hand-built loci travel with a filler locus of sixteen narrow families (32 pairs), which is taken out again."""
    global _FILLER
    kw.setdefault("n_cu", 1)
    if _FILLER is None:
        _FILLER = ([seq(501) for _ in range(N_FILLER)], forked(seq(300), [seq(199), seq(200)]))
    main = _abi.PackedBatch(loci)
    f = _lib.debug_plan_families(_abi.PackedBatch(list(loci) + [_FILLER]), **kw)
    mine = [fam for fam in f["families"] if min(fam["out_idx"]) < main.ll_size]
    assert all(max(fam["out_idx"]) < main.ll_size for fam in mine)
    filler = len(f["families"]) - len(mine)
    assert filler in (0, N_FILLER)
    return dict(families=mine, members=f["members"] - 2 * filler, n_pairs=f["n_pairs"] - 2 * N_FILLER, filler=filler)


def f32(v):
    return np.float64(np.float32(v))


def bound(p):
    """((g + lpc[p-1]) + d) + MATCH, lpc[p-1] = (p - 2) x c: the float-typed defaults of the reference promoted to double."""
    return ((f32(-10.448214728) + (p - 2) * f32(-1.0)) + f32(-0.458675)) + f32(-0.000100005)


@pytest.mark.parametrize("C, W", [(320, None), (321, 6), (384, 6), (385, 7), (640, 10), (641, 11)])
def test_band_edges_on_request(C, W):
    m = C + 1
    tails = [seq(C - 251), seq(C - 201), seq(C - 141)]            # windows of C - 50, C, C + 60 rows that share 200
    reads = [seq(m), seq(m)]
    f = _lib.debug_plan_families(_abi.PackedBatch([(reads, forked(seq(200), tails))]), n_cu=1, families=2)
    if W is None:
        assert f["families"] == [] and f["members"] == 0
        return
    assert len(f["families"]) == 2 and f["members"] == 6 and f["n_pairs"] == 6
    for fam in f["families"]:
        assert (fam["count"], fam["p"], fam["W"]) == (3, 200, W) and sorted(fam["n"]) == [C - 50, C, C + 60]
        assert (fam["dd_min"], fam["dd_max"]) == (C - 50 - m, C + 60 - m)
        assert fam["U"] == bound(200)
    # members of a family are one run of the sorted pair list, the two families side by side
    a, b = f["families"]
    assert b["first"] == a["first"] + a["count"] and sorted(a["out_idx"] + b["out_idx"]) == list(range(6))
    assert sorted(a["out_idx"]) in ([0, 1, 2], [3, 4, 5])


def test_by_rule_only_what_a_packed_class_holds():
    locus = lambda n_reads: [([seq(501) for _ in range(n_reads)], forked(seq(300), [seq(199), seq(200)]))]
    raw = lambda n_reads, **kw: _lib.debug_plan_families(_abi.PackedBatch(locus(n_reads)), **kw)["families"]
    # one CU: 16 reads x 2 haplotypes = 32 pairs are packed on 32 lanes, and sixteen families are a grid's worth
    got = raw(16, n_cu=1)
    assert len(got) == 16 and all((fam["count"], fam["p"], fam["W"]) == (2, 300, 8) for fam in got)
    # 15 reads: 30 pairs stay one pair per wavefront -- nothing by rule, although fifteen families are enough for a launch
    assert raw(15, n_cu=1) == [] and len(raw(15, n_cu=1, families=2)) == 15
    # two CUs pack from 64 pairs up: 24 reads are families enough (24) and pairs too few (48)
    assert raw(24, n_cu=2) == [] and len(raw(32, n_cu=2)) == 32 and len(raw(24, n_cu=2, families=2)) == 24
    # packed, but fewer than twelve families per CU: eleven narrow families beside 10 pairs that share nothing
    few = locus(11) + [([seq(201) for _ in range(5)], [hap(seq(200)), hap(seq(210))])]
    assert _lib.debug_plan_families(_abi.PackedBatch(few), n_cu=1)["families"] == []
    assert len(_lib.debug_plan_families(_abi.PackedBatch(few), n_cu=1, families=2)["families"]) == 11
    # knob 1: the wide band only, on any batch; knob -1: never
    for n_reads in (15, 16):
        assert raw(n_reads, n_cu=1, families=1) == [] and raw(n_reads, n_cu=1, families=-1) == []
    # the narrow band needs twelve per CU of its own: six wide families and six narrow ones are twelve, but the narrow six are
    # not formed, and the wide six alone are then too few; eleven narrow beside twelve wide leave the wide twelve as they were
    wide = lambda k: ([seq(701) for _ in range(k)], forked(seq(300), [seq(399), seq(400)]))
    narrow = lambda k: ([seq(501) for _ in range(k)], forked(seq(300), [seq(199), seq(200)]))
    rest = ([seq(201) for _ in range(4)], [hap(seq(200)), hap(seq(210))])
    widths = lambda loci, **kw: sorted(fam["W"] for fam in _lib.debug_plan_families(_abi.PackedBatch(loci), n_cu=1, **kw)["families"])
    assert widths([wide(6), narrow(6), rest]) == [] and widths([wide(6), narrow(6), rest], families=2) == [8] * 6 + [11] * 6
    assert widths([wide(12), narrow(11), rest]) == [11] * 12
    assert widths([wide(12), narrow(12), rest]) == [8] * 12 + [11] * 12
    assert widths([wide(3), narrow(12), rest]) == [8] * 12 + [11] * 3
    assert widths([wide(12), narrow(12), rest], families=1) == [11] * 12


def test_the_cost_rule_compares_modelled_work():
    """C = 640: the family runs strips of 10 on 64 lanes, a packed member strips of 20 on 32.  Two windows of 640 rows:
    family (p - 1 + 63) + 2 (640 - p + 63) = 1468 - p steps x 11.5; members 2 x (639 + 31) steps x 21.5 x 32/64 = 14 405.
    p = 64: 16 146 -- not by rule; p = 300: 13 432 -- by rule."""
    read = seq(641)
    assert (1468 - 64) * 11.5 > 2 * 670 * 21.5 * 0.5 > (1468 - 300) * 11.5
    even = [([read], forked(seq(64), [seq(575), seq(575)]))]
    f = families(even)
    assert f["filler"] == N_FILLER and f["families"] == []
    assert [(fam["count"], fam["p"], fam["W"], fam["n"]) for fam in families(even, families=2)["families"]] == [(2, 64, 10, [640, 640])]
    assert families(even, families=1)["families"] == []
    deep = [([read], forked(seq(300), [seq(339), seq(339)]))]
    assert [(fam["count"], fam["p"], fam["W"], fam["n"]) for fam in families(deep)["families"]] == [(2, 300, 10, [640, 640])]
    # the minimum of shared rows is the wide band's: no knob lifts it
    short = [([read], forked(seq(40), [seq(599), seq(599)]))]
    assert families(short, families=2)["families"] == [] and [fam["p"] for fam in families(short, families=2, family_min_rows=32)["families"]] == [40]


@pytest.mark.parametrize("knob", [0, 2])
@pytest.mark.parametrize("what", ["none", "short haplotype", "far haplotype", "N in the read", "masked haplotype", "risky length difference",
                                  "no chance against the bound", "asymmetric model", "explicit mode"])
def test_exclusions(what, knob):
    prefix, read, kw = seq(200), seq(501), {}
    haps = forked(prefix, [seq(249), seq(299), seq(359)])
    want = [(3, 200)]
    if what == "short haplotype":
        haps.append(seq(50))                                                          # hap_full_len <= 60: constant score
    elif what == "far haplotype":
        haps = forked(prefix, [seq(249), seq(299), seq(359), seq(1000)])              # |n - m| > 600: constant score
    elif what == "N in the read":
        read = read[:300] + b"N" + read[301:]; want = []
    elif what == "masked haplotype":
        haps = forked(prefix, [seq(249), seq(299), seq(359), seq(309)])
        haps[1] = haps[1][:400] + b"acgtn" + haps[1][405:]                            # bytes outside ACGT behind the fork
    elif what == "risky length difference":
        haps = forked(seq(400), [seq(99), seq(149), seq(620)]); want = [(2, 400)]      # n - m = 520: straight to the exact body
    elif what == "no chance against the bound":
        haps = forked(prefix, [seq(249), seq(299), seq(359), seq(520)])               # n - m = 220: f + 219 a = -229.4 < U(200) = -208.9
    elif what == "asymmetric model":
        kw["params"] = _abi.make_params((-1.0, -0.45, -1.0, -0.5, -0.0001, -10.0, -9.0)); want = []
    elif what == "explicit mode":
        kw["mode"] = 0; want = []
    f = families([([read], haps)], families=knob, **kw)
    assert [(fam["count"], fam["p"]) for fam in f["families"]] == want
    assert f["members"] == sum(c for c, _ in want) and all(fam["W"] == 8 for fam in f["families"])


def test_families_of_both_bands_are_one_launch_ahead_of_the_plan_kernel():
    L = _lib.lib()
    nk = L.ltr_debug_num_classes()
    loci = [([seq(701) for _ in range(6)], forked(seq(200), [seq(449), seq(499), seq(559)])),
            ([seq(501) for _ in range(12)], forked(seq(200), [seq(249), seq(299), seq(359)])),
            ([seq(201)] * 3, [hap(seq(200)), hap(seq(210))])]
    batch = _abi.PackedBatch(loci)
    formed = _lib.debug_plan_families(batch, n_cu=1)
    assert sorted(fam["W"] for fam in formed["families"]) == [8] * 12 + [11] * 6 and formed["members"] == 54
    s = _lib.debug_plan_schedule(batch, np.full(nk + 3, 512, dtype=np.int32), n_cu=1)
    assert s["use_plan"] and [l["kind"] for l in s["launches"]] == ["family", "plan"]
    fam = s["launches"][0]
    assert fam["pairs"] == 54 and fam["small"] and fam["cmax"] == 700 and L.ltr_kernel_family(fam["cls"]) == 2
    # the plan kernel never sees the members: not as one-wave pairs of their strip widths (8, 11), not as packed pairs on strips of 16
    assert s["launches"][1]["pairs"] == 6
    assert all(not (e["kind"] == 0 and e["W"] in (8, 11)) and not (e["kind"] == 1 and e["W"] == 16) for e in s["entries"])
    cf = s["class_first"]
    assert int(cf[fam["cls"] + 1] - cf[fam["cls"]]) == 54 and sum(int(cf[k + 1] - cf[k]) for k in range(nk) if k != fam["cls"]) == 6
