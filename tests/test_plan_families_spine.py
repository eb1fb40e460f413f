"""CPU: the spine of a haplotype family (csrc/ltr_plan_families.cpp, choose_spine) on hand-built loci, through
ltr_debug_plan_family_forks: which member the stream follows beyond the fork row p, where every other member leaves it, which of
those rows are parked when there are more than the park slots hold, and that forming itself (ltr_debug_plan_families) does not
depend on it.  Every expectation is formed here from the windows alone.  tests/test_gpu_families_spine.py pins the scores."""
import itertools

import numpy as np

from longtr_amd import _abi, _lib

RNG = np.random.default_rng(409)
FLANK = 30                                                        # window = hap[35 - F : len - (35 - F)], F = indel_flank_len = 5
M = 701                                                           # read bases: 700 columns, strips of 11 on 64 lanes


def seq(n, rng=RNG):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


def other(base, avoid=b""):
    return bytes([next(c for c in b"ACGT" if c != base and c not in avoid)])


def hap(window):
    return seq(FLANK) + window + seq(FLANK)


def lcp(a, b):
    k = 0
    while k < min(len(a), len(b)) and a[k] == b[k]:
        k += 1
    return k


def model(wins, p, slots):
    """The rule as the issue states it: spine, fork rows, kept rows, slot of every member, modelled steps (L = 64 lanes)."""
    H = len(wins)
    fork = lambda s, k: max(p, min(lcp(wins[s], wins[k]), len(wins[k]) - 1))
    rows = [len(wins[s]) - p + sum(len(wins[k]) - fork(s, k) for k in range(H) if k != s) for s in range(H)]
    plain = (p - 1) + 63 + sum(len(w) - p + 63 for w in wins)
    s = rows.index(min(rows))
    forks = [len(wins[k]) if k == s else fork(s, k) for k in range(H)]
    beyond = sorted({f for k, f in enumerate(forks) if k != s and f > p})
    if not beyond:
        return dict(spine=-1, steps=plain)
    saved = lambda kept: sum(max([p] + [v for v in kept if v <= forks[k]]) - p for k in range(H) if k != s)
    best = max(saved(kept) for r in range(1, slots) for kept in itertools.combinations(beyond, min(r, len(beyond))))
    return dict(spine=s, forks=forks, beyond=beyond, best_saved=best, plain=plain, steps_uncapped=(len(wins[s]) - 1) + 63 + sum(len(wins[k]) - forks[k] + 63 for k in range(H) if k != s))


def forks_of(wins, n_reads=1, **kw):
    """One locus of its own: the families of its reads (random reads: forming on request does not look at them)."""
    batch = _abi.PackedBatch([([seq(M) for _ in range(n_reads)], [hap(w) for w in wins])])
    kw.setdefault("families", 1)
    kw.setdefault("family_spine", 1)                              # (on request: by rule a plan this small keeps plain families)
    f = _lib.debug_plan_family_forks(batch, **kw)
    kw.pop("family_spine")
    g = _lib.debug_plan_families(batch, families=kw["families"])
    assert len(f["families"]) == n_reads == len(g["families"])
    for a, b in zip(f["families"], g["families"]):
        assert b["n"] == [len(w) for w in wins]                   # members in haplotype order
    return f, g


def check(wins, fam, p):
    """One family against the model; returns the model."""
    mo = model(wins, p, fam["park_slots"])
    assert fam["p"] == p and fam["spine"] == mo["spine"]
    if mo["spine"] < 0:
        assert fam["slots"] == 0 and fam["steps"] == mo["steps"] and fam["fork"] == [p] * len(wins)
        return mo
    s = mo["spine"]
    assert fam["fork"] == mo["forks"]
    assert fam["slot_rows"][0] == p and fam["slot_rows"] == sorted(set(fam["slot_rows"])) and set(fam["slot_rows"][1:]) <= set(mo["beyond"])
    assert fam["slots"] == min(len(mo["beyond"]) + 1, fam["park_slots"])
    start = [fam["slot_rows"][fam["slot"][k]] for k in range(len(wins))]
    for k in range(len(wins)):
        if k != s:                                                # the nearest kept row at or below the member's own
            assert start[k] == max(v for v in fam["slot_rows"] if v <= mo["forks"][k]), (k, start, mo["forks"])
    assert sum(start[k] - p for k in range(len(wins)) if k != s) == mo["best_saved"]
    assert fam["steps"] == (len(wins[s]) - 1) + 63 + sum(len(wins[k]) - start[k] + 63 for k in range(len(wins)) if k != s)
    assert fam["steps"] < mo["plain"]
    return mo


def tr(prefix, unit, copies, suffix):
    return [prefix + unit * k + suffix for k in copies]


def test_the_spine_minimises_the_modelled_rows():
    unit = seq(9)
    prefix, suffix = seq(150), other(unit[0]) + seq(300)
    # (the two longest alleles of a pure repeat always tie -- each shares with the other what the other shares with it -- and the
    # first of them in haplotype order is taken: here neither the first nor the last haplotype)
    wins = tr(prefix, unit, (20, 23, 27, 25), suffix)
    f, _ = forks_of(wins, n_reads=2)
    p = 150 + 9 * 20
    for fam in f["families"]:
        mo = check(wins, fam, p)
        assert mo["spine"] == 2 and fam["fork"] == [p, p + 27, len(wins[2]), p + 45] and fam["slot"] == [0, 1, 0, 2]
        assert fam["slot_rows"] == [p, p + 27, p + 45]
        assert (fam["dd_min"], fam["dd_max"]) == (len(wins[0]) - M, len(wins[2]) - M)
    assert f["with_spine"] == 2 and f["steps_saved"] == 2 * (27 + 45 + 63)      # the units the 23- and 25-copy alleles share with the spine, one fill/drain


def test_two_members_with_the_same_fork_row():
    unit = seq(9)
    prefix = seq(150)
    suf_a = other(unit[0]) + seq(250)
    suf_b = other(unit[0], avoid=suf_a[:1]) + seq(240)
    wins = [prefix + unit * 20 + suf_a, prefix + unit * 27 + suf_a, prefix + unit * 23 + suf_a, prefix + unit * 23 + suf_b]
    f, _ = forks_of(wins)
    (fam,) = f["families"]
    mo = check(wins, fam, 150 + 9 * 20)
    assert mo["spine"] == 1 and fam["fork"][2] == fam["fork"][3] == 150 + 9 * 23 and fam["slots"] == 2 and fam["slot"][2] == fam["slot"][3] == 1


def test_a_member_forks_where_it_leaves_the_spine_not_where_it_leaves_its_nearest_relative():
    unit = seq(9)
    prefix, suffix = seq(100), other(unit[0]) + seq(220)
    long_ = prefix + unit * 30 + suffix
    q = 100 + 9 * 22 + 4                                           # a substitution inside the repeat
    z1 = long_[:q] + other(long_[q]) + long_[q + 1:]
    z2 = z1[:q + 20] + other(z1[q + 20]) + z1[q + 21:]
    wins = [prefix + unit * 20 + suffix, long_, prefix + unit * 29 + suffix, prefix + unit * 28 + suffix, z1, z2]
    f, _ = forks_of(wins)
    (fam,) = f["families"]
    mo = check(wins, fam, 100 + 9 * 20)
    assert mo["spine"] == 1 and lcp(z1, z2) == q + 20 > lcp(z1, long_) == q
    assert fam["fork"][4] == fam["fork"][5] == q


def test_a_window_that_is_a_prefix_of_the_spine_has_a_one_row_tail():
    y = seq(720)
    a = y[:600] + other(y[600]) + seq(80)
    d = y[:710] + other(y[710]) + seq(20)
    wins = [a, y, y[:690], d]
    f, _ = forks_of(wins)
    (fam,) = f["families"]
    mo = check(wins, fam, 600)
    assert mo["spine"] == 1 and fam["fork"][2] == 689 and len(wins[2]) - fam["fork"][2] == 1
    # ... and the other way round: the SPINE is a prefix of a member, which leaves it at the spine's end (row n_s)
    wins = [a, y, y[:690]]
    (fam,) = forks_of(wins)[0]["families"]
    mo = check(wins, fam, 600)
    assert mo["spine"] == 2 and fam["fork"][1] == 690 == len(wins[2]) and fam["slot_rows"] == [600, 690]


def test_more_fork_rows_than_park_slots():
    unit = seq(6)
    prefix, suffix = seq(120), other(unit[0]) + seq(199)
    wins = tr(prefix, unit, range(60, 72), suffix)               # 12 alleles: the shortest fixes p, the others leave the spine at ten more rows
    f, _ = forks_of(wins)
    (fam,) = f["families"]
    p = 120 + 6 * 60
    mo = check(wins, fam, p)
    others = [k for k in range(12) if k != mo["spine"]]
    assert mo["spine"] == 10 and len({fam["fork"][k] for k in others}) == 11 and len(mo["beyond"]) == 10      # (70 and 71 copies tie: the first)
    assert fam["slots"] == fam["park_slots"] < 11
    lost = [k for k in others if fam["fork"][k] > p and fam["fork"][k] not in fam["slot_rows"]]
    assert len(lost) == 10 - (fam["slots"] - 1)
    for k in lost:                                                 # the nearest kept row below: some rows run again
        assert p <= fam["slot_rows"][fam["slot"][k]] < fam["fork"][k]
    assert mo["steps_uncapped"] < fam["steps"] < mo["plain"]


def test_nothing_beyond_p_is_a_plain_family():
    x = seq(300)
    wins = [x + b"ACGT"[k:k + 1] + seq(380 + 10 * k) for k in range(3)]
    f, _ = forks_of(wins)
    (fam,) = f["families"]
    mo = check(wins, fam, 300)
    assert mo["spine"] == -1 and f["with_spine"] == 0 and f["steps_saved"] == 0


def test_the_knob_forms_no_spine_and_forming_does_not_depend_on_it():
    unit = seq(9)
    suffix = other(unit[0]) + seq(300)
    x = seq(300)
    loci = [([seq(M), seq(M)], [hap(w) for w in tr(seq(150), unit, (20, 23, 27, 25), suffix)]),
            ([seq(M)], [hap(x + b"ACGT"[k:k + 1] + seq(380 + 10 * k)) for k in range(3)]),
            ([seq(901), seq(M)], [hap(w) for w in tr(seq(200), seq(6), range(60, 72), other(unit[0]) + seq(199))])]
    batch = _abi.PackedBatch(loci)
    on = _lib.debug_plan_family_forks(batch, families=1, family_spine=1)
    off = _lib.debug_plan_family_forks(batch, families=1, family_spine=-1)
    listed = _lib.debug_plan_families(batch, families=1)          # (the library's default: by rule -- seven families are far too few)
    by_rule = _lib.debug_plan_family_forks(batch, families=1, family_spine=0, n_cu=1)
    assert by_rule["with_spine"] == 0 and _lib.debug_plan_family_forks(batch, families=1, family_spine=0)["with_spine"] == 0
    assert on["with_spine"] == 4 and off["with_spine"] == 0 and off["steps_saved"] == 0 and on["steps_saved"] > 0
    assert all(f["spine"] == -1 and f["slots"] == 0 and f["fork"] == [f["p"]] * f["count"] for f in off["families"])
    cols = ("first", "count", "p", "W", "dd_min", "dd_max", "out_idx")
    assert [[f[c] for c in cols] for f in off["families"]] == [[f[c] for c in cols] for f in listed["families"]]
    # the same families with the same members, fork rows and ranges, whatever the knob; a family's place in the launch order
    # follows its modelled steps, which the spine lowers
    key = lambda f: min(f["out_idx"])
    assert [[f[c] for c in cols[1:]] for f in sorted(on["families"], key=key)] == [[f[c] for c in cols[1:]] for f in sorted(off["families"], key=key)]
    plain = {key(f): f["steps"] for f in off["families"]}
    assert all(f["steps"] < plain[key(f)] if f["spine"] >= 0 else f["steps"] == plain[key(f)] for f in on["families"])


def test_the_pinned_hook_lists_the_same_families_under_active_spines():
    """ltr_debug_plan_families has no spine knob: it plans by rule.  On a one-CU device 26 families are enough for the rule (24 per CU),
    so there its six columns, U, the members' windows and LL indices are listed with every family run along a spine -- and equal, entry
    for entry, what the same device lists with the knob at -1."""
    unit = seq(9)
    wins = tr(seq(150), unit, (20, 23, 27, 25), other(unit[0]) + seq(300))
    batch = _abi.PackedBatch([([seq(M) for _ in range(26)], [hap(w) for w in wins])])
    active = _lib.debug_plan_family_forks(batch, families=1, family_spine=0, n_cu=1)
    assert active["with_spine"] == 26 == len(active["families"]) and all(f["spine"] == 2 for f in active["families"])
    listed = _lib.debug_plan_families(batch, families=1, n_cu=1)            # by rule: the spines are active
    off = _lib.debug_plan_family_forks(batch, families=1, family_spine=-1, n_cu=1)
    assert off["with_spine"] == 0 and len(listed["families"]) == 26
    cols = ("first", "count", "p", "W", "dd_min", "dd_max", "out_idx")
    assert [[f[c] for c in cols] for f in listed["families"]] == [[f[c] for c in cols] for f in off["families"]] == [[f[c] for c in cols] for f in active["families"]]
    p = 150 + 9 * 20
    f32 = lambda v: np.float64(np.float32(v))
    bound = ((f32(-10.448214728) + (p - 2) * f32(-1.0)) + f32(-0.458675)) + f32(-0.000100005)
    assert all(f["U"] == bound and f["n"] == [len(w) for w in wins] for f in listed["families"])
    # 23 reads are one family short of the rule: plain families
    fewer = _abi.PackedBatch([([seq(M) for _ in range(23)], [hap(w) for w in wins])])
    assert _lib.debug_plan_family_forks(fewer, families=1, family_spine=0, n_cu=1)["with_spine"] == 0
