"""CPU: the planning units of ltr_plan_create (csrc/ltr_plan_*.cpp, one header: csrc/ltr_plan.h) through their ltr_debug_* entry points -- the table of
launch classes, the rule that gives a pair its class and launch-order key, the class sort with folding.  They decide
WHICH kernel scores a pair and in what order, never the score (the GPU tests run every case in ten scheduling modes)."""
import ctypes as C

import numpy as np
import pytest

from longtr_amd import _abi, _lib

L = _lib.lib()
NK = L.ltr_debug_num_classes()
N_CU = 256


def class_info(k):
    v = [C.c_int(0) for _ in range(4)]
    assert L.ltr_debug_class_info(k, *[C.byref(x) for x in v]) == 0
    return dict(zip(("family", "W", "waves", "lanes"), (x.value for x in v)))


def classify(n, m, mode=-1, pairs=10 ** 6, long_pairs=0, hfl=None, generic=0, params=None):
    cls, key, xl = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    p = params or _abi.default_params()
    hfl = n + 60 if hfl is None else hfl
    assert L.ltr_debug_classify(C.byref(p), mode, N_CU, pairs, long_pairs, n, m, hfl, generic, C.byref(cls), C.byref(key), C.byref(xl)) == 0
    return cls.value, key.value, xl.value


def test_class_table_is_consistent_with_the_library():
    assert NK == L.ltr_num_kernels()
    fam = {0: 0, 1: 0, 2: 0, 3: 0}
    for k in range(NK):
        ci = class_info(k)
        assert ci["family"] == L.ltr_kernel_family(k) and ci["lanes"] == L.ltr_kernel_lanes_per_pair(k)
        fam[ci["family"]] += 1
        if ci["family"] == 1:
            assert ci["lanes"] in (2, 4, 8, 16, 32) and 1 <= ci["W"] <= 20
    assert fam[0] == 20 and fam[1] == 100 and fam[3] == 6


def test_every_pair_fits_its_class():
    """Whatever the rule picks, the read's columns fit the class: lanes x strip width (one block) for the packed and
    workgroup classes; one-wave classes take any length (column blocks)."""
    rng = np.random.default_rng(3)
    for mode in (-1, 0, 1, 2, 3, 5, 6, 7, 8):
        for _ in range(400):
            m = int(rng.integers(2, 12000)) if rng.random() < 0.3 else int(rng.integers(2, 700))
            n = max(2, m + int(rng.integers(-40, 40)))
            pairs = int(10 ** rng.uniform(1, 7))
            cls, key, xl = classify(n, m, mode=mode, pairs=pairs, long_pairs=int(rng.integers(0, 5000)))
            ci = class_info(cls)
            C_ = m - 1
            assert ci["family"] in (0, 1, 2) and (1 <= key <= 511 or abs(n - m) > 600)
            if ci["family"] == 1:
                assert C_ <= ci["lanes"] * ci["W"] and (ci["lanes"] * (ci["W"] - 1) < C_ or ci["W"] == 1), (m, ci)
            elif ci["family"] == 2:
                assert C_ <= ci["lanes"] * ci["W"]
            else:
                ncb = -(-C_ // 1280)
                assert ci["W"] == -(-C_ // (64 * ncb))
            assert (xl == 1) == (C_ <= 256) or xl != 1


def test_modes_and_batch_size_rules():
    # a one-locus batch keeps one pair per wavefront; a big batch packs short reads; explicit modes force the geometry
    assert class_info(classify(220, 221, pairs=224)[0])["family"] == 0
    assert class_info(classify(40, 40, pairs=3 * 10 ** 6)[0])["family"] == 1
    assert class_info(classify(40, 40, mode=0)[0])["family"] == 0
    for mode, lanes in ((1, 32), (5, 16), (6, 8), (7, 4), (8, 2)):
        ci = class_info(classify(40, 40, mode=mode)[0])
        assert ci["family"] == 1 and ci["lanes"] == lanes and ci["W"] == -(-39 // lanes)
    # a read too long for the forced segment takes the next wider one; beyond 641 bases one pair per wavefront
    assert class_info(classify(200, 200, mode=8)[0])["lanes"] == 16                  # 199 columns: 2 x 20 and 4 x 20 and 8 x 20 too few
    assert class_info(classify(700, 700, mode=1)[0])["family"] == 0
    # long reads: workgroup kernels while there are few of them, column blocks on one wavefront otherwise / in mode 3
    assert class_info(classify(5000, 5000, long_pairs=100)[0])["lanes"] == 512       # one round either way: eight waves finish a pair sooner
    ci = class_info(classify(5000, 5000, long_pairs=600)[0])                         # one round of four-wave workgroups, two of eight-wave ones
    assert ci["lanes"] == 256 and ci["W"] == 20
    assert class_info(classify(5000, 5000, long_pairs=1868)[0])["lanes"] == 256      # 2.4 rounds: two whole ones on four waves; ltr_plan_create moves the rest to eight (config5hifi)
    assert class_info(classify(5000, 5000, long_pairs=800)[0])["lanes"] == 512       # one round and a bit: two rounds of eight waves are as good
    assert class_info(classify(6000, 6000, long_pairs=100)[0])["lanes"] == 512
    # reads of up to two column blocks (2560 columns): four-wave workgroups while the batch cannot fill the GPU's wave slots; in a
    # batch that can they stay with the one-wave classes -- the plan kernel holds every wave slot, a launch beside it would starve
    assert class_info(classify(2000, 2000, pairs=2000, long_pairs=100)[0])["lanes"] == 256
    ci = class_info(classify(2000, 2000, long_pairs=100)[0])
    assert ci["family"] == 0 and ci["W"] == 16                                       # 1999 columns = two blocks of 64 x 16
    assert class_info(classify(2000, 2000, mode=1, long_pairs=100)[0])["lanes"] == 256   # (explicit modes: no plan kernel)
    assert class_info(classify(2700, 2700, long_pairs=100)[0])["lanes"] == 256
    # a length difference no certificate can hold goes straight to its exact list (automatic mode)
    cls, _, xl = classify(300, 880)
    assert class_info(cls)["family"] == 3 and cls == NK - 6 + xl
    assert class_info(classify(300, 780)[0])["family"] != 3 and class_info(classify(300, 880, mode=3)[0])["family"] == 0
    assert class_info(classify(5000, 5000, long_pairs=9216)[0])["lanes"] == 256       # wide four-wave strips: beyond the eight-wave regime too
    assert class_info(classify(5000, 5000, long_pairs=10 ** 5)[0])["family"] == 0     # ... up to 80 long pairs per CU
    assert class_info(classify(3000, 3000, long_pairs=10 ** 5)[0])["family"] == 0
    assert class_info(classify(6000, 6000, long_pairs=10 ** 5)[0])["family"] == 0
    assert class_info(classify(5000, 5000, mode=3, long_pairs=100)[0])["family"] == 0
    # shortcuts keep a one-wave class and the last place in the launch order; non-ACGT pairs start in the generic exact list
    cls, key, _ = classify(0, 50, hfl=50)
    assert class_info(cls)["family"] == 0 and key == 0
    cls, key, _ = classify(1000, 50)
    assert key == 0
    cls, _, xl = classify(100, 100, generic=1)
    assert class_info(cls)["family"] == 3 and xl == 0
    # mode 4: every pair straight to the exact kernel of its length
    for m, want in ((100, 1), (400, 2), (900, 3), (2000, 4), (6000, 5)):
        cls, _, xl = classify(m, m, mode=4)
        assert class_info(cls)["family"] == 3 and xl == want
    # an asymmetric indel model has no LUT exact kernels and no workgroup kernels; under the plan kernel (automatic mode) its failed
    # certificates still go by read length -- to the threshold bodies the plan kernel calls itself (round 6) --, without it to the
    # generic list
    asym = _abi.make_params((-1.0, -0.45, -1.0, -0.5, -0.0001, -10.0, -9.0))
    cls, _, xl = classify(5000, 5000, long_pairs=10, params=asym)
    assert class_info(cls)["family"] == 0 and xl == 5
    cls, _, xl = classify(5000, 5000, long_pairs=10, params=asym, mode=0)
    assert class_info(cls)["family"] == 0 and xl == 0


def test_order_key_is_monotone_in_the_work():
    keys = [classify(n, n, mode=0)[1] for n in (30, 60, 120, 250, 500, 1000, 2000, 4000)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def _sort(cls, key, fold):
    cls = np.ascontiguousarray(cls, dtype=np.int16); key = np.ascontiguousarray(key, dtype=np.int16)
    order = np.zeros(len(cls), dtype=np.int32); first = np.zeros(NK + 1, dtype=np.int32)
    assert L.ltr_debug_sort_by_class(cls.ctypes.data, key.ctypes.data, len(cls), int(fold), N_CU, order.ctypes.data, first.ctypes.data) == 0
    return order, first


def test_sort_by_class_is_a_stable_partition_longest_first():
    rng = np.random.default_rng(11)
    n = 300000                                                          # several 64 k blocks and 32 k segments: the parallel paths
    cls = rng.choice([3, 11, 14, 25, 47, 90, NK - 2], size=n).astype(np.int16)
    key = rng.integers(0, 512, size=n).astype(np.int16)
    order, first = _sort(cls, key, fold=False)
    assert sorted(order.tolist()) == list(range(n)) and first[0] == 0 and first[NK] == n
    for k in range(NK):
        seg = order[first[k]:first[k + 1]]
        assert (cls[seg] == k).all()
        kk = key[seg]
        assert (np.diff(kk.astype(np.int32)) <= 0).all()                # longest first
        same = np.flatnonzero(np.diff(kk.astype(np.int32)) == 0)
        assert (seg[same] < seg[same + 1]).all()                        # input order kept inside a key
    assert _sort(np.zeros(0), np.zeros(0), False)[1][NK] == 0
    bad = np.array([NK], dtype=np.int16)
    o = np.zeros(1, dtype=np.int32); f = np.zeros(NK + 1, dtype=np.int32)
    assert L.ltr_debug_sort_by_class(bad.ctypes.data, np.zeros(1, dtype=np.int16).ctypes.data, 1, 0, N_CU, o.ctypes.data, f.ctypes.data) == _abi.LTR_ERR_INVALID


def test_folding_merges_underfilled_classes_into_wider_strips_only():
    # one-wave classes W = 11 (k = 10) .. 14 with a few pairs each: folded upwards while the strip stays within 4/3
    cls = np.array([10] * 50 + [11] * 60 + [12] * 70 + [13] * 80 + [19] * 5, dtype=np.int16)
    key = np.arange(len(cls), dtype=np.int16) % 500 + 1
    order, first = _sort(cls, key, fold=True)
    sizes = {k: int(first[k + 1] - first[k]) for k in range(NK) if first[k + 1] > first[k]}
    assert sum(sizes.values()) == len(cls)
    assert sizes.get(13) == 260 and sizes.get(19) == 5 and 10 not in sizes and 11 not in sizes and 12 not in sizes
    for k, s in sizes.items():                                          # a pair never lands in a NARROWER class than its own
        assert (cls[order[first[k]:first[k + 1]]] <= k).all()
    # a class that fills the GPU stays where it is, and a lone small class keeps its strip width (nothing wider to join)
    big = np.array([10] * 200000 + [11] * 50, dtype=np.int16)
    _, first = _sort(big, np.ones(len(big), dtype=np.int16), fold=True)
    assert first[11] - first[10] == 200000 and first[12] - first[11] == 50


def test_folding_of_the_workgroup_families():
    # four-wave classes W = 17 and W = 18 with a few hundred pairs each become one launch; a class that fills several rounds
    # of workgroups stays; the eight-wave family folds the same way; never across families
    wg4 = next(k for k in range(NK) if class_info(k)["family"] == 2 and class_info(k)["lanes"] == 256 and class_info(k)["W"] == 17)
    wg8 = next(k for k in range(NK) if class_info(k)["family"] == 2 and class_info(k)["lanes"] == 512 and class_info(k)["W"] == 12)
    cls = np.array([wg4] * 1116 + [wg4 + 1] * 420 + [wg8] * 30 + [wg8 + 2] * 40, dtype=np.int16)
    _, first = _sort(cls, np.ones(len(cls), dtype=np.int16), fold=True)
    sizes = {k: int(first[k + 1] - first[k]) for k in range(NK) if first[k + 1] > first[k]}
    assert sizes == {wg4 + 1: 1536, wg8 + 2: 70}
    cls = np.array([wg4] * 5000 + [wg4 + 1] * 420, dtype=np.int16)
    _, first = _sort(cls, np.ones(len(cls), dtype=np.int16), fold=True)
    assert first[wg4 + 1] - first[wg4] == 5000 and first[wg4 + 2] - first[wg4 + 1] == 420
    last4 = max(k for k in range(NK) if class_info(k)["family"] == 2 and class_info(k)["lanes"] == 256)
    cls = np.array([last4] * 10 + [last4 + 1] * 10, dtype=np.int16)              # the widest four-wave class next to the narrowest eight-wave one
    _, first = _sort(cls, np.ones(len(cls), dtype=np.int16), fold=True)
    assert first[last4 + 1] - first[last4] == 10


# The fold walk, family by family: hand-made class counts as ((family, strip width, lanes per pair), pairs).  256 CUs, kFoldRounds 6:
# a one-wave or packed width folds below 6144 wavefronts, a workgroup class below 1536 pairs.
ONE, PK, WG4, WG8 = (lambda W: (0, W, 64)), (lambda W, lanes: (1, W, lanes)), (lambda W: (2, W, 256)), (lambda W: (2, W, 512))
FOLD_CASES = {
    # a chain of three under-filled neighbours folds twice (below and inside the widths of the multi-width launch, which fold 2 leaves alone)
    "one-wave chain": [(ONE(6), 50), (ONE(7), 60), (ONE(8), 70), (ONE(12), 50), (ONE(13), 60), (ONE(14), 70)],
    # 6 -> 7 -> 8 fold; 9 is more than 4/3 of 6: the group ends at 8, and 9 is a lone class behind it
    "one-wave ratio": [(ONE(6), 50), (ONE(7), 60), (ONE(8), 70), (ONE(9), 80)],
    "one-wave small": [(ONE(1), 10), (ONE(2), 20), (ONE(3), 30), (ONE(4), 40), (ONE(5), 50)],      # the <= 4 exception; 5 is not within 4/3 of 1
    "one-wave lone": [(ONE(10), 50)],                                                              # no target: keeps its strip width
    "one-wave full": [(ONE(6), 7000), (ONE(7), 60), (ONE(8), 70)],                                 # a class that fills the GPU stays
    # every lanes-per-pair class of a width moves together, each into its own lanes' class of the next width
    "packed chain": [(PK(6, 32), 50), (PK(6, 16), 30), (PK(7, 32), 60), (PK(8, 16), 70), (PK(14, 32), 50), (PK(15, 32), 60), (PK(16, 8), 70)],
    "packed ratio": [(PK(6, 32), 50), (PK(7, 16), 60), (PK(8, 32), 70), (PK(9, 32), 80)],
    "packed small": [(PK(1, 2), 10), (PK(2, 4), 20), (PK(3, 2), 30), (PK(4, 32), 40), (PK(5, 32), 50)],
    "packed lone": [(PK(10, 8), 50)],
    # the fill is wavefronts: 40 000 pairs at 8 lanes are 5000 wavefronts (folds), 13 000 at 32 lanes are 6500 (stays)
    "packed full": [(PK(6, 8), 40000), (PK(7, 32), 13000), (PK(8, 32), 70)],
    "four-wave chain": [(WG4(15), 100), (WG4(16), 200), (WG4(17), 300)],
    "four-wave ratio": [(WG4(6), 50), (WG4(7), 60), (WG4(8), 70), (WG4(9), 80)],                   # (no <= 4 exception: no such width)
    "four-wave lone": [(WG4(20), 50), (WG8(8), 50)],                                               # the widest four-wave class: never into the eight-wave family
    "four-wave full": [(WG4(15), 1600), (WG4(16), 200), (WG4(17), 300)],
    "eight-wave chain": [(WG8(12), 100), (WG8(13), 200), (WG8(14), 300)],
    "eight-wave ratio": [(WG8(9), 50), (WG8(10), 60), (WG8(11), 70), (WG8(12), 80), (WG8(13), 90)],
    "eight-wave lone": [(WG8(20), 50)],
    "eight-wave full": [(WG8(12), 1600), (WG8(13), 200), (WG8(14), 300)],
}
# (case, fold) -> pairs of every non-empty class after the sort: class_first is their running sum.  Recorded from the library of the
# commit BEFORE the four fold loops became one walk (tests/manual/plan_units_ab.py --fold-literals), not from the code under test.
FOLD_EXPECTED = {
    ('one-wave chain', 1): {7: 180, 13: 180},
    ('one-wave chain', 2): {7: 180, 11: 50, 12: 60, 13: 70},
    ('one-wave chain', 3): {5: 50, 6: 60, 7: 70, 11: 50, 12: 60, 13: 70},
    ('one-wave ratio', 1): {7: 180, 8: 80},
    ('one-wave ratio', 2): {7: 180, 8: 80},
    ('one-wave ratio', 3): {5: 50, 6: 60, 7: 70, 8: 80},
    ('one-wave small', 1): {3: 100, 4: 50},
    ('one-wave small', 2): {3: 100, 4: 50},
    ('one-wave small', 3): {0: 10, 1: 20, 2: 30, 3: 40, 4: 50},
    ('one-wave lone', 1): {9: 50},
    ('one-wave lone', 2): {9: 50},
    ('one-wave lone', 3): {9: 50},
    ('one-wave full', 1): {5: 7000, 7: 130},
    ('one-wave full', 2): {5: 7000, 7: 130},
    ('one-wave full', 3): {5: 7000, 6: 60, 7: 70},
    ('packed chain', 1): {75: 70, 87: 100, 107: 110, 115: 110},
    ('packed chain', 2): {75: 70, 87: 100, 107: 110, 113: 50, 114: 60},
    ('packed chain', 3): {75: 70, 85: 30, 87: 70, 105: 50, 106: 60, 113: 50, 114: 60},
    ('packed ratio', 1): {87: 60, 107: 120, 108: 80},
    ('packed ratio', 2): {87: 60, 107: 120, 108: 80},
    ('packed ratio', 3): {86: 60, 105: 50, 107: 70, 108: 80},
    ('packed small', 1): {23: 40, 43: 20, 103: 40, 104: 50},
    ('packed small', 2): {23: 40, 43: 20, 103: 40, 104: 50},
    ('packed small', 3): {20: 10, 22: 30, 41: 20, 103: 40, 104: 50},
    ('packed lone', 1): {69: 50},
    ('packed lone', 2): {69: 50},
    ('packed lone', 3): {69: 50},
    ('packed full', 1): {66: 40000, 106: 13000, 107: 70},
    ('packed full', 2): {66: 40000, 106: 13000, 107: 70},
    ('packed full', 3): {65: 40000, 106: 13000, 107: 70},
    ('four-wave chain', 1): {132: 600},
    ('four-wave chain', 2): {132: 600},
    ('four-wave chain', 3): {132: 600},
    ('four-wave ratio', 1): {123: 180, 124: 80},
    ('four-wave ratio', 2): {123: 180, 124: 80},
    ('four-wave ratio', 3): {123: 180, 124: 80},
    ('four-wave lone', 1): {135: 50, 136: 50},
    ('four-wave lone', 2): {135: 50, 136: 50},
    ('four-wave lone', 3): {135: 50, 136: 50},
    ('four-wave full', 1): {130: 1600, 132: 500},
    ('four-wave full', 2): {130: 1600, 132: 500},
    ('four-wave full', 3): {130: 1600, 132: 500},
    ('eight-wave chain', 1): {142: 600},
    ('eight-wave chain', 2): {142: 600},
    ('eight-wave chain', 3): {142: 600},
    ('eight-wave ratio', 1): {140: 260, 141: 90},
    ('eight-wave ratio', 2): {140: 260, 141: 90},
    ('eight-wave ratio', 3): {140: 260, 141: 90},
    ('eight-wave lone', 1): {148: 50},
    ('eight-wave lone', 2): {148: 50},
    ('eight-wave lone', 3): {148: 50},
    ('eight-wave full', 1): {140: 1600, 142: 500},
    ('eight-wave full', 2): {140: 1600, 142: 500},
    ('eight-wave full', 3): {140: 1600, 142: 500},
}


def fold_case_arrays(case):
    """Launch classes and launch-order keys of the pairs of one fold case."""
    cls = np.concatenate([np.full(n, _class(*c), dtype=np.int16) for c, n in case])
    return cls, (np.arange(len(cls)) % 500 + 1).astype(np.int16)


@pytest.mark.parametrize("fold", [1, 2, 3])
@pytest.mark.parametrize("family", ["one-wave", "packed", "four-wave", "eight-wave"])
def test_fold_walk_of_every_family(family, fold):
    """One walk for the four families (fold 1: a launch per class; 2: the multi-width launches leave the one-wave widths from 11 and
    the packed widths from 13 alone; 3: the plan kernel leaves both families alone): class_first against the recorded arrays, and
    every pair in a class of its own family no narrower than its own."""
    cases = [name for name in FOLD_CASES if name.startswith(family)]
    assert len(cases) >= 4
    for name in cases:
        cls, key = fold_case_arrays(FOLD_CASES[name])
        order, first = _sort(cls, key, fold)
        sizes = np.zeros(NK, dtype=np.int64)
        for k, n in FOLD_EXPECTED[(name, fold)].items():
            sizes[k] = n
        assert first.tolist() == [0] + np.cumsum(sizes).tolist(), (name, fold)
        for k in np.flatnonzero(sizes):
            src = cls[order[first[k]:first[k + 1]]]
            assert (src <= k).all() and all(class_info(int(s))["lanes"] == class_info(int(k))["lanes"] for s in set(src.tolist())), (name, fold, k)


def test_shard_costs_are_the_plans_own_model():
    """longtr_amd/shard.py balances shards on ltr_debug_pair_costs = the cost classify_pair derives the launch-order key from
    (no hand copy of the model in Python): for a grid of (window, read columns) -- packed geometries, one wavefront per pair,
    column blocks beyond 1280 columns, workgroup kernels when long pairs are few -- key == clamp(int(16 log2 cost) - 16)."""
    import math
    from longtr_amd import shard
    for pairs, long_pairs in ((1 << 21, 1 << 20), (1 << 21, 100), (3000, 0)):
        for n in (2, 25, 64, 200, 640, 900, 1300, 2600, 5000):
            for Cc in (1, 20, 63, 64, 129, 400, 641, 1280, 1281, 2000, 3585, 5200):
                if abs(n - (Cc + 1)) > 600:
                    continue
                _, key, _ = classify(n, Cc + 1, pairs=pairs, long_pairs=long_pairs)
                win, rl = np.asarray([n], dtype=np.int32), np.asarray([Cc + 1], dtype=np.int32)
                hl, out = win + 60, np.zeros(1)
                p = _abi.default_params()
                assert L.ltr_debug_pair_costs(C.byref(p), -1, N_CU, pairs, long_pairs, 1, win.ctypes.data, rl.ctypes.data, hl.ctypes.data, out.ctypes.data) == 0
                c = float(out[0])
                assert key == min(511, max(1, (int(math.log2(c) * 16.0) if c > 1.0 else 0) - 16)), (n, Cc, pairs, long_pairs, c, key)
    # the Python entry point: same numbers, vectorised; a long pair costs more than a short one, cost grows with both sides
    c = shard.pair_time_cost(np.asarray([50, 50, 500, 900]), np.asarray([49, 99, 499, 899]))
    assert (np.diff(c) > 0).all() and c[0] > 0


def test_risky_pairs_go_straight_to_the_exact_body_per_gap_direction():
    """A pair whose length difference alone costs ~520 of the 600 the reference allows (HapAligner.cpp:283, :297-306) cannot hold a
    one-cell-per-lane certificate: it starts with the exact body (class family 3).  The cost of a gap depends on its direction
    (:285-295): haplotype longer = match->ins f, ins->ins a, ins->match b; read longer = g, c, d.  Round 6: one threshold per
    direction (a model with a != c let the dearer direction's pairs through on the cheaper direction's threshold)."""
    fam = lambda n, m, **kw: class_info(classify(n, m, **kw)[0])["family"]
    # defaults: a = c = -1, open + close = 10.9: risky from |n - m| = 511
    assert fam(700, 700 - 510) != 3 and fam(700, 700 - 511) == 3
    assert fam(700 - 510, 700) != 3 and fam(700 - 511, 700) == 3
    # a != c: ins->ins -1.2 (haplotype longer: (520 - 5.3) / 1.2 + 1 = 430), del->del -0.9 (read longer: (520 - 4.5) / 0.9 + 1 = 574)
    asym = _abi.make_params((-1.2, -0.3, -0.9, -0.5, -0.0001, -5.0, -4.0))
    assert fam(700, 700 - 429, params=asym) != 3 and fam(700, 700 - 430, params=asym) == 3
    assert fam(700 - 573, 700, params=asym) != 3 and fam(700 - 574, 700, params=asym) == 3
    # not in the explicit modes (mode 0: every pair keeps its certificate class)
    assert fam(700, 100, mode=0) != 3


# ---- the host half of ltr_plan_create (ltrp::describe_batch) and the pure pieces of ltr_plan_execute, without a GPU ----

def _random_batch(rng, n_loci=40):
    loci = []
    for _ in range(n_loci):
        tr = int(rng.integers(20, 900))
        haps = [bytes(rng.choice(list(b"ACGT"), size=tr + 70 + int(rng.integers(-15, 15))).astype(np.uint8)) for _ in range(int(rng.integers(1, 6)))]
        reads = [bytes(rng.choice(list(b"ACGT"), size=max(2, tr + int(rng.integers(-30, 30)))).astype(np.uint8)) for _ in range(int(rng.integers(1, 12)))]
        if rng.random() < 0.2:
            reads[0] = reads[0][:1] + b"N" + reads[0][2:]                # a pair outside ACGT: starts out in an exact list
        if rng.random() < 0.2:
            haps.append(b"ACGT" * 10)                                    # 40 <= 60 bases: the constant-score shortcut
        if rng.random() < 0.1:
            reads.append(bytes(rng.choice(list(b"ACGT"), size=tr + 700).astype(np.uint8)))      # more than 600 longer than any window: the other shortcut
        loci.append((reads, haps))
    return _abi.PackedBatch(loci)


def test_describe_batch_rejects_invalid_batches_with_the_library_text():
    """Every LTR_ERR_INVALID exit of the host half, each with the text ltr_plan_create reports."""
    good = lambda: _abi.PackedBatch([([b"ACGT" * 30, b"ACGTT" * 20], [b"ACGT" * 40, b"AC" * 70])])

    def fails(batch, text, params=None):
        with pytest.raises(_lib.LtrError) as e:
            _lib.debug_describe_batch(batch, params=params)
        assert e.value.code == _abi.LTR_ERR_INVALID and text in str(e.value), str(e.value)

    b = good(); b.struct.n_reads = -1
    fails(b, "negative counts")
    b = good(); b.struct.read_off = None
    fails(b, "null offset array")
    b = good(); b.locus_read_off[1] = 3
    fails(b, "locus offsets out of range")
    b = good(); b.read_off[1], b.read_off[2] = b.read_off[2], b.read_off[1] - 1
    fails(b, "read offsets not ascending")
    b = good(); b.hap_off[1] = b.hap_off[2] + 1
    fails(b, "haplotype offsets not ascending")
    b = good(); b.read_off[1] = b.read_off[0]
    fails(b, "empty or oversized read")
    fails(_abi.PackedBatch([([b"ACGT" * 30], [b"A" * ((1 << 20) + 1)])]), "bad haplotype length")       # (real bytes: the ACGT scan reads them first)
    p = _abi.default_params(); p.indel_flank_len = 0
    fails(_abi.PackedBatch([([b"ACGT" * 30], [b"AC" * 35])]), "haplotype window is empty", params=p)      # 70 bases less 2 x 35 of flank: nothing left
    assert _lib.debug_describe_batch(good())["n_pairs"] == 4


def test_describe_batch_sorts_every_pair_into_its_class():
    rng = np.random.default_rng(5)
    for mode in (-1, 0, 1):
        batch = _random_batch(rng)
        d = _lib.debug_describe_batch(batch, mode=mode, n_cu=N_CU)
        first = d["class_first"]
        assert d["n_pairs"] == batch.ll_size == d["ll_size"] and first[0] == 0 and first[NK] == d["n_pairs"] and (np.diff(first) >= 0).all()
        assert sorted(d["out_idx"].tolist()) == list(range(batch.ll_size))
        prm = _abi.default_params()
        for k in range(NK):
            seg = slice(first[k], first[k + 1])
            assert (np.diff(d["key"][seg].astype(np.int32)) <= 0).all()                      # keys descend inside a class
            if k < NK - 6:
                ck = class_info(k)
                for n, m in zip(d["n"][seg], d["m"][seg]):
                    k0 = classify(int(n), int(m), mode=mode, pairs=d["n_pairs"])[0]
                    if mode != -1:
                        assert k0 == k
                    else:                                                                    # automatic mode folds an under-filled class into a wider one of its family
                        c0 = class_info(k0)
                        assert (c0["family"], c0["waves"], c0["lanes"]) == (ck["family"], ck["waves"], ck["lanes"]) and c0["W"] <= ck["W"], (k0, k)
            if k < NK - 6 and class_info(k)["family"] == 1:
                ci = class_info(k)
                assert ((d["m"][seg] - 1) <= ci["lanes"] * ci["W"]).all()                   # every pair fits the class it was sorted into
        # cells: sum of n * m over the pairs that are not shortcuts, pair by pair inside a locus, locus by locus
        # (a shortcut by the reference's own rule, HapAligner.cpp:241-252: haplotype of at most 60 bases, or lengths more than 600 apart)
        by_out = np.argsort(d["out_idx"], kind="stable")
        locus_of = np.searchsorted(batch.ll_off, d["out_idx"][by_out], side="right") - 1
        hap_len = np.diff(batch.hap_off)
        cells, longest = 0.0, 1
        for l in range(batch.n_loci):
            acc = 0.0
            H = int(batch.locus_hap_off[l + 1] - batch.locus_hap_off[l])
            for i in by_out[locus_of == l]:
                hl = int(hap_len[batch.locus_hap_off[l] + (d["out_idx"][i] - batch.ll_off[l]) % H])
                shortcut = hl <= 60 or abs(int(d["n"][i]) - int(d["m"][i])) > 600
                assert (d["key"][i] == 0) == shortcut and (shortcut or d["n"][i] == hl - 60)   # (window: the haplotype less 2 x 30 of flank)
                if not shortcut:
                    acc += float(d["n"][i]) * float(d["m"][i])
                    longest = max(longest, int(d["n"][i]), int(d["m"][i]))
            cells += acc
        assert d["cells"] == cells and d["max_len"] == longest                          # (shortcut pairs are never laid out: they do not size the tables)
        assert d["input_bytes"] == float(batch.read_off[-1] + batch.hap_off[-1] + 8 * batch.ll_size)


def test_threshold_groups_merge_neighbouring_narrow_eight_wave_classes():
    wg = [k for k in range(NK) if L.ltr_kernel_family(k) == 2 and class_info(k)["waves"] in (4, 8)]
    rng = np.random.default_rng(9)
    for _ in range(50):
        counts = np.zeros(NK, dtype=np.int64)
        for k in rng.choice(wg, size=int(rng.integers(1, 8)), replace=False):
            counts[k] = int(rng.integers(1, 500))
        counts[int(rng.integers(0, 20))] = 1000                                               # (classes of other families are left alone)
        first = np.zeros(NK + 1, dtype=np.int32); first[1:] = np.cumsum(counts)
        for merge in (True, False):
            nw, w, npairs = _lib.debug_threshold_groups(first, merge=merge)
            assert npairs.sum() == counts[wg].sum() and (nw[counts == 0] == 0).all() and (nw[[k for k in range(NK) if k not in wg]] == 0).all()
            lead = -1
            for k in wg:
                if counts[k] == 0:
                    continue
                assert nw[k] in (4, 8) and w[k] % 2 == 0
                if npairs[k] == 0:                                                            # led by another class: its pairs follow the leader's without a gap
                    assert merge and lead >= 0 and nw[k] == 8 and w[k] <= 10 and w[lead] >= w[k]
                    assert all(counts[j] == 0 or (nw[j] == 8 and w[j] <= 10) for j in range(lead, k))
                else:
                    assert npairs[k] >= counts[k]
                    lead = k
                    run_end = k
                    while sum(counts[k:run_end + 1]) < npairs[k]:
                        run_end += 1
                    assert sum(counts[k:run_end + 1]) == npairs[k]                           # a leader's launch = a contiguous range of the sorted pairs
            if not merge:
                assert (npairs[wg] == counts[wg]).all()
        # "wgt_keep_waves": every class keeps its waves and its own launch, whatever `merge` says
        for merge in (True, False):
            nw, w, npairs = _lib.debug_threshold_groups(first, merge=merge, keep_waves=True)
            assert (npairs[wg] == counts[wg]).all()
            for k in wg:
                if counts[k]:
                    ci = class_info(k)
                    assert nw[k] == ci["waves"] and w[k] == ci["W"] + (ci["W"] & 1)


# ---- the launch schedule of a plan (ltrp::build_schedule) through ltr_debug_plan_schedule: every expectation below is worked out
# ---- here from the loci, never read back from the function ----

def _locus(rng, m, n_reads, n_haps, hap_len=None):
    """n_reads reads of m bases against n_haps haplotypes whose window (the haplotype less 2 x 30 of flank) is m bases too."""
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    return [seq(m) for _ in range(n_reads)], [seq(m + 60 if hap_len is None else hap_len) for _ in range(n_haps)]


def _grids(value=1000, **named):
    """Made-up occupancy grids: `value` everywhere; named: class index (int key via cls=...) or multi / pack_multi / plan."""
    g = np.full(NK + 3, value, dtype=np.int32)
    for name, v in named.items():
        g[{"multi": NK, "pack_multi": NK + 1, "plan": NK + 2}[name]] = v
    return g


def _class(family, W, lanes):
    return next(k for k in range(NK) if (class_info(k)["family"], class_info(k)["W"], class_info(k)["lanes"]) == (family, W, lanes))


def test_schedule_a_packed_width_is_one_launch_under_its_widest_segments():
    rng = np.random.default_rng(21)
    # mode 8: two lanes per pair whenever the read fits 2 x 20 columns, else the next segment width that holds it in 20 columns:
    # 640 columns = 32 x 20, 160 = 8 x 20 (4 x 20 is too few), 40 = 2 x 20 -- strip width 20 at 32, 8 and 2 lanes per pair
    batch = _abi.PackedBatch([_locus(rng, 641, 3, 2), _locus(rng, 161, 5, 2), _locus(rng, 41, 20, 2)])
    k32, k8, k2 = _class(1, 20, 32), _class(1, 20, 8), _class(1, 20, 2)
    s = _lib.debug_plan_schedule(batch, _grids(), mode=8)
    first = s["class_first"]
    assert [int(first[k + 1] - first[k]) for k in (k32, k8, k2)] == [6, 10, 40] and first[NK] == 56
    assert len(s["launches"]) == 1 and s["by_class"] == s["launches"] and not s["use_plan"] and not s["entries"]
    l = s["launches"][0]
    # waves: 6 pairs two at a time, 10 pairs eight at a time, 40 pairs 32 at a time = 3 + 2 + 2; four waves a workgroup
    assert (l["kind"], l["cls"], l["W"], l["members"]) == ("packed", k32, 20, [k32])
    assert l["cmax"] == 640 and l["pairs"] == 56 and l["cells"] == 6 * 641.0 * 641 + 10 * 161.0 * 161 + 40 * 41.0 * 41
    assert l["grid"] == 2 and l["small"]
    # ... capped by the occupancy grid of the class it is listed under (and by no other class's)
    g = _grids()
    g[k32] = 1
    l = _lib.debug_plan_schedule(batch, g, mode=8)["launches"][0]
    assert l["grid"] == 1 and not l["small"]
    g = _grids()
    g[k8] = g[k2] = 1
    assert _lib.debug_plan_schedule(batch, g, mode=8)["launches"][0]["grid"] == 2
    # without the 32-lane pairs the launch is listed under the 8-lane class
    s = _lib.debug_plan_schedule(_abi.PackedBatch([_locus(rng, 161, 5, 2), _locus(rng, 41, 20, 2)]), _grids(), mode=8)
    assert [(l["cls"], l["cmax"], l["pairs"], l["grid"]) for l in s["launches"]] == [(k8, 160, 50, 1)]


def _mixed_batch(rng, one_wave=(1201, 801), packed=(601, 481), extra=()):
    """Automatic mode at one CU (every batch counts as large: short reads are packed): one-wave classes for the reads beyond 641
    bases, packed classes below (41-base reads: 40 columns = 8 lanes x 5); 41-base reads against a 40-base haplotype are shortcuts
    (constant score): they keep the one-wave class of their length, W = 1.  24 pairs a one-wave class, 48 a packed one: six rounds of one CU's four wave slots, so
    that no class is folded into a wider one."""
    loci = [_locus(rng, m, 4, 6) for m in one_wave] + [_locus(rng, m, 4, 12) for m in packed]
    loci.append(_locus(rng, 41, 4, 12))
    loci.append(_locus(rng, 41, 4, 6, hap_len=40))
    loci.extend(extra)
    return _abi.PackedBatch(loci)


def test_schedule_launch_per_class_is_ordered_by_longest_read_ties_in_class_order():
    s = _lib.debug_plan_schedule(_mixed_batch(np.random.default_rng(22)), _grids(), n_cu=1, plan_kernel=1, no_multi=1)
    assert s["launches"] == s["by_class"] and not s["use_plan"] and not s["entries"] and s["n_tabs"] == 0
    assert all((l["kind"], l["pairs"]) in (("one-wave", 24), ("packed", 48)) for l in s["launches"])
    # W: 1200 columns in one block of 64 x 19, 800 in 64 x 13; packed 600 = 32 x 19, 480 = 32 x 15, 40 = 8 x 5; the shortcuts 40 = 64 x 1
    assert [(l["kind"], l["W"], l["cmax"]) for l in s["launches"]] == [
        ("one-wave", 19, 1200), ("one-wave", 13, 800), ("packed", 19, 600), ("packed", 15, 480), ("packed", 5, 40), ("one-wave", 1, 40)]
    assert s["launches"][4]["cls"] > s["launches"][5]["cls"]                 # the tie at 40 columns: descending class index
    assert s["launches"][5]["cells"] == 0.0 and s["launches"][4]["cells"] == 48 * 41.0 * 41      # (a shortcut has no cells)
    # 24 waves (one pair / two pairs each), four waves a workgroup; 48 pairs eight at a time = 6 waves
    assert [l["grid"] for l in s["launches"]] == [6, 6, 6, 6, 2, 6] and all(l["small"] for l in s["launches"])


def test_schedule_multi_width_launches_need_two_widths_with_pairs():
    rng = np.random.default_rng(23)
    kMultiMinW, kPackMultiMinW = 11, 13
    s = _lib.debug_plan_schedule(_mixed_batch(rng), _grids(multi=5), n_cu=1, plan_kernel=1, no_multi=-1)
    got = [(l["kind"], l["cmax"], l["pairs"], [class_info(k)["W"] for k in l["members"]]) for l in s["launches"]]
    assert got == [("multi", 1200, 48, [19, 13]), ("packed-multi", 600, 96, [19, 15]), ("packed", 40, 48, [5]), ("one-wave", 40, 24, [1])]
    assert all(class_info(k)["W"] >= kMultiMinW for k in s["launches"][0]["members"]) and all(class_info(k)["W"] >= kPackMultiMinW for k in s["launches"][1]["members"])
    multi, pmulti = s["launches"][:2]
    assert multi["cls"] == _class(0, 19, 64) and multi["grid"] == 5 and not multi["small"]        # 48 waves = 12 workgroups against 5 resident
    assert pmulti["cls"] == _class(1, 19, 32) and pmulti["grid"] == 12 and pmulti["small"] and s["n_tabs"] == 2     # 2 x 24 waves
    assert multi["cells"] == 24 * (1201.0 * 1201 + 801.0 * 801)
    # the level-2 list holds every class separately
    assert [(l["kind"], l["W"], l["cmax"], l["pairs"]) for l in s["by_class"]] == [
        ("one-wave", 19, 1200, 24), ("one-wave", 13, 800, 24), ("packed", 19, 600, 48), ("packed", 15, 480, 48), ("packed", 5, 40, 48), ("one-wave", 1, 40, 24)]
    # one width each: nothing to share, a launch per class
    s = _lib.debug_plan_schedule(_mixed_batch(rng, one_wave=(1201,), packed=(601,)), _grids(), n_cu=1, plan_kernel=1, no_multi=-1)
    assert [(l["kind"], l["W"], l["cmax"]) for l in s["launches"]] == [("one-wave", 19, 1200), ("packed", 19, 600), ("packed", 5, 40), ("one-wave", 1, 40)]
    assert s["launches"] == s["by_class"] and s["n_tabs"] == 0
    # two one-wave widths, one of them below kMultiMinW: 700 columns = 64 x 11, 40 (the shortcuts) = 64 x 1
    s = _lib.debug_plan_schedule(_mixed_batch(rng, one_wave=(701,), packed=()), _grids(), n_cu=1, plan_kernel=1, no_multi=-1)
    assert [(l["kind"], l["W"]) for l in s["launches"] if l["kind"] != "packed"] == [("one-wave", 11), ("one-wave", 1)] and len(s["launches"]) == 3


def _entry_longest(e, cmax, lanes=64):
    """The plan kernel's launch-order model of an entry: column blocks x (longest read + fill) x strip cost; packed: one block."""
    if e["kind"] == 1:
        return (cmax + float(lanes)) * (e["W"] + 1.5)
    return max(-(-cmax // (64 * e["W"])), 1) * (cmax + 64.0) * (e["W"] + 1.5)


def test_schedule_plan_kernel_is_one_launch_with_a_table_longest_first():
    rng = np.random.default_rng(24)
    # two list starters on top of the mixed batch: a read with a byte outside ACGT (generic list), a read 520 bases longer than
    # its window (no certificate can hold that: the list of its length, 820 columns = kXLong)
    n_read = _locus(rng, 201, 1, 2)
    n_read[0][0] = n_read[0][0][:5] + b"N" + n_read[0][0][6:]
    risky = _locus(rng, 821, 1, 3, hap_len=301 + 60)
    batch = _mixed_batch(rng, extra=[n_read, risky])
    s = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1)
    assert s["use_plan"] and len(s["launches"]) == 1 and s["n_tabs"] == 3
    p = s["launches"][0]
    one = [_class(0, w, 64) for w in (19, 13, 1)]
    packs = [_class(1, 19, 32), _class(1, 15, 32), _class(1, 5, 8)]
    assert p["kind"] == "plan" and p["cls"] == one[0] and p["members"] == one + packs and p["cmax"] == 1200 and p["pairs"] == 3 * 24 + 3 * 48
    # wavefronts: 3 x 24 one-wave pairs + 24 + 24 + 6 packed groups + 2 + 3 starters = 131 -> 33 workgroups against 20 resident
    assert p["grid"] == 20 and not p["small"] and s["max_grid"] == 20
    assert (s["xcand"] == 0).all() and (s["x_grid"] == 0).all()              # the plan kernel scores failed certificates and starters itself
    ents = s["entries"]
    assert [(e["kind"], e["W"], e["pairs"]) for e in ents[:2]] == [(2, 0, 2), (2, 1, 3)]      # the starters, generic list first
    cmax = {(0, 19): 1200, (0, 13): 800, (0, 1): 40, (1, 19): 600, (1, 15): 480, (1, 5): 40}
    # (the entry of the class the launch is listed under carries the launch's longest read, the first packed width the longest of
    # any packed width: here their own)
    want = sorted(cmax, key=lambda kw: -_entry_longest(dict(kind=kw[0], W=kw[1]), cmax[kw], lanes=8 if kw[1] == 5 else 32))
    assert [(e["kind"], e["W"]) for e in ents[2:]] == want
    assert [e["pairs"] for e in ents[2:] if e["kind"] == 0] == [24, 24, 24]
    fw = [e["first_wave"] for e in ents]
    assert fw[0] == 0 and fw == sorted(fw) and fw[-1] <= p["grid"] * 4 and len(set(fw)) > 2
    s1 = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1, plan_share=1)
    assert [e["first_wave"] for e in s1["entries"]] == [0] + [0x7fffffff] * (len(ents) - 1)
    assert [(e["kind"], e["W"]) for e in s1["entries"]] == [(e["kind"], e["W"]) for e in ents]

    # chain = 1: the chained walk (kind 3) for one-wave widths kMultiMinW .. kWMax whose scratch strip holds the parked row
    def chained(sched, lo=11, hi=20):
        have = 6 * ((sched["max_len"] + 2 + 15) // 16) * 16
        out = []
        for e in sched["entries"]:
            need = 2 * e["W"] * 64 + ((e["W"] + 3) // 4) * 32 + 2
            out.append(3 if e["kind"] == 0 and lo <= e["W"] <= hi and need <= have else e["kind"])
        return out
    sc = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1, chain=1)
    assert sc["max_len"] == 1201 and [e["kind"] for e in sc["entries"]] == chained(sc) and [e["kind"] for e in sc["entries"]].count(3) == 2
    sc = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1, chain=1, chain_min_w=14)
    assert [e["kind"] for e in sc["entries"]] == chained(sc, lo=14) and [e["kind"] for e in sc["entries"]].count(3) == 1
    sc = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1, chain=1, chain_min_w=3)       # (never below kMultiMinW)
    assert [e["kind"] for e in sc["entries"]].count(3) == 2
    asym = _abi.make_params((-1.0, -0.45, -1.0, -0.5, -0.0001, -10.0, -9.0))
    sc = _lib.debug_plan_schedule(batch, _grids(plan=20), n_cu=1, chain=1, params=asym)
    assert sc["use_plan"] and 3 not in [e["kind"] for e in sc["entries"]]
    # a strip too short for the parked row: the W = 11 class holds shortcuts only (701-base reads against a 40-base haplotype), and
    # shortcuts do not size the strips -- 201-base reads do: need = 2 x 11 x 64 + 3 x 32 + 2 = 1506 > have = 6 x 208 = 1248
    short = _abi.PackedBatch([_locus(rng, 701, 4, 6, hap_len=40), _locus(rng, 201, 4, 6)])
    sc = _lib.debug_plan_schedule(short, _grids(), n_cu=1, chain=1)
    assert sc["max_len"] == 201 and [(e["kind"], e["W"]) for e in sc["entries"]] == [(0, 11), (1, 7)] and chained(sc) == [0, 1]


def test_schedule_without_work_for_the_plan_kernel_falls_back_to_the_exact_launches():
    rng = np.random.default_rng(25)
    # a small batch (it cannot fill 256 CUs) with few long pairs: 1400 columns on four-wave workgroups, strips of 6 columns
    wg = _locus(rng, 1401, 3, 2)
    n_read = _locus(rng, 201, 1, 2)
    n_read[0][0] = n_read[0][0][:5] + b"N" + n_read[0][0][6:]
    s = _lib.debug_plan_schedule(_abi.PackedBatch([wg, n_read]), _grids(), n_cu=256)
    assert not s["use_plan"] and not s["entries"] and s["n_tabs"] == 0
    assert [(l["kind"], l["W"], l["cmax"], l["pairs"], l["grid"], l["members"]) for l in s["launches"]] == [("workgroup", 6, 1400, 6, 6, [])]
    assert class_info(s["launches"][0]["cls"])["lanes"] == 256 and s["by_class"] == s["launches"]
    # the two starters are the generic exact launch's; a failed certificate of the workgroup pairs lands in the four-wave list
    assert s["xcand"].tolist() == [2, 0, 0, 0, 6, 0] and s["x_grid"].tolist() == [1, 0, 0, 0, 6, 0]
    # with one pair for it the plan kernel takes the starters: they leave the exact launches' sizes
    s = _lib.debug_plan_schedule(_abi.PackedBatch([wg, n_read, _locus(rng, 201, 1, 1)]), _grids(), n_cu=256)
    assert s["use_plan"] and s["xcand"].tolist() == [0, 0, 0, 0, 6, 0] and [e["kind"] for e in s["entries"]] == [2, 0]
    assert [l["kind"] for l in s["launches"]] == ["workgroup", "plan"]


def test_schedule_grid_cap_lowers_the_strip_launches_only():
    rng = np.random.default_rng(26)
    # 100 one-wave pairs (a small batch keeps one pair per wavefront) = 25 workgroups; ten workgroup pairs = 10 workgroups
    batch = _abi.PackedBatch([_locus(rng, 301, 10, 10), _locus(rng, 1401, 5, 2)])
    for kw, kind in ((dict(), "plan"), (dict(plan_kernel=1, no_multi=1), "one-wave")):
        s = _lib.debug_plan_schedule(batch, _grids(), n_cu=256, **kw)
        assert [(l["kind"], l["grid"]) for l in s["launches"]] == [("workgroup", 10), (kind, 25)] and s["max_grid"] == 25
        c = _lib.debug_plan_schedule(batch, _grids(), n_cu=256, cap=7, **kw)
        assert [(l["kind"], l["grid"]) for l in c["launches"]] == [("workgroup", 10), (kind, 7)] and c["max_grid"] == 7
        assert all(l["grid"] == (10 if l["kind"] == "workgroup" else 7) for l in c["by_class"])
        assert [{**l, "grid": 0} for l in c["launches"]] == [{**l, "grid": 0} for l in s["launches"]]       # nothing else moves
        # the exact launches that park column blocks in strips are capped, the workgroup lists are not
        assert (c["x_grid"][:4] == np.minimum(s["x_grid"][:4], 7)).all() and (c["x_grid"][4:] == s["x_grid"][4:]).all()
        big = _lib.debug_plan_schedule(batch, _grids(), n_cu=256, cap=40, **kw)
        assert big["launches"] == s["launches"] and big["max_grid"] == 25


def test_schedule_grid_cap_switch_lowers_every_launch():
    """ltr_ctx_set_debug "grid_cap" (Schedule::cap_every_grid): the launches cap_grids leaves alone -- packed, workgroup, the four- and
    eight-wave exact lists, the W = 20 exact launch -- are lowered too, and nothing but grids moves."""
    rng = np.random.default_rng(27)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    # twelve families (one CU: families by rule from twelve up) of three members: twelve reads of 701 bases against three windows that share
    # 200 rows -> 3 workgroups; six workgroup pairs (2700 columns: a plan of twelve pairs per CU and more keeps reads of up to 2560 on
    # one wavefront; fewer than ten long pairs per CU) -> 6 workgroups and six
    # candidates of the four-wave list, whose W = 20 launch gets ceil(6 / 4) = 2; a read with an N -> the generic list
    prefix = seq(200)
    fam = ([seq(701) for _ in range(12)], [seq(30) + prefix + b"ACG"[k:k + 1] + seq(n) + seq(30) for k, n in enumerate((449, 499, 559))])
    n_read = _locus(rng, 201, 1, 2)
    n_read[0][0] = n_read[0][0][:5] + b"N" + n_read[0][0][6:]
    batch = _mixed_batch(rng, extra=[fam, _locus(rng, 2701, 3, 2), n_read])
    for kw, kinds in ((dict(), {"family", "workgroup", "plan"}), (dict(plan_kernel=1, no_multi=1), {"workgroup", "one-wave", "packed"})):
        s = _lib.debug_plan_schedule(batch, _grids(), n_cu=1, **kw)       # (families go with the plan kernel: a launch per class has none)
        assert {l["kind"] for l in s["launches"]} == kinds
        for kind in kinds:                                        # every kind has a launch the cap bites on
            assert max(l["grid"] for l in s["launches"] if l["kind"] == kind) > 2, kind
        # (the plan kernel scores its failed certificates in line; per class the 24 pairs of 1200 columns are candidates of the four-wave list too)
        n4 = 6 if not kw else 30
        assert s["x_grid"][4] == n4 and s["max_grid_wide"] == (n4 + 3) // 4 and s["max_grid"] > 2
        for cap in (1, 2):
            c = _lib.debug_plan_schedule(batch, _grids(), n_cu=1, grid_cap=cap, **kw)
            for name in ("launches", "by_class"):
                assert [l["grid"] for l in c[name]] == [min(l["grid"], cap) for l in s[name]]
                assert [{**l, "grid": 0} for l in c[name]] == [{**l, "grid": 0} for l in s[name]]                   # nothing else moves
            assert len(c["x_grid"]) == 6 and (c["x_grid"] == np.minimum(s["x_grid"], cap)).all() and c["x_grid"][4] == cap
            assert c["max_grid_wide"] == min(s["max_grid_wide"], cap) == cap and c["max_grid"] == cap
            assert c["entries"] == s["entries"] and c["n_tabs"] == s["n_tabs"] and c["use_plan"] == s["use_plan"] and c["max_len"] == s["max_len"]
            assert (c["xcand"] == s["xcand"]).all() and (c["class_first"] == s["class_first"]).all()
        # 0 is no cap
        assert _lib.debug_plan_schedule(batch, _grids(), n_cu=1, grid_cap=0, **kw)["launches"] == s["launches"]
