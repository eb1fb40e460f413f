"""CPU: the crafted short-path cases of short_util (the inputs of tests/test_gpu_short_geometry.py) reach the side lengths,
flank shapes and block lengths they are meant to reach, the restatement scores them (rc 0, finite), and the geometry rules
of the library's short_geometry (ltr_short_batch.cpp) restated in short_util.geometry give the constants worked out by hand below -- and
the restatement equals the library's rule itself (test hook ltr_debug_short_geometry), for every case here and over a grid."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle_lib as ol
import short_util as su
from longtr_amd import _abi, _lib


def lib_geometry(max_side, max_block, max_hap, n_pairs, lane_knob=0):
    """short_geometry of the library for a batch with these maxima, in short_util.geometry's terms (+ LP, grid, per_block)."""
    out = (C.c_int64 * 8)()
    assert _lib.lib().ltr_debug_short_geometry(max_side, max_block, max_hap, n_pairs, lane_knob, out) == 0
    S, HS, LP, lds, cap, wave, grid, per_block = list(out)
    return dict(S=S, HS=HS, lds_bytes=lds, chunk_cap=cap, four_launch=bool(wave)), dict(LP=LP, grid=grid, per_block=per_block)


def geometry(max_side, max_block, max_hap, n_pairs):
    """su.geometry, held to the library's rule"""
    g = su.geometry(max_side, max_block, max_hap, n_pairs)
    assert g == lib_geometry(max_side, max_block, max_hap, n_pairs)[0], (max_side, max_block, max_hap, n_pairs)
    return g


def geometry_of(blocks, side_list, n_pairs):
    """su.geometry_of, held to the library's rule"""
    g = su.geometry_of(blocks, side_list, n_pairs)
    mb = max(len(a) for a in blocks[1]["alleles"])
    args = (max(max(s) for s in side_list), mb, len(blocks[0]["alleles"][0]) + mb + len(blocks[2]["alleles"][0]), n_pairs)
    assert g == su.geometry(*args) == lib_geometry(*args)[0], args
    return g


def _prm():
    return _abi.make_params(_abi.default_params().as_tuple()[:7], use_short_path=1)


def _score(blocks, alns):
    rc, probs, seeds = ol.oracle_process_reads_short(_prm(), _abi.default_stutter_params(), blocks, alns)
    assert rc == 0 and (seeds > 0).all(), seeds
    assert np.isfinite(probs).all() and (probs < 1e-10).all()
    return su.sides(alns, seeds)


def test_seed_sits_where_the_builder_says():
    rng = np.random.default_rng(1)
    blocks = su.crafted_locus(35, [b"A" * 14, b"A" * 9], 40)
    assert set(blocks[0]["alleles"][0] + blocks[2]["alleles"][0]) <= set(b"CGT")
    for allele in (0, 1):
        a = su.crafted_read(blocks, allele, 23, 11, "left", rng)
        assert ol.oracle_calc_seed_base(a, blocks) == 23 + (35 - 1) // 2 and len(a["seq"]) == 23 + 35 + len(blocks[1]["alleles"][allele]) + 40 + 11
        a = su.crafted_read(blocks, allele, 23, 11, "right", rng)
        assert len(a["seq"]) - ol.oracle_calc_seed_base(a, blocks) - 1 == 11 + 40 // 2
        a = su.crafted_read(blocks, allele, -10, -7, "left", rng)                       # starts / ends inside the flanks
        assert ol.oracle_calc_seed_base(a, blocks) == (25 - 1) // 2 and len(a["seq"]) == 25 + len(blocks[1]["alleles"][allele]) + 33
        a = su.crafted_read(blocks, allele, -10, -7, "right", rng)
        assert len(a["seq"]) - ol.oracle_calc_seed_base(a, blocks) - 1 == 33 // 2
    # fewer than 9 flank bases under the '=' run: no seed (MIN_SEED_DIST); 9: sides of 4
    assert ol.oracle_calc_seed_base(su.crafted_read(blocks, 0, -27, 0, "left", rng), blocks) == -1
    assert ol.oracle_calc_seed_base(su.crafted_read(blocks, 0, -26, 0, "left", rng), blocks) == 4
    a = su.crafted_read(blocks, 0, 0, 0, "left", rng, plant_quals={0: " ", 3: "!", -1: "~"}, plant_bases={5: "N", -2: "a"})
    assert a["qual"][0] == ord(" ") and a["qual"][3] == ord("!") and a["qual"][-1] == ord("~") and a["seq"][5] == ord("N") and a["seq"][-2] == ord("a")
    assert min(a["qual"][1:3]) >= ord("#") and max(a["qual"][:-1]) <= ord("J")
    for lf, s in [(35, 4), (35, 16), (35, 17), (35, 512), (12, 4), (9, 4), (200, 30), (200, 99), (200, 260)]:
        b = su.crafted_locus(lf, [b"A" * 5], lf)
        a = su.crafted_read(b, 0, su.left_pad_for(lf, s), 0, "left", rng)
        assert ol.oracle_calc_seed_base(a, b) == s
        a = su.crafted_read(b, 0, 0, su.right_pad_for(lf, s), "right", rng)
        assert len(a["seq"]) - ol.oracle_calc_seed_base(a, b) - 1 == s


def test_case_a_and_b_reach_every_edge_side():
    blocks, alns = su.case_a()
    sd = _score(blocks, alns)
    assert set(su.EDGE_SIDES) <= {l for l, _ in sd} and set(su.EDGE_SIDES) <= {r for _, r in sd}
    assert max(max(s) for s in sd) == 512
    assert all(min(s) <= 64 for s in sd)                                                  # the other side of every read is short
    assert geometry_of(blocks, sd, 3 * len(alns))["four_launch"]
    assert any(b" " in a["qual"] and b"!" in a["qual"] and b"~" in a["qual"] and b"N" in a["seq"] and a["seq"] != a["seq"].upper() for a in alns)
    blocks, alns = su.case_b()
    sb = _score(blocks, alns)
    assert sb[:len(sd)] == sd
    assert set(su.EDGE_SIDES + su.PAST_512) <= {l for l, _ in sb} and set(su.EDGE_SIDES + su.PAST_512) <= {r for _, r in sb}
    assert not geometry_of(blocks, sb, 3 * len(alns))["four_launch"]


@pytest.mark.parametrize("which", [1, 2, 3, 4])
def test_case_c_block_shapes(which):
    blocks, alns = su.case_c(which)
    sd = _score(blocks, alns)
    flat = [x for s in sd for x in s]
    assert min(flat) < 128 and max(flat) > 256 if which != 4 else max(flat) > 128
    lens = sorted(len(a) for a in blocks[1]["alleles"])
    g = geometry_of(blocks, sd, len(alns) * len(lens))
    assert g["four_launch"]
    if which == 1:
        assert lens == [0, 1, 2, 3, 5, 6, 7, 13]                                          # num_deletions 0, 1, 2, 3, 5, 6, 6, 6
    if which == 2:
        assert all(b"G" in a for a in blocks[1]["alleles"])
    if which == 3:
        assert min(flat) == 10 and 365 <= max(flat) <= 375 and any(l < 298 and r > 298 for l, r in sd) and any(r < 298 and l > 298 for l, r in sd)
    if which == 4:                                                                        # no read as long as the longest block + 2
        assert max(flat) + 2 < 301 + 2 and g["S"] == 301 + 2 + 2


@pytest.mark.parametrize("lf_len,rf_len,ne", [(lf, rf, ne) for (lf, rf), ne in zip(su.FLANK_SHAPES, [13, 13, 11, 11, 62, 64, 65, 140, 209])])
def test_case_d_flank_shapes(lf_len, rf_len, ne):
    blocks, alns = su.case_d(lf_len, rf_len)
    sd = _score(blocks, alns)
    assert len(blocks[0]["alleles"][0]) == lf_len and len(blocks[2]["alleles"][0]) == rf_len
    assert 2 + (lf_len - 1) + (rf_len - 1) == ne                                          # the final kernel's entry count
    want = {4, 30, 129, 260}
    if lf_len >= 9:
        assert want <= {l for l, _ in sd}
    if rf_len >= 9:
        assert want <= {r for _, r in sd}
    assert len(alns) == 4 * ((lf_len >= 9) + (rf_len >= 9)) > 0


def test_case_f_and_the_lds_rule():
    # lds_bytes = (4 S + n_ilog) * 8 + (6 maxB + 8) * 4 + roundup8(S) + HS + 64, S = max(side, maxB + 2, 13) + 2, HS = maxHS + 4,
    # n_ilog = maxHS + maxB + 16, maxHS = 35 + maxB + 35:
    #   maxB  601: S  605, maxHS  671, n_ilog 1288: 3708 * 8 = 29664, 3614 * 4 = 14456,  608,  675, 64 ->  45467  (<= 65536)
    #   maxB 1501: S 1505, maxHS 1571, n_ilog 3088: 9108 * 8 = 72864, 9014 * 4 = 36056, 1512, 1575, 64 -> 112071  (>  65536)
    for block_len, lds, four in [(600, 45467, True), (1500, 112071, False)]:
        blocks, alns = su.case_f(block_len)
        sd = _score(blocks, alns)
        assert 6 <= len(alns) <= 8 and max(max(s) for s in sd) < 512 and max(max(s) for s in sd) > 256 and min(min(s) for s in sd) < 128
        g = geometry_of(blocks, sd, 2 * len(alns))
        assert g["lds_bytes"] == lds and g["four_launch"] is four and g["S"] == block_len + 5


def test_chunk_rule_constants():
    # cap = (2^30 - 64) // (2 * 13 * 8 * S): a maximum side of 512 (block 15) gives S = 514, 208 * 514 = 106912,
    # 1073741760 // 106912 = 10043 (10043 * 106912 = 1073717216, remainder 24544)
    g = geometry(512, 15, 85, 10 ** 6)
    assert g["S"] == 514 and g["chunk_cap"] == 10043
    assert geometry(512, 15, 85, 300)["chunk_cap"] == 300                              # one chunk when the call is small
    assert geometry(20, 300, 370, 10 ** 6)["S"] == 304                                 # the block, not the side
    assert geometry(5, 0, 13, 10 ** 6)["S"] == 15                                      # the 13 artifact sizes
    blocks, alns = su.case_e()
    sd = _score(blocks, alns)
    assert len(alns) == 48 and sorted(max(s) for s in sd)[-3:] == [sorted(max(s) for s in sd)[-3], 512, 512] and sorted(max(s) for s in sd)[-3] <= 64
    assert sd[0][0] == 512 and sd[1][1] == 512
    cap = geometry_of(blocks, sd, 10 ** 6)["chunk_cap"]
    tiles, rr, rh, pairs = su.case_e_tiling(len(alns), cap)
    assert cap == 10043 and pairs == tiles * 46 * 2 and 2 * cap < pairs <= 2 * cap + 92 and rr[0] and rr[1]      # three chunks, the last partial


def test_restatement_equals_the_library_rule_over_a_grid():
    for max_side, max_block, n_pairs in itertools.product([1, 4, 128, 129, 511, 512, 513, 700, 1100], [0, 1, 15, 300, 601, 1501], [1, 300, 10 ** 6]):
        g = geometry(max_side, max_block, 70 + max_block, n_pairs)
        assert g["four_launch"] == (max_side <= 512 and g["lds_bytes"] <= 65536)
        # the knob ("short_lane_kernel") forces the lane-per-pair kernel and changes nothing else
        want, rest = lib_geometry(max_side, max_block, 70 + max_block, n_pairs)
        forced, rest_forced = lib_geometry(max_side, max_block, 70 + max_block, n_pairs, lane_knob=1)
        assert not forced["four_launch"] and dict(forced, four_launch=want["four_launch"]) == want and rest_forced == rest
        # LP = max(S, HS) + 8; per_block = (19 S + LP + 2 (HS + 2)) * 64 doubles; grid = min(ceil(pairs / 64), 4096, 8 GB / per_block bytes)
        assert rest["LP"] == max(g["S"], g["HS"]) + 8 and rest["per_block"] == (19 * g["S"] + rest["LP"] + 2 * (g["HS"] + 2)) * 64
        assert rest["grid"] == min((n_pairs + 63) // 64, 4096, max(1, (8 << 30) // (rest["per_block"] * 8)))
    assert _lib.lib().ltr_debug_short_geometry(-1, 0, 70, 1, 0, (C.c_int64 * 8)()) != 0
