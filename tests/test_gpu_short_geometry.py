"""GPU: the seeded stutter kernels (ltr_short.hip) at every side length, flank shape and block shape at which short_geometry or a
kernel takes another branch, against the CPU restatement ol.oracle_process_reads_short: bit for bit, every read, seeds equal.
The inputs are the crafted cases of short_util (tests/test_short_geometry_cases.py checks on the CPU that they reach their
shapes; every case here checks it again from the restatement's seeds before it compares).  The kernel path a call took is
read from set_debug("short_split"): the four-launch path leaves four positive device times, the lane-per-pair kernel none."""
import time

import numpy as np
import pytest

import oracle_lib as ol
import short_util as su
from longtr_amd import _abi

pytestmark = pytest.mark.gpu


def _prm():
    return _abi.make_params(_abi.default_params().as_tuple()[:7], use_short_path=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(blocks, alns, **kw):
    rc, want, ws = ol.oracle_process_reads_short(_prm(), _abi.default_stutter_params(), blocks, alns, **kw)
    assert rc == 0
    return want, ws


def _run(ctx, blocks, alns, lane_knob=False, **kw):
    """process_reads with the split events on -> (probs, seeds, the four split times); knobs and parameters restored."""
    ctx.set_params(_prm())
    try:
        ctx.short_kernel_split(reset=True)
        ctx.set_debug("short_split", 1)
        if lane_knob:
            ctx.set_debug("short_lane_kernel", 1)
        try:
            got, gs = ctx.process_reads(blocks, alns, **kw)
        finally:
            ctx.set_debug("short_lane_kernel", 0)
            ctx.set_debug("short_split", 0)
        split = ctx.short_kernel_split(reset=True)
    finally:
        ctx.set_params(_abi.default_params())
    return got, gs, split


def _same(got, gs, want, ws, what):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    m = ~np.isnan(want)
    bad = np.argwhere(bits(np.where(m, got, 0.0)) != bits(np.where(m, want, 0.0)))
    assert len(bad) == 0, (what, f"{len(bad)} of {want.size} scores differ; first (read, haplotype)", bad[:5].tolist())
    assert np.array_equal(gs, ws), what


def _check(ctx, blocks, alns, four_launch, what):
    """One call, no knob: equal to the restatement; the split times show the expected path.  Returns the sides."""
    want, ws = _oracle(blocks, alns)
    assert (ws > 0).all() and np.isfinite(want).all()
    sd = su.sides(alns, ws)
    mb = max(len(a) for a in blocks[1]["alleles"])
    assert su.geometry_of(blocks, sd, want.size)["four_launch"] is four_launch, what
    got, gs, split = _run(ctx, blocks, alns)
    print(f"{what}: sides {sorted(set(x for s in sd for x in s))}, longest block {mb}, split ms {split}")
    _same(got, gs, want, ws, what)
    if four_launch:
        assert len(split) == 4 and all(ms > 0 for ms in split), (what, split)
    else:
        assert split == [0.0, 0.0, 0.0, 0.0], (what, split)
    return sd, got


def test_a_side_length_edges_four_launch_path(gpu_ctx):
    blocks, alns = su.case_a()
    sd, got = _check(gpu_ctx, blocks, alns, True, "A")
    assert set(su.EDGE_SIDES) <= {l for l, _ in sd} and set(su.EDGE_SIDES) <= {r for _, r in sd}
    assert max(max(s) for s in sd) == 512                     # S = 514: the block kernel's thread loops run two full rounds
    lane, ls, split = _run(gpu_ctx, blocks, alns, lane_knob=True)
    assert split == [0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(bits(lane), bits(got)) and np.array_equal(ls, [s for s, _ in sd])


def test_b_past_512_the_rule_picks_the_lane_kernel(gpu_ctx):
    blocks, alns = su.case_b()
    sd, _ = _check(gpu_ctx, blocks, alns, False, "B")
    want = set(su.EDGE_SIDES + su.PAST_512)
    assert want <= {l for l, _ in sd} and want <= {r for _, r in sd}


@pytest.mark.parametrize("which", [1, 2, 3, 4])
def test_c_repeat_block_shapes(gpu_ctx, which):
    blocks, alns = su.case_c(which)
    sd, got = _check(gpu_ctx, blocks, alns, True, f"C{which}")
    flat = [x for s in sd for x in s]
    if which == 1:                                            # the empty block's in-place row on the lane-per-pair kernel, too
        lane, ls, split = _run(gpu_ctx, blocks, alns, lane_knob=True)
        assert split == [0.0, 0.0, 0.0, 0.0]
        assert np.array_equal(bits(lane), bits(got)) and np.array_equal(ls, [s for s, _ in sd])
    if which == 4:                                            # S from the longest block + 2, not from a read
        assert max(flat) + 2 < max(len(a) for a in blocks[1]["alleles"]) + 2
    else:
        assert min(flat) < 128 and max(flat) > 256
    if which == 1:
        assert sorted(len(a) for a in blocks[1]["alleles"]) == [0, 1, 2, 3, 5, 6, 7, 13]
    if which == 3:
        assert min(flat) == 10 and max(flat) >= 365 and any(l < 298 < r for l, r in sd) and any(r < 298 < l for l, r in sd)


@pytest.mark.parametrize("lf_len,rf_len,ne", [(lf, rf, ne) for (lf, rf), ne in zip(su.FLANK_SHAPES, [13, 13, 11, 11, 62, 64, 65, 140, 209])])
def test_d_flank_shapes_and_final_entries(gpu_ctx, lf_len, rf_len, ne):
    blocks, alns = su.case_d(lf_len, rf_len)
    assert 2 + (len(blocks[0]["alleles"][0]) - 1) + (len(blocks[2]["alleles"][0]) - 1) == ne
    sd, _ = _check(gpu_ctx, blocks, alns, True, f"D({lf_len},{rf_len})")
    if lf_len >= 9:
        assert {4, 30, 129, 260} <= {l for l, _ in sd}
    if rf_len >= 9:
        assert {4, 30, 129, 260} <= {r for _, r in sd}


def test_e_chunk_loop_three_chunks(gpu_ctx):
    blocks, distinct = su.case_e()
    want1, ws1 = _oracle(blocks, distinct)
    sd = su.sides(distinct, ws1)
    assert max(max(s) for s in sd) == 512
    S = max(512, max(len(a) for a in blocks[1]["alleles"]) + 2, 13) + 2
    cap = (2 ** 30 - 64) // (2 * 13 * 8 * S)                  # short_geometry: the block row's terms of a chunk fit one GB
    assert cap == 10043
    tiles, rr1, rh, pairs = su.case_e_tiling(len(distinct), cap)
    assert pairs > 2 * cap and pairs - 2 * cap < cap          # three chunks, the last partial
    alns, rr = distinct * tiles, np.tile(rr1, tiles)
    assert int(rr.sum()) * int(rh.sum()) == pairs
    want1, ws1 = _oracle(blocks, distinct, realign_hap=rh, realign_read=rr1)
    want, ws = np.tile(want1, (tiles, 1)), np.tile(ws1, tiles)
    t0 = time.perf_counter()
    got, gs, split = _run(gpu_ctx, blocks, alns, realign_hap=rh, realign_read=rr)
    print(f"E: {len(alns)} reads, {pairs} pairs, chunk capacity {cap}, process_reads {time.perf_counter() - t0:.2f} s, split ms (first chunk) {split}")
    assert all(ms > 0 for ms in split), split
    _same(got, gs, want, ws, "E")
    assert np.isfinite(got[np.ix_(rr == 1, rh == 1)]).all() and np.isnan(got[rr == 0]).all() and np.isnan(got[:, rh == 0]).all()


def test_f_lds_rule(gpu_ctx):
    # lds_bytes of short_geometry (worked out in tests/test_short_geometry_cases.py):
    #   alleles A*600,  A*601:   45467 bytes <= 64 KB -> the four launches
    #   alleles A*1500, A*1501: 112071 bytes >  64 KB -> the lane-per-pair kernel, though every side is under 512
    for block_len, lds, four in [(600, 45467, True), (1500, 112071, False)]:
        blocks, alns = su.case_f(block_len)
        sd, _ = _check(gpu_ctx, blocks, alns, four, f"F({block_len})")
        assert max(max(s) for s in sd) < 512 and 6 <= len(alns) <= 8
        assert su.geometry_of(blocks, sd, 2 * len(alns))["lds_bytes"] == lds


def test_g_one_batch_over_loci_of_very_different_geometry(gpu_ctx):
    from test_gpu_host_path import _expected_calc_hap_aln_probs
    loci = [su.case_a(), su.case_c(1), su.case_c(3), su.case_d(1, 12), su.case_c(4), su.case_d(200, 9)]
    for blocks, alns in loci:
        assert len(set(a["seq"] for a in alns)) == len(alns)  # every read is its own pool
    prm = _prm()
    gpu_ctx.set_params(prm)
    try:
        got = gpu_ctx.calc_hap_aln_probs([(b, a) for b, a in loci])
    finally:
        gpu_ctx.set_params(_abi.default_params())
    all_sides = set()
    for k, ((blocks, alns), (probs, seeds)) in enumerate(zip(loci, got)):
        want, ws = _expected_calc_hap_aln_probs(prm, _abi.default_stutter_params(), blocks, alns)
        assert np.isfinite(want).all()
        _same(probs, seeds, want, ws, f"G locus {k}")
        all_sides |= {x for s in su.sides(alns, ws) for x in s}
    assert min(all_sides) == 4 and max(all_sides) == 512      # one S stride for sides of 4 and of 512
