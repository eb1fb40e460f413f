"""-m gpu: ltr_edit_distances (longtr_amd/csrc/ltr_editdist.hip, the bit-vector block kernel) == the plain DP (tests/cluster_util.py) on
every geometry edge of the kernel: block edges and the partial last block, segments of 1 / 2 / 4 / 64 lanes in one launch, the pass
boundary at 4096 rows with the boundary strip in LDS and in global memory, the host's shortcut for |n - m| >= cap and its launched
neighbour, odd alphabets, empty groups, many wavefronts.  Integers, compared for equality."""
import numpy as np
import pytest

import cluster_util as cu
from longtr_amd import _abi, _lib

pytestmark = pytest.mark.gpu


def _rand(rng, n):
    return cu.BASES[rng.integers(0, 4, size=n)].tobytes()


def _check(ctx, groups, cap):
    got = ctx.edit_distances(groups, cap)
    assert len(got) == len(groups)
    for g, (seqs, d) in enumerate(zip(groups, got)):
        want = cu.lev_matrix(seqs, cap)
        assert d.shape == want.shape and d.dtype == np.int32
        assert np.array_equal(d, want), (g, np.argwhere(d != want)[:5], d[d != want][:5], want[d != want][:5])
    return got


def test_block_edges_and_mixed_segment_widths(gpu_ctx):
    """Patterns of 0, 1, 63, 64, 65, 127, 128, 129 rows (LP 1 / 2 / 4) against texts of the same length, +1 and +70, noisy copies and
    unrelated sequences, all in ONE group: segments of different widths share the launch."""
    rng = np.random.default_rng(401)
    seqs = []
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        p = _rand(rng, n)
        seqs.append(p)
        for extra in (0, 1, 70):
            noisy = cu.noisy_copy(rng, p, 0.08)
            seqs.append((noisy + _rand(rng, n + extra))[:n + extra])        # a noisy copy, cut or filled to the length
            seqs.append(_rand(rng, n + extra))                              # unrelated
    seqs = sorted(set(seqs))
    assert len(seqs) >= 50 and b"" in seqs
    d = _check(gpu_ctx, [seqs], 32767)[0]
    assert np.array_equal(d, d.T) and (np.diag(d) == 0).all() and d.max() > 129
    _check(gpu_ctx, [seqs], 20)


def test_pass_boundary_and_boundary_strips(gpu_ctx):
    """Noisy copies of one another of 4095 / 4096 / 4097 / 4100 / 8200 / 8300 bases: LP = 64, one pass (4095, 4096), two passes with
    the boundary strip in LDS (4097 x 4100) and in global memory (4097 x 8200, text beyond 8192 columns), three passes (8200 x 8300)."""
    rng = np.random.default_rng(402)
    base = _rand(rng, 8300)
    seqs = [cu.noisy_copy(rng, base[:n], 0.02)[:n] for n in (4095, 4096, 4097, 4100, 8200, 8300)]
    seqs = [s + _rand(rng, n - len(s)) for s, n in zip(seqs, (4095, 4096, 4097, 4100, 8200, 8300))]
    assert [len(s) for s in seqs] == [4095, 4096, 4097, 4100, 8200, 8300]
    d = _check(gpu_ctx, [seqs], 32767)[0]
    assert 0 < d[2, 3] < 400 and d[4, 5] < 700 and d[0, 5] >= 8300 - 4095


def test_cap_and_the_host_shortcut(gpu_ctx):
    rng = np.random.default_rng(403)
    p = _rand(rng, 200)
    seqs = [p] + [cu.noisy_copy(rng, p, 0.02)[:150] + _rand(rng, 50 + k) for k in (49, 50, 51)] + [_rand(rng, 200)]
    assert [len(s) - 200 for s in seqs[1:4]] == [49, 50, 51]             # |n - m| = cap - 1 (launched), cap, cap + 1 (the host's)
    d = _check(gpu_ctx, [seqs], 50)[0]
    assert d[0, 2] == 50 and d[0, 3] == 50 and d.max() == 50
    d1 = _check(gpu_ctx, [seqs + [p[:199] + b"A", p[:199] + b"C"]], 1)[0]
    assert set(np.unique(d1)) == {0, 1}


def test_bytes_are_compared_as_they_are_and_33_codes_are_refused(gpu_ctx):
    rng = np.random.default_rng(404)
    p = _rand(rng, 90)
    odd = [p, p.lower(), p[:30] + b"N" * 30 + p[60:], p[:30] + b"n" * 30 + p[60:], b"N" * 90, p[:45] + p[45:].lower()]
    d = _check(gpu_ctx, [odd], 701)[0]
    assert d[0, 1] == 90 and d[2, 3] == 30 and d[2, 4] == 60             # N equals N; nothing is case-folded
    many = [bytes(range(40, 73)), bytes(range(41, 73)) + b"A"]           # 33 distinct bytes
    dist = np.full(1 + 4, -7, dtype=np.int32)
    with pytest.raises(_lib.LtrError) as e:
        _lib.edit_distances(gpu_ctx, [[b"AC"], many], 10, dist=dist)
    assert e.value.code == _abi.LTR_ERR_INVALID and "group 1" in str(e.value) and (dist == -7).all()
    ok = [bytes(range(40, 72)), bytes(range(41, 72)) + b"("]             # 32 are accepted
    _check(gpu_ctx, [ok], 100)
    for cap in (0, 32768):
        with pytest.raises(_lib.LtrError):
            _lib.edit_distances(gpu_ctx, [[b"AC", b"AG"]], cap)


def test_small_groups_next_to_a_large_one(gpu_ctx):
    rng = np.random.default_rng(405)
    p = _rand(rng, 330)
    forty = sorted({cu.noisy_copy(rng, p, 0.05) for _ in range(40)})
    groups = [[], [_rand(rng, 50)], [_rand(rng, 70), _rand(rng, 75)], forty, [], [b"", b""]]
    got = _check(gpu_ctx, groups, 701)
    assert got[0].shape == (0, 0) and got[1].tolist() == [[0]] and got[5].tolist() == [[0, 0], [0, 0]]


def test_many_groups_in_one_call(gpu_ctx):
    """300 groups of 20 sequences of ~100 bases: 57 000 pairs, many wavefronts, a partial last segment in most of them."""
    rng = np.random.default_rng(406)
    groups = []
    for g in range(300):
        p = _rand(rng, int(rng.integers(60, 140)))
        groups.append([cu.noisy_copy(rng, p, 0.1) + bytes([65 + g % 4]) * (k % 3) for k in range(20)])
    got = gpu_ctx.edit_distances(groups, 701)
    pairs = [(g, i, j) for g in range(300) for i in range(20) for j in range(i + 1, 20)]
    want = cu.lev_batch([(groups[g][i], groups[g][j]) for g, i, j in pairs])
    bad = [(g, i, j, int(got[g][i, j]), w) for (g, i, j), w in zip(pairs, want) if got[g][i, j] != w or got[g][j, i] != w]
    assert not bad, bad[:5]
    assert all((np.diag(d) == 0).all() for d in got)
