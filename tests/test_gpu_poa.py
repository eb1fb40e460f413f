"""-m gpu: ltr_poa_consensus (longtr_amd/csrc/ltr_poa.hip) against tests/poa_util.poa_consensus, byte for byte: a fuzz over group sizes,
lengths and alphabets with the groups where every tie rule fires, a group past one block of 64 columns many times over, more groups than
a launch keeps resident, and the memory rule (per-group cap, per-call budget) at lowered values."""
import numpy as np
import pytest

import cluster_util as cu
import poa_util as pu
from longtr_amd import _lib

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 89, 100, 127, 128, 129, 150, 200]


def _rand(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return bytes(a[rng.integers(0, len(a), n)])


def _noisy_group(rng, size, length, err, alphabet=b"ACGT"):
    true = _rand(rng, length, alphabet)
    out = []
    for _ in range(size):
        s = cu.noisy_copy(rng, true, err)
        out.append(s if len(s) > 0 or length == 0 else true)
    return out


def fuzz_groups():
    rng = np.random.default_rng(20261020)
    groups = []
    for i in range(203):
        size = 2 + i % 29                                           # 2 .. 30
        length = LENGTHS[(i * 7) % len(LENGTHS)]
        alphabet = b"ACGTN" if i % 3 == 0 else b"ACGT"
        if i % 5 == 4:                                              # unrelated members: long gaps, many columns
            groups.append([_rand(rng, max(1, int(rng.integers(length // 2, length + 1))), alphabet) for _ in range(size)])
        else:
            groups.append(_noisy_group(rng, size, length, (0.02, 0.08, 0.2)[i % 3], alphabet))
    for size in (31, 45, 64):                                       # the strided 30
        groups.append(_noisy_group(rng, size, 40, 0.1))
    groups.append([b"ACGTACGT", b"", b"ACGAACGT", b"", b"ACGTACGT"])                  # empty members are dropped
    groups.append([b"A" * n for n in (7, 9, 8, 12, 7, 1, 10)])                          # homopolymers: every tie rule fires
    base = _rand(rng, 90)
    subs = []
    for k in range(9):                                              # substitutions only, equal lengths
        b = bytearray(base)
        for p in rng.integers(0, 90, 4):
            b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + k % 3) % 4]
        subs.append(bytes(b))
    groups.append(subs)
    dup = _noisy_group(rng, 4, 70, 0.05)
    groups.append([dup[0], dup[1], dup[0], dup[2], dup[1], dup[3], dup[0]])           # duplicate members
    groups.append([b"", b""])                                       # nothing left
    groups.append([b"", b"GATTACA"])                                # one member left: that member
    groups.append([b"ACGT", b"ACGT", b"AGGT"])
    return groups


def test_fuzz_equals_the_restatement(gpu_ctx):
    groups = fuzz_groups()
    assert len(groups) >= 200
    want = [pu.poa_consensus(g) for g in groups]
    got, status = gpu_ctx.poa_consensus(groups, with_status=True)
    assert status == [0] * len(groups)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (bad[:10], [(len(groups[i]), max(len(s) for s in groups[i])) for i in bad[:10]])
    assert got[-1] == b"ACGT" and got[-2] == b"GATTACA" and got[-3] == b""


def test_long_group_crosses_the_column_blocks(gpu_ctx):
    """8 members of about 2100 bases: 33 blocks of 64 columns a row, int16 cells (8 x 2100 + 2100 <= 32767), graph arrays in scratch."""
    rng = np.random.default_rng(7)
    unit = _rand(rng, 4)
    true = _rand(rng, 10) + unit * 520 + _rand(rng, 10)
    group = []
    while len(group) < 8:
        s = cu.noisy_copy(rng, true, 0.04)
        if s not in group:
            group.append(s)
    want = pu.poa_consensus(group)
    got, status = gpu_ctx.poa_consensus([group], with_status=True)
    assert status == [0] and got[0] == want
    assert cu.lev(want, true) < min(cu.lev(s, true) for s in group)


def test_wide_cells(gpu_ctx):
    """30 members of 1100 bases: 33 000 bases + 1100 > 32767, so the rows are int32 cells."""
    rng = np.random.default_rng(11)
    true = _rand(rng, 1100)
    group = [cu.noisy_copy(rng, true, 0.02) for _ in range(30)]
    assert sum(len(s) for s in group) + max(len(s) for s in group) > 32767
    got = gpu_ctx.poa_consensus([group])
    assert got[0] == pu.poa_consensus(group)


def test_a_thousand_groups_in_any_order(gpu_ctx):
    rng = np.random.default_rng(3)
    groups = [_noisy_group(rng, 3, 20, 0.1) for _ in range(1000)]
    want = [pu.poa_consensus(g) for g in groups]
    got = gpu_ctx.poa_consensus(groups)
    assert got == want
    assert gpu_ctx.poa_consensus(groups) == got                     # the same call twice: the same bytes
    perm = rng.permutation(len(groups))
    shuffled = gpu_ctx.poa_consensus([groups[k] for k in perm])
    assert shuffled == [want[k] for k in perm]


def test_group_over_the_cap_reports_it_and_leaves_its_neighbours(gpu_ctx):
    """cap = 256 KB.  4 x 20 bases: graph arrays in LDS, rows of a few KB.  8 x 1000 bases: the graph arrays alone (50 bytes a base = 400 KB)
    are over the cap, the host says so.  6 x 300 bases: graph arrays 90 KB, rows of the second alignment (300 + 1) x (300 + 1) x 2 =
    181 KB > 256 - 90 KB: the wavefront says so."""
    rng = np.random.default_rng(5)
    small = [_noisy_group(rng, 4, 20, 0.1) for _ in range(4)]
    by_host, by_wave = _noisy_group(rng, 8, 1000, 0.03), _noisy_group(rng, 6, 300, 0.03)
    assert min(len(s) for s in by_wave) >= 280
    groups = [small[0], by_host, small[1], small[2], by_wave, small[3]]
    want = [pu.poa_consensus(g) for g in groups]
    try:
        gpu_ctx.set_debug("poa_group_cap_bytes", 256 << 10)
        got, status = gpu_ctx.poa_consensus(groups, with_status=True)
    finally:
        gpu_ctx.set_debug("poa_group_cap_bytes", 0)
    assert status == [0, 1, 0, 0, 1, 0]
    assert got == [want[0], b"", want[2], want[3], b"", want[5]]
    assert [pu.poa_consensus_capped(g, 256 << 10) for g in groups] == list(zip(got, status))     # the rule as the restatement states it
    got, status = gpu_ctx.poa_consensus(groups, with_status=True)   # the library's own cap: all aligned
    assert status == [0] * 6 and got == want


def test_budget_that_forces_three_launch_sets_changes_nothing(gpu_ctx):
    """9 groups of 4 x 100 bases (none longer): 400 bases each = 20 KB of graph arrays (over the 16 KB that go to LDS) + at most 401 x 101 x 2 = 81 KB
    of rows, some 100 KB a group; a budget of 350 KB holds three of them, so the call takes three launch sets."""
    rng = np.random.default_rng(9)
    groups = []
    for _ in range(9):
        true = _rand(rng, 100)
        g = []
        for _ in range(4):
            b = bytearray(true)
            for p in rng.integers(0, 100, 5):
                b[p] = b"ACGT"[int(rng.integers(0, 4))]
            del b[int(rng.integers(0, 100))]
            b.insert(int(rng.integers(0, 99)), b"ACGT"[int(rng.integers(0, 4))])
            g.append(bytes(b))
        groups.append(g)
    assert all(len(s) == 100 for g in groups for s in g)
    want = [pu.poa_consensus(g) for g in groups]
    one = gpu_ctx.poa_consensus(groups)
    try:
        gpu_ctx.set_debug("poa_call_budget_bytes", 350 << 10)
        three, status = gpu_ctx.poa_consensus(groups, with_status=True)
    finally:
        gpu_ctx.set_debug("poa_call_budget_bytes", 0)
    assert status == [0] * 9 and three == one == want
