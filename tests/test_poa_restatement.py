"""tests/poa_util.py, the specification ltr_poa_consensus is held to, checked on its own: hand-checked groups, the alignment
score against a plain global alignment, and the consensus against the true sequence it was drawn from."""
import numpy as np

import cluster_util as cu
import poa_util as pu


def _rand(rng, n):
    return bytes(cu.BASES[rng.integers(0, 4, n)])


def test_hand_checked_groups():
    assert pu.poa_consensus([b"ACGT", b"ACGT", b"AGGT"]) == b"ACGT"
    assert pu.poa_consensus([b"GATTACA"]) == b"GATTACA"                              # one member: that member
    assert pu.poa_consensus([b"", b"GATTACA", b""]) == b"GATTACA"                    # empty members are dropped
    assert pu.poa_consensus([b"", b"", b""]) == b"" and pu.poa_consensus([]) == b""
    assert pu.poa_consensus([b"ACGT", b"AGGT"]) == b"ACGT"                           # equal weights and scores: the lower node id
    assert pu.poa_consensus([b"AAAA", b"AAAAAA", b"AAAAAA"]) == b"AAAAAA"


def test_a_group_of_31_uses_exactly_the_strided_30():
    rng = np.random.default_rng(1)
    true = _rand(rng, 60)
    members = [cu.noisy_copy(rng, true, 0.1) for _ in range(31)]
    picked = [members[(k * 31) // 30] for k in range(30)]
    assert picked == members[:30] and pu.used_members(members) == picked            # floor(k 31 / 30) = k for k < 30: the last one is left out
    assert pu.poa_consensus(members) == pu.poa_consensus(picked)
    # ... in a group whose consensus the 31st member would change: 15 against 15 is a tie that the lower node id wins
    odd = [b"ACGTACGT"] * 15 + [b"ACGAACGT"] * 16
    assert pu.used_members(odd) == odd[:30]
    assert pu.poa_consensus(odd) == pu.poa_consensus(odd[:30]) == b"ACGTACGT"
    assert pu.poa_consensus(odd[1:]) == b"ACGAACGT"                                  # (14 against 16, all thirty used)
    spread = [bytes([65 + i]) * 3 for i in range(45)]                               # of 45: the members at floor(k 45 / 30)
    assert pu.used_members(spread) == [spread[(k * 45) // 30] for k in range(30)] and spread[1] in pu.used_members(spread) and spread[2] not in pu.used_members(spread)
    assert pu.used_members([b""] * 5 + members) == picked                            # empty members are dropped first


def _global_alignment(a, b):
    """Plain Needleman-Wunsch: match +1, mismatch -1, gap -1."""
    prev = [-j for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        cur = [-i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = max(prev[j - 1] + (1 if a[i - 1] == b[j - 1] else -1), prev[j] - 1, cur[j - 1] - 1)
        prev = cur
    return prev[len(b)]


def test_against_a_chain_the_end_score_is_the_global_alignment():
    rng = np.random.default_rng(2)
    for k in range(20):
        a = _rand(rng, int(rng.integers(1, 60)))
        b = cu.noisy_copy(rng, a, 0.2) if k % 2 else _rand(rng, int(rng.integers(1, 60)))
        if not b:
            b = b"A"
        g = pu.Graph()
        g.add(a, [-1] * len(a))
        H = g.scores(b)
        end = g.end_node(H, len(b))
        assert end == len(a) - 1 and int(H[end][len(b)]) == _global_alignment(a, b), (a, b)
        aln = g.align(b)                                            # the traceback accounts for that score
        matches = sum(1 for c, v in zip(b, aln) if v >= 0 and g.letter[v] == c)
        mismatches = sum(1 for c, v in zip(b, aln) if v >= 0 and g.letter[v] != c)
        gaps = sum(1 for v in aln if v < 0) + (len(a) - matches - mismatches)
        assert matches - mismatches - gaps == _global_alignment(a, b)


def test_nine_copies_with_one_substitution_each_give_the_sequence():
    rng = np.random.default_rng(3)
    true = _rand(rng, 150)
    copies = []
    for k in range(9):
        p = 5 + 16 * k                                              # at least ten bases from every other copy's
        b = bytearray(true)
        b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + k % 3) % 4]
        copies.append(bytes(b))
    assert len(set(copies)) == 9 and true not in copies
    assert pu.poa_consensus(copies) == true


def draw(seed, n_reads=12, n_bases=300, err=0.05):
    """10 random bases + unit x k + 10 random bases, period 2 .. 6; n_reads unique noisy copies, ordered by length then sequence."""
    rng = np.random.default_rng(seed)
    period = int(rng.integers(2, 7))
    unit = _rand(rng, period)
    true = _rand(rng, 10) + unit * ((n_bases - 20) // period) + _rand(rng, 10)
    reads = set()
    while len(reads) < n_reads:
        reads.add(cu.noisy_copy(rng, true, err))
    return true, sorted(reads, key=cu._order)


SEEDS = tuple(range(12))


def test_the_consensus_is_closer_to_the_true_allele_than_the_medoid():
    """Twelve draws of 12 reads x 300 bases at error 0.05.  Seeds 0 .. 11 were tried on the CPU; the consensus was strictly closer than
    cluster_util.medoid for every one of them (distance 0 every time, against the medoid's 5 .. 12), so none was replaced."""
    for seed in SEEDS:
        true, reads = draw(seed)
        D = cu._Dist(reads, cu.lev_matrix(reads))
        medoid = cu.medoid(reads, {r: 1 for r in reads}, D)
        consensus = pu.poa_consensus(reads)
        print(seed, cu.lev(consensus, true), cu.lev(medoid, true))
        assert cu.lev(consensus, true) < cu.lev(medoid, true), seed
