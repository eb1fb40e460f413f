"""The clustering of reads without an exact allele (gen_candidate_seqs, HaplotypeGenerator.cpp:376-472), host part: ltr_cluster_sequences
(longtr_amd/csrc/ltr_cluster.cpp) against the Python restatement tests/cluster_util.py on matrices from the plain DP, and the claim both
rest on -- the reference's needleman_wunsch with its row abort decides `score < T` exactly as the true distance does, except for an
empty second argument.  CPU only; everything is compared for equality."""
import numpy as np
import pytest

import cluster_util as cu
from longtr_amd import _abi, _lib


def _two_alleles(seed, la, lb, n_reads, err, period=5):
    rng = np.random.default_rng(seed)
    motif = cu.BASES[rng.integers(0, 4, size=period)]
    a, b = np.tile(motif, la // period + 1)[:la].tobytes(), np.tile(motif, lb // period + 1)[:lb].tobytes()
    return a, b, [cu.noisy_copy(rng, a if i % 2 == 0 else b, err) for i in range(n_reads)]


def _both(reads, candidates=(), shuffle_seed=None):
    """(sequences, counts, restatement's result with its trace, library's result), the library fed in a shuffled order when asked."""
    keys, counts = cu.unique_counts(reads)
    dist = cu.lev_matrix(keys, cu.CAP)
    trace = []
    want = cu.cluster(keys, counts, dist, candidates, trace=trace)
    got = _lib.cluster_sequences(keys, counts, dist, candidates)
    assert got == want
    if shuffle_seed is not None:                                    # the function orders its input itself
        perm = np.random.default_rng(shuffle_seed).permutation(len(keys))
        g2 = _lib.cluster_sequences([keys[i] for i in perm], [counts[i] for i in perm], dist[np.ix_(perm, perm)], candidates)
        assert g2["threshold"] == want["threshold"]
        assert [dict(c, centroid=int(perm[c["centroid"]]), members=[int(perm[m]) for m in c["members"]]) for c in g2["clusters"]] == want["clusters"]
    return keys, counts, want, trace


def test_reference_nw_with_row_abort_decides_like_the_distance():
    rng = np.random.default_rng(20240)
    n_pairs = 0
    for _ in range(300):
        a = cu.BASES[rng.integers(0, 4, size=int(rng.integers(0, 40)))].tobytes()
        b = cu.noisy_copy(rng, a, 0.25) if rng.random() < 0.6 else cu.BASES[rng.integers(0, 4, size=int(rng.integers(0, 40)))].tobytes()
        d = cu.lev(a, b)
        for T in (3, 5, 10, 20, 50):
            for x, y in ((a, b), (b, a)):
                score = cu.needleman_wunsch(x, y, T)
                assert (score < T) == (cu.nw_score(x, y, T, min(d, cu.CAP)) < T)     # what the clustering reads off the matrix
                if len(y) == 0 and len(x) > 0:                      # the exception: the inner loop never runs, min_score_per_row stays 1000
                    assert score == T + 1
                    continue
                assert (score < T) == (d < T), (x, y, T, score, d)
                if score < T:
                    assert score == d
                n_pairs += 1
    assert n_pairs > 2000
    # the exception, explicitly, both ways round: ("ACG", "") never joins, ("", "ACG") answers the length
    assert cu.needleman_wunsch(b"ACG", b"", 20) == 21 and cu.lev(b"ACG", b"") == 3
    assert cu.needleman_wunsch(b"", b"ACG", 20) == 3
    assert cu.needleman_wunsch(b"", b"", 20) == 0


# (seed, allele lengths, reads, error) -> (accepted threshold, clusters, new alleles, events the restatement must have seen)
SHAPES = {
    "two alleles 3 %": ((38, 300, 360, 30, 0.03), (20, 2, 2, {("merge", 20)})),
    "two alleles 3 %, 26 of 30 reads covered": ((22, 300, 360, 30, 0.03), (20, 6, 2, {("merge", 20)})),
    "two alleles 8 %": ((4, 300, 360, 30, 0.08), (50, 2, 2, {("too many centroids", 20), ("merge", 50)})),
    "two alleles of 1 kb": ((3, 1000, 1100, 30, 0.03), (80, 2, 2, {("too many centroids", 20), ("too many centroids", 50), ("merge", 80)})),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_two_allele_samples(name):
    (seed, la, lb, n_reads, err), (thr, n_clusters, n_new, events) = SHAPES[name]
    a, b, reads = _two_alleles(seed, la, lb, n_reads, err)
    keys, counts, want, trace = _both(reads, shuffle_seed=seed)
    new = sorted(len(keys[c["centroid"]]) for c in want["clusters"] if c["new_allele"])
    print(name, want["threshold"], len(want["clusters"]), new, trace)
    assert want["threshold"] == thr and len(want["clusters"]) == n_clusters and len(new) == n_new and events <= set(trace)
    assert abs(new[0] - la) <= 0.03 * la and abs(new[1] - lb) <= 0.03 * lb
    covered = sum(counts[m] for c in want["clusters"] if c["counted"] for m in c["members"])
    assert covered >= int(0.8 * n_reads) and (name != "two alleles 3 %, 26 of 30 reads covered" or covered == 26)


def test_one_allele_is_one_cluster_and_a_known_centroid_is_not_new():
    rng = np.random.default_rng(7)
    motif = cu.BASES[rng.integers(0, 4, size=5)]
    allele = np.tile(motif, 12).tobytes()
    reads = [cu.noisy_copy(rng, allele, 0.05) for _ in range(24)]
    keys, counts, want, _ = _both(reads, shuffle_seed=1)
    assert want["threshold"] == 20 and len(want["clusters"]) == 1 and want["clusters"][0]["new_allele"]
    assert sorted(want["clusters"][0]["members"]) == list(range(len(keys)))
    centroid = keys[want["clusters"][0]["centroid"]]
    _, _, again, _ = _both(reads, candidates=[b"ACGT", centroid])      # :457-458: already a candidate
    assert again["threshold"] == 20 and again["clusters"][0]["counted"] and not again["clusters"][0]["new_allele"]


def test_unrelated_sequences_pass_no_threshold():
    rng = np.random.default_rng(11)
    reads = [cu.BASES[rng.integers(0, 4, size=int(rng.integers(1500, 2500)))].tobytes() for _ in range(12)]
    keys, counts, want, trace = _both(reads)
    assert want == dict(threshold=-1, clusters=[]) and trace == []     # twelve clusters of one read at every threshold: none counts


def test_empty_sequence_first_follows_the_argument_order():
    """"" is the first std::map key and so the first centroid.  In the greedy step it is the SECOND argument: needleman_wunsch(read, "")
    answers T + 1 whatever the read's length, and no read joins it.  In merge_clusters it is the FIRST: needleman_wunsch("", centroid)
    answers the centroid's length, and it takes over every cluster whose centroid is shorter than T."""
    rng = np.random.default_rng(5)
    allele = cu.BASES[rng.integers(0, 4, size=12)].tobytes()
    reads = [b""] * 4 + [cu.noisy_copy(rng, allele, 0.15) for _ in range(20)]
    keys, counts, want, trace = _both(reads, shuffle_seed=3)
    assert keys[0] == b"" and max(len(k) for k in keys) < 20           # every read is nearer than T = 20 to "" by distance
    dist = cu.lev_matrix(keys, cu.CAP)
    greedy = {}
    assert cu.greedy_clustering([keys[0]] + sorted(keys[1:], key=cu._order), greedy, 20, cu._Dist(keys, dist))
    assert greedy[b""] == [b""] and len(greedy) == 2                    # by distance alone every read would have joined ""
    assert want["threshold"] == 20 and trace == [("merge", 20)] and len(want["clusters"]) == 1
    assert want["clusters"][0]["members"][0] == 0 and sorted(want["clusters"][0]["members"]) == list(range(len(keys)))
    assert keys[want["clusters"][0]["centroid"]] != b"" and want["clusters"][0]["new_allele"]          # the medoid of the merged cluster
    d = np.array([[0, 3], [3, 0]], dtype=np.int32)
    got = _lib.cluster_sequences([b"ACG", b""], [5, 5], d)
    assert got == cu.cluster([b"ACG", b""], [5, 5], d) and got["threshold"] == 20 and [c["members"] for c in got["clusters"]] == [[1, 0]]


def test_bad_input_is_refused():
    d = np.zeros((2, 2), dtype=np.int32)
    with pytest.raises(_lib.LtrError) as e:
        _lib.cluster_sequences([b"AC", b"AC"], [1, 1], d)               # the keys of a std::map are unique
    assert e.value.code == _abi.LTR_ERR_INVALID
    with pytest.raises(_lib.LtrError):
        _lib.cluster_sequences([b"AC", b"AG"], [1, 0], d)
    assert _lib.cluster_sequences([], [], np.zeros((0, 0), dtype=np.int32)) == dict(threshold=-1, clusters=[])


def test_edit_distances_without_a_context_is_an_error_not_a_fallback():
    with pytest.raises(_lib.LtrError) as e:
        _lib.edit_distances(None, [[b"ACGT", b"ACGA"]], 10)
    assert e.value.code == _abi.LTR_ERR_NO_DEVICE
