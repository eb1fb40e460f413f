"""The checker of the clustering step (gen_candidate_seqs, reference src/SeqAlignment/HaplotypeGenerator.cpp:376-472), restated in Python:

  lev / lev_batch / lev_matrix   the plain unit-cost DP (the recurrence of :224), vectorised over a row / over many pairs
  needleman_wunsch               :201-234 literally, with its length test and its row abort
  nw_score                       what the clustering reads off a distance matrix instead, with the empty-centroid exception
  greedy_clustering              :237-268
  merge_clusters                 :271-293
  cluster                        the ladder, the refinement and the acceptance of :399-470 for one sample, with the cluster MEDOID where
                                 the reference calls poa (:427; spoa is not reproducible: it samples with std::random_device)
  build_haplotype_clustered      oracle/ltr_oracle_prep.py's build_haplotype as it is, with `cluster` per sample between :373 and :475

Everything is an integer or a byte string: the tests compare for equality."""
import numpy as np

LADDER = (20, 50, 80, 100, 150, 200, 300, 400, 500, 600, 700)       # :405
CAP = 701
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def lev(a, b):
    """Unit-cost edit distance, bytes compared for equality (:223-224), one numpy row per base of the shorter sequence."""
    a, b = np.frombuffer(bytes(a), dtype=np.uint8), np.frombuffer(bytes(b), dtype=np.uint8)
    if len(a) > len(b):
        a, b = b, a
    idx = np.arange(len(b) + 1, dtype=np.int64)
    prev = idx.copy()
    t = np.empty(len(b) + 1, dtype=np.int64)
    for i, ca in enumerate(a, 1):
        t[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + (b != ca), out=t[1:])
        prev = np.minimum.accumulate(t - idx) + idx                 # D[i][j] = min_k (t[k] + j - k): the horizontal gaps
    return int(prev[-1])


def lev_batch(pairs, chunk=None):
    """lev for many (a, b) pairs at once: one DP over [pairs x columns] per chunk of pairs of similar length, padded (the pad never
    reaches D[n][m]); int16 rows while the lengths allow it (the rows stay in cache)."""
    if not pairs:
        return []
    pairs = [(bytes(a), bytes(b)) if len(a) <= len(b) else (bytes(b), bytes(a)) for a, b in pairs]
    order = sorted(range(len(pairs)), key=lambda p: (len(pairs[p][0]), len(pairs[p][1])))
    chunk = chunk or max(16, min(1024, 131072 // (max(len(b) for _, b in pairs) + 1)))
    result = [0] * len(pairs)
    for c0 in range(0, len(order), chunk):
        sel = order[c0:c0 + chunk]
        sub = [pairs[p] for p in sel]
        P, nmax, mmax = len(sub), max(len(a) for a, _ in sub), max(len(b) for _, b in sub)
        dt = np.int16 if nmax + mmax < 30000 else np.int32
        A, B = np.full((P, max(nmax, 1)), 254, dtype=np.uint8), np.full((P, max(mmax, 1)), 255, dtype=np.uint8)
        n, m = np.array([len(a) for a, _ in sub]), np.array([len(b) for _, b in sub])
        for p, (a, b) in enumerate(sub):
            A[p, :len(a)] = np.frombuffer(a, dtype=np.uint8)
            B[p, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        B = B[:, :mmax]
        idx = np.arange(mmax + 1, dtype=dt)
        prev = np.tile(idx, (P, 1))
        out = np.where(n == 0, m, -1).astype(np.int64)
        rows = np.arange(P)
        t = np.empty((P, mmax + 1), dtype=dt)
        for i in range(1, nmax + 1):
            t[:, 0] = i
            np.minimum(prev[:, 1:] + dt(1), prev[:, :-1] + (B != A[:, i - 1:i]), out=t[:, 1:])
            t -= idx
            np.minimum.accumulate(t, axis=1, out=prev)                  # D[i][j] = min_k (t[k] + j - k): the horizontal gaps
            prev += idx
            done = n == i
            if done.any():
                out[done] = prev[rows[done], m[done]]
        for p, v in zip(sel, out):
            result[p] = int(v)
    return result


def lev_matrix(seqs, cap=None):
    """U x U int32 matrix of lev, capped (the output of ltr_edit_distances for one group)."""
    U = len(seqs)
    ij = [(i, j) for i in range(U) for j in range(i + 1, U)]
    d = np.zeros((U, U), dtype=np.int32)
    big = [(i, j) for i, j in ij if max(len(seqs[i]), len(seqs[j])) > 2000]
    small = [(i, j) for i, j in ij if max(len(seqs[i]), len(seqs[j])) <= 2000]
    for (i, j), v in zip(small, lev_batch([(seqs[i], seqs[j]) for i, j in small])):
        d[i, j] = d[j, i] = v
    for i, j in big:
        d[i, j] = d[j, i] = lev(seqs[i], seqs[j])
    return d if cap is None else np.minimum(d, cap).astype(np.int32)


def needleman_wunsch(cent_seq, read_seq, T):
    """:201-234, cell by cell: the score the reference returns."""
    n, m = len(cent_seq), len(read_seq)
    if abs(n - m) > T:                                              # :203-206
        return T + 1
    dp = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        dp[i][0] = i
    for j in range(m + 1):
        dp[0][j] = j
    for i in range(1, n + 1):
        min_score_per_row = 1000                                    # :221
        for j in range(1, m + 1):
            S = 0 if cent_seq[i - 1] == read_seq[j - 1] else 1
            dp[i][j] = min(dp[i - 1][j] + 1, min(dp[i][j - 1] + 1, dp[i - 1][j - 1] + S))
            if dp[i][j] + abs((n - m) - (i - j)) < min_score_per_row:
                min_score_per_row = dp[i][j] + abs((n - m) - (i - j))
        if min_score_per_row > T:                                   # :227-230
            return T + 1
    return dp[n][m]


def nw_score(a, b, T, d):
    """needleman_wunsch(a, b, T) for T <= 700 from d = min(lev(a, b), 701): the distance when it is < T, else something >= T; with an
    empty SECOND argument and a non-empty first the reference's inner loop never runs and it answers T + 1."""
    if len(b) == 0 and len(a) > 0:
        return T + 1
    return int(d) if d < T else T + 1


def _order(s):
    return (len(s), s)                                              # orderByLengthAndSequence


class _Dist:
    def __init__(self, seqs, dist):
        self.at = {s: i for i, s in enumerate(seqs)}
        self.d = np.asarray(dist)

    def __call__(self, a, b):
        return int(self.d[self.at[a], self.at[b]])


def greedy_clustering(seqs, clusters, threshold, D):
    """:237-268.  seqs in the reference's order; clusters: dict centroid -> members (filled)."""
    centroids = [seqs[0]]
    clusters.setdefault(seqs[0], []).append(seqs[0])
    for i in range(1, len(seqs)):
        min_score, min_cntr = 2 ** 31 - 1, -1
        for j in range(len(centroids)):
            T = threshold
            score = nw_score(seqs[i], centroids[j], T, D(seqs[i], centroids[j]))
            if score < T and score < min_score:
                min_cntr, min_score = j, score
        if min_cntr != -1:
            clusters[centroids[min_cntr]].append(seqs[i])
        else:
            centroids.append(seqs[i])
            if len(centroids) > 15:                                 # :261
                return False
            clusters.setdefault(seqs[i], []).append(seqs[i])
    return True


def merge_clusters(new_centroids, clusters, threshold, D):
    """:271-293, quirks included: j starts at 1, a merged-away cluster is skipped, (centroid i, centroid j) argument order."""
    updated = False
    for i in range(len(new_centroids)):
        T = threshold
        for j in range(1, len(new_centroids)):
            if i != j and new_centroids[i] in clusters and new_centroids[j] in clusters:
                score = nw_score(new_centroids[i], new_centroids[j], T, D(new_centroids[i], new_centroids[j]))
                if score < T:
                    updated = True
                    clusters[new_centroids[i]].extend(list(clusters[new_centroids[j]]))
                    del clusters[new_centroids[j]]
    return updated


def medoid(members, counts, D):
    """Stands in for poa (:427): the member with the smallest count-weighted sum of distances, ties to the earlier in
    length-then-sequence order."""
    return min(members, key=lambda x: (sum(counts[y] * D(x, y) for y in members), _order(x)))


def cluster(seqs, counts, dist, candidates=(), trace=None):
    """:399-470 for one sample.  seqs: its unique unplaced sequences (bytes, any order), counts[i] reads each, dist the U x U matrix
    capped at 701; trace: a list that receives ("too many centroids", T) / ("merge", T) events.  Returns what _lib.cluster_sequences returns: dict(threshold, clusters=[dict(centroid, members, counted, new_allele)])."""
    if not seqs:
        return dict(threshold=-1, clusters=[])
    D = _Dist(seqs, dist)
    cnt = {s: int(c) for s, c in zip(seqs, counts)}
    ignored = sum(cnt.values())
    unique = sorted(seqs)                                           # the keys of the std::map, :400-402
    unique = [unique[0]] + sorted(unique[1:], key=_order)           # :403
    for t in LADDER:
        clusters = {}
        if not greedy_clustering(unique, clusters, t, D):
            if trace is not None:
                trace.append(("too many centroids", t))
            continue
        not_converged = True
        while not_converged:                                        # :422-440
            updated, new_centroids = {}, []
            for key in sorted(clusters):
                consensus = medoid(clusters[key], cnt, D)
                if consensus not in new_centroids:
                    new_centroids.append(consensus)
                    updated[consensus] = list(clusters[key])
                else:
                    updated[consensus].extend(clusters[key])
            new_centroids = [new_centroids[0]] + sorted(new_centroids[1:], key=_order)      # :437
            not_converged = merge_clusters(new_centroids, updated, t, D)
            if not_converged and trace is not None:
                trace.append(("merge", t))
            clusters = updated
        new_seqs_added, rows = 0, []
        for key in sorted(clusters):                                # :448-462
            sum_per_cluster = sum(cnt[s] for s in clusters[key])
            counted = sum_per_cluster > min(int(ignored * 0.10), 10)
            if counted:
                new_seqs_added += sum_per_cluster
            rows.append(dict(centroid=D.at[key], members=[D.at[s] for s in clusters[key]], counted=counted,
                             new_allele=counted and key not in candidates))
        if new_seqs_added >= int(0.80 * ignored):                   # :463
            return dict(threshold=t, clusters=rows)
    return dict(threshold=-1, clusters=[])


def noisy_copy(rng, seq, err):
    """A read of seq with substitutions, 1-base insertions and 1-base deletions, err in total per base."""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    r = rng.random(len(s))
    out = []
    for c, x in zip(s, r):
        if x < err / 3:
            continue
        if x < 2 * err / 3:
            out.append(int(BASES[(int(np.searchsorted(BASES, c)) + int(rng.integers(1, 4))) % 4]) if c in BASES else int(c))
        else:
            out.append(int(c))
        if x >= 1.0 - err / 3:
            out.append(int(BASES[rng.integers(0, 4)]))
    return bytes(out)


def unique_counts(seqs):
    """(unique sequences in std::map order, their counts)."""
    c = {}
    for s in seqs:
        c[s] = c.get(s, 0) + 1
    keys = sorted(c)
    return keys, [c[k] for k in keys]


def build_haplotype_clustered(op, left_alns, n_samples, region_start, region_stop, period, chrom_seq, chrom_seq_start, chrom_len, indel_flank_len=5,
                              dist_fn=None):
    """op.build_haplotype (oracle/ltr_oracle_prep.py, unchanged) with the clustering step where the reference has it: op hands its candidates
    (:373, sorted :475) to its `trim`; there, per sample with ignored > 0.25 * reads (:392) in order (:398), `cluster` runs against the
    candidates so far (:457-458) and the new centroids join them, flagged inexact; the list is sorted again (:475) and goes on to op's trim.
    Returns op's dict + inexact (per allele of the repeat block) + cluster_threshold (per sample: T, -1, or 0 = not needed)."""
    dist_fn = dist_fn or (lambda seqs: lev_matrix(seqs, CAP))
    real_trim = op.trim
    state = dict(inexact=None, thr=[0] * n_samples)

    def trim_with_clustering(ideal_min_length, left_pad, right_pad, rs, re, sequences):
        gen = [a for a in left_alns if a.get("use_for_hap_generation", True)]
        per_sample = [[] for _ in range(n_samples)]
        for a in gen:
            s = op.extract_sequence(a, rs, re)
            if s is not None:
                per_sample[a["sample"]].append(s)
        exact = list(sequences)
        groups = []
        for i in range(n_samples):                                  # :376-395, all samples against the exact candidates
            missing = [s for s in per_sample[i] if s not in exact]
            if len(missing) > len(per_sample[i]) * 0.25:
                groups.append((i, missing))
        flags = {s: 0 for s in sequences}
        sequences = list(sequences)
        for i, missing in groups:
            keys, counts = unique_counts([s.encode("latin-1") for s in missing])
            res = cluster(keys, counts, dist_fn(keys), [s.encode("latin-1") for s in sequences])
            state["thr"][i] = res["threshold"]
            for c in res["clusters"]:
                if c["new_allele"]:
                    s = keys[c["centroid"]].decode("latin-1")
                    sequences.append(s)
                    flags[s] = 1
        sequences = [sequences[0]] + sorted(sequences[1:], key=_order)
        state["inexact"] = [flags[s] for s in sequences]
        return real_trim(ideal_min_length, left_pad, right_pad, rs, re, sequences)

    op.trim = trim_with_clustering
    try:
        out = op.build_haplotype(left_alns, n_samples, region_start, region_stop, period, chrom_seq, chrom_seq_start, chrom_len, indel_flank_len)
    finally:
        op.trim = real_trim
    out["inexact"] = state["inexact"] if out["blocks"] is not None else None
    out["cluster_threshold"] = state["thr"] if state["inexact"] is not None else [0] * n_samples
    return out
