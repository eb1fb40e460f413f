"""The checker of the consensus step (HaplotypeGenerator::poa, reference src/SeqAlignment/HaplotypeGenerator.cpp:167-199, called at :427),
restated in Python.  This is partial-order alignment by the PUBLISHED method (Lee, Grasso & Sharlow 2002, heaviest-bundle consensus) with the
scoring the reference hands to spoa (:169: global, linear gap, match +1, mismatch -1, gap -1) and every tie rule fixed;
it is not spoa's bytes.  The kernel (longtr_amd/csrc/ltr_poa.hip) is held to this file.

  poa_consensus              one cluster -> its consensus
  poa_consensus_capped       ... with the memory rule of ltr_poa_consensus: (consensus, status), status 1 = over the per-group cap
  cluster_consensus          cluster_util.cluster with the consensus where the reference calls poa (:427), distances computed where needed
  build_haplotype_consensus  oracle/ltr_oracle_prep.py's build_haplotype with cluster_consensus per sample between :373 and :475

Everything is an integer or a byte string: the tests compare for equality."""
import numpy as np

import cluster_util as cu

MAX_MEMBERS = 30                                                    # :171


def used_members(seqs):
    """The members the alignment takes, in order: empty ones dropped; of more than 30 those at floor(k * n / 30), k = 0 .. 29 (the
    reference draws 30 at random, :182-192)."""
    seqs = [bytes(s) for s in seqs if len(s) > 0]
    n = len(seqs)
    if n > MAX_MEMBERS:
        seqs = [seqs[(k * n) // MAX_MEMBERS] for k in range(MAX_MEMBERS)]
    return seqs


class Graph:
    def __init__(self):
        self.letter, self.aligned, self.pred, self.succ = [], [], [], []      # pred[v]: {predecessor: weight}; succ[v]: set
        self.cells = 0                                                        # DP cells of all alignments so far (nodes x columns)

    def new_node(self, c):
        self.letter.append(c); self.aligned.append([]); self.pred.append({}); self.succ.append(set())
        return len(self.letter) - 1

    def order(self):
        """Kahn's algorithm, always the smallest ready node id."""
        n = len(self.letter)
        deg = [len(p) for p in self.pred]
        ready = sorted(v for v in range(n) if deg[v] == 0)
        out = []
        import heapq
        heapq.heapify(ready)
        while ready:
            v = heapq.heappop(ready)
            out.append(v)
            for w in self.succ[v]:
                deg[w] -= 1
                if deg[w] == 0:
                    heapq.heappush(ready, w)
        assert len(out) == n
        return out

    def scores(self, s):
        """H as a dict node -> numpy row of len(s) + 1 (key -1: the virtual row)."""
        m = len(s)
        sb = np.frombuffer(s, dtype=np.uint8)
        idx = np.arange(m + 1, dtype=np.int64)
        H = {-1: -idx}
        for v in self.order():
            preds = sorted(self.pred[v]) or [-1]
            sc = np.where(sb == self.letter[v], 1, -1)
            t = np.empty(m + 1, dtype=np.int64)
            t[0] = max(H[p][0] for p in preds) - 1
            diag = np.max([H[p][:-1] for p in preds], axis=0) + sc
            vert = np.max([H[p][1:] for p in preds], axis=0) - 1
            t[1:] = np.maximum(diag, vert)
            H[v] = np.maximum.accumulate(t + idx) - idx             # H[v][j] = max_k (t[k] - (j - k)): the horizontal gaps
        self.cells += len(self.letter) * m
        return H

    def end_node(self, H, m):
        ends = [v for v in range(len(self.letter)) if not self.succ[v]]
        return min(ends, key=lambda v: (-int(H[v][m]), v))

    def align(self, s):
        """Per base of s the node it is aligned to, or -1."""
        m = len(s)
        H = self.scores(s)
        v, j = self.end_node(H, m), m
        aln = [-1] * m
        while v != -1 or j > 0:
            if v == -1:                                             # the virtual row: horizontal moves only
                j -= 1
                continue
            preds = sorted(self.pred[v]) or [-1]
            h = int(H[v][j])
            step = None
            if j > 0:
                sc = 1 if s[j - 1] == self.letter[v] else -1
                for p in preds:
                    if int(H[p][j - 1]) + sc == h:
                        step = ("d", p)
                        break
            if step is None:
                for p in preds:
                    if int(H[p][j]) - 1 == h:
                        step = ("v", p)
                        break
            if step is None:
                assert j > 0 and int(H[v][j - 1]) - 1 == h
                j -= 1
            elif step[0] == "d":
                aln[j - 1] = v
                v, j = step[1], j - 1
            else:
                v = step[1]
        return aln

    def add(self, s, aln):
        prev = -1
        for c, a in zip(s, aln):
            if a == -1:
                cur = self.new_node(c)
            elif self.letter[a] == c:
                cur = a
            else:
                same = [x for x in self.aligned[a] if self.letter[x] == c]
                if same:
                    cur = same[0]
                else:
                    cur = self.new_node(c)
                    column = [a] + self.aligned[a]
                    for x in column:
                        self.aligned[x].append(cur)
                    self.aligned[cur] = column
            if prev != -1:
                self.pred[cur][prev] = self.pred[cur].get(prev, 0) + 1
                self.succ[prev].add(cur)
            prev = cur

    def consensus(self):
        n = len(self.letter)
        score, back = [0] * n, [-1] * n
        for v in self.order():
            if self.pred[v]:
                p = min(self.pred[v], key=lambda p: (-self.pred[v][p], -score[p], p))
                score[v], back[v] = score[p] + self.pred[v][p], p
        ends = [v for v in range(n) if not self.succ[v]]
        v = min(ends, key=lambda v: (-score[v], v))
        out = []
        while v != -1:
            out.append(self.letter[v])
            v = back[v]
        return bytes(reversed(out))


LDS_GRAPH_BYTES = 16 << 10
GROUP_CAP_BYTES = 512 << 20


def poa_graph(seqs, cap_bytes=None):
    """The graph of the members used (None when fewer than two are left).  cap_bytes: the memory rule of ltr_poa_consensus
    (include/ltr_gpu.h), restated -- "over" is returned for a group over the per-group cap.  B bases in all, longest member L: graph arrays
    of 48 B + 4 ceil(B / 32) + 4 L + B rounded up to 16 bytes, the sum rounded up to 256, in LDS up to 16 KB and in the group's scratch otherwise;
    before every alignment the rows, (nodes + 1) x (m + 1) cells of 2 bytes (4 when B + L > 32767), must fit what the cap leaves."""
    use = used_members(seqs)
    if len(use) < 2:
        return None
    rows = None
    if cap_bytes is not None:
        B, L = sum(len(s) for s in use), max(len(s) for s in use)
        graph = 48 * B + 4 * ((B + 31) // 32) + 4 * L + ((B + 15) // 16) * 16
        graph = ((graph + 255) // 256) * 256
        lds = graph <= LDS_GRAPH_BYTES
        if not lds and graph > cap_bytes:
            return "over"
        cell = 4 if B + L > 32767 else 2
        rows = min((B + 1) * (L + 1) * cell, cap_bytes - (0 if lds else graph))
    g = Graph()
    g.add(use[0], [-1] * len(use[0]))
    for s in use[1:]:
        if rows is not None and (len(g.letter) + 1) * (len(s) + 1) * cell > rows:
            return "over"
        g.add(s, g.align(s))
    return g


def poa_consensus(seqs):
    """The consensus of one cluster: members in the order the cluster's vector holds them, every member weighs 1."""
    return poa_consensus_capped(seqs, None)[0]


def poa_consensus_capped(seqs, cap_bytes=GROUP_CAP_BYTES):
    """(consensus, status) as ltr_poa_consensus gives them: status 1 and an empty consensus for a group over the cap."""
    use = used_members(seqs)
    if len(use) < 2:
        return (use[0] if use else b""), 0
    g = poa_graph(seqs, cap_bytes)
    return (b"", 1) if g == "over" else (g.consensus(), 0)


class _AnyDist:
    """Distances between any two strings, computed where needed (capped at 701) and remembered."""

    def __init__(self):
        self.memo = {}

    def __call__(self, a, b):
        if a == b:
            return 0
        k = (a, b) if a <= b else (b, a)
        if k not in self.memo:
            self.memo[k] = min(cu.lev(a, b), cu.CAP)
        return self.memo[k]


def cluster_consensus(seqs, counts, dist, candidates=(), trace=None, cap_bytes=GROUP_CAP_BYTES):
    """cluster_util.cluster (:399-470 for one sample) with the consensus of a cluster's members where the reference calls poa (:427).  The
    greedy step reads the sample's matrix; a consensus is not one of the sequences, so the merge takes distances computed where needed.
    A cluster over the memory cap (poa_consensus_capped) keeps its medoid.  rounds: passes of the refinement loop (:422) over all thresholds tried;
    medoid_kept: final clusters whose centre is a medoid for the cap's sake.
    Returns dict(threshold, rounds, medoid_kept, clusters=[dict(centroid=bytes, members, counted, new_allele)])."""
    if not seqs:
        return dict(threshold=-1, rounds=0, medoid_kept=0, clusters=[])
    D = cu._Dist(seqs, dist)
    A = _AnyDist()
    cnt = {s: int(c) for s, c in zip(seqs, counts)}
    memo = {}

    def consensus_fn(members):
        k = tuple(members)
        if k not in memo:
            c, status = poa_consensus_capped(members, cap_bytes)
            memo[k] = (cu.medoid(members, cnt, D), True) if status else (c, False)
        return memo[k]

    ignored = sum(cnt.values())
    unique = sorted(seqs)
    unique = [unique[0]] + sorted(unique[1:], key=cu._order)
    rounds = 0
    for t in cu.LADDER:
        clusters = {}
        if not cu.greedy_clustering(unique, clusters, t, D):
            if trace is not None:
                trace.append(("too many centroids", t))
            continue
        not_converged = True
        kept = {}
        while not_converged:
            rounds += 1
            updated, new_centroids, kept = {}, [], {}
            for key in sorted(clusters):
                consensus, medoid_kept = consensus_fn(clusters[key])
                if consensus not in new_centroids:
                    new_centroids.append(consensus)
                    updated[consensus] = list(clusters[key])
                    kept[consensus] = medoid_kept
                else:
                    updated[consensus].extend(clusters[key])
                    if trace is not None:
                        trace.append(("same consensus", t))
            new_centroids = [new_centroids[0]] + sorted(new_centroids[1:], key=cu._order)
            not_converged = cu.merge_clusters(new_centroids, updated, t, A)
            if not_converged and trace is not None:
                trace.append(("merge", t))
            clusters = updated
        new_seqs_added, rows = 0, []
        for key in sorted(clusters):
            sum_per_cluster = sum(cnt[s] for s in clusters[key])
            counted = sum_per_cluster > min(int(ignored * 0.10), 10)
            if counted:
                new_seqs_added += sum_per_cluster
            rows.append(dict(centroid=key, members=[D.at[s] for s in clusters[key]], counted=counted, new_allele=counted and key not in candidates))
        if new_seqs_added >= int(0.80 * ignored):
            return dict(threshold=t, rounds=rounds, medoid_kept=sum(1 for key in clusters if kept.get(key)), clusters=rows)
    return dict(threshold=-1, rounds=rounds, medoid_kept=0, clusters=[])


def build_haplotype_consensus(op, left_alns, n_samples, region_start, region_stop, period, chrom_seq, chrom_seq_start, chrom_len, indel_flank_len=5,
                              cap_bytes=GROUP_CAP_BYTES, trace=None):
    """cluster_util.build_haplotype_clustered with cluster_consensus per sample.  Returns op's dict + inexact + cluster_threshold +
    consensus_rounds and medoid_kept (per sample)."""
    real_trim = op.trim
    state = dict(inexact=None, thr=[0] * n_samples, rounds=[0] * n_samples, kept=[0] * n_samples)

    def trim_with_clustering(ideal_min_length, left_pad, right_pad, rs, re, sequences):
        gen = [a for a in left_alns if a.get("use_for_hap_generation", True)]
        per_sample = [[] for _ in range(n_samples)]
        for a in gen:
            s = op.extract_sequence(a, rs, re)
            if s is not None:
                per_sample[a["sample"]].append(s)
        exact = list(sequences)
        groups = []
        for i in range(n_samples):
            missing = [s for s in per_sample[i] if s not in exact]
            if len(missing) > len(per_sample[i]) * 0.25:
                groups.append((i, missing))
        flags = {s: 0 for s in sequences}
        sequences = list(sequences)
        for i, missing in groups:
            keys, counts = cu.unique_counts([s.encode("latin-1") for s in missing])
            res = cluster_consensus(keys, counts, cu.lev_matrix(keys, cu.CAP), [s.encode("latin-1") for s in sequences], trace=trace,
                                    cap_bytes=cap_bytes)
            state["thr"][i], state["rounds"][i], state["kept"][i] = res["threshold"], res["rounds"], res["medoid_kept"]
            for c in res["clusters"]:
                s = c["centroid"].decode("latin-1")
                if c["new_allele"]:
                    sequences.append(s)
                    flags[s] = 1
                elif c["counted"] and trace is not None:
                    trace.append(("already a candidate", i, "inexact" if flags[s] else "exact"))
        sequences = [sequences[0]] + sorted(sequences[1:], key=cu._order)
        state["inexact"] = [flags[s] for s in sequences]
        return real_trim(ideal_min_length, left_pad, right_pad, rs, re, sequences)

    op.trim = trim_with_clustering
    try:
        out = op.build_haplotype(left_alns, n_samples, region_start, region_stop, period, chrom_seq, chrom_seq_start, chrom_len, indel_flank_len)
    finally:
        op.trim = real_trim
    done = state["inexact"] is not None
    out["inexact"] = state["inexact"] if out["blocks"] is not None else None
    out["cluster_threshold"] = state["thr"] if done else [0] * n_samples
    out["consensus_rounds"] = state["rounds"] if done else [0] * n_samples
    out["medoid_kept"] = state["kept"] if done else [0] * n_samples
    return out
