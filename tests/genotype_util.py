"""Shared by test_prune_blocks.py / test_gpu_plan_genotype.py: synthetic loci for ltr_plan_genotype, a Python restatement of
Haplotype::next() (Haplotype.cpp:123-196), and the prune-and-re-genotype chain written out with (a) the oracle's functions
and (b) the library's existing one-locus entry points."""
import numpy as np

import oracle_lib as ol
from longtr_amd import _abi, _lib, synth


def gray_counts(n_options):
    """Allele index per block of every haplotype in Haplotype::next() order (forward direction): at step counter -> counter + 1 the
    LAST block whose factor (the product of the option counts before it) divides counter + 1 moves one step in its direction, and
    turns round when it arrives at either end."""
    nb = len(n_options)
    factors, ncombs = [], 1
    for n in n_options:
        factors.append(ncombs)
        ncombs *= n
    counts, dirs, out = [0] * nb, [1] * nb, []
    for counter in range(ncombs):
        out.append(tuple(counts))
        if counter == ncombs - 1:
            break
        index = max(j for j in range(nb) if (counter + 1) % factors[j] == 0)
        counts[index] += dirs[index]
        if counts[index] == 0 or counts[index] == n_options[index] - 1:
            dirs[index] = -dirs[index]
    return out


def gray_seqs(blocks):
    return [b"".join(blocks[b]["alleles"][k] for b, k in enumerate(c)) for c in gray_counts([len(b["alleles"]) for b in blocks])]


def remove_alleles(blocks, removed):
    """HapBlock::remove_alleles on a list of block dicts; removed[b] = allele indices of block b."""
    return [dict(b, alleles=[a for i, a in enumerate(b["alleles"]) if i not in set(removed[k])]) for k, b in enumerate(blocks)]


def make_case(seed, n_loci=220, reads=(4, 40)):
    """Loci for one plan: H from 2 up, 1-6 samples (some without reads), some loci with a second multi-allelic block (the left
    flank with one substituted base), some reads far longer than the haplotypes (scores of -700, below the -600 clamp), some samples filtered, random phasing priors."""
    rng = np.random.default_rng(seed)
    loci = []
    for i in range(n_loci):
        nall = int(rng.integers(2, 8)) if i % 2 else int(rng.integers(2, 4))
        R = int(rng.integers(reads[0], reads[1]))
        n_true = nall if rng.random() < 0.75 else min(int(rng.integers(1, 4)), nall)
        L = synth.synth_locus(rng, int(rng.integers(10, 120)), int(rng.integers(1, 7)), nall, R, sub_rate=0.002, indel_rate=0.001,
                              true_alleles=rng.choice(nall, size=n_true, replace=False))
        blocks = L.blocks()
        if i % 4 == 1:                                           # second multi-allelic block: a base the trimmed reads cover
            f = bytearray(blocks[0]["alleles"][0])
            f[32] = ord("A") if f[32] != ord("A") else ord("C")
            blocks[0]["alleles"] = [blocks[0]["alleles"][0], bytes(f)]
        trimmed = list(L.trimmed_reads)
        if i % 7 == 3:
            for k in range(min(2, R)):
                trimmed[int(rng.integers(0, R))] = synth._rand_seq(rng, 1000).tobytes()        # |n - m| > 600: HapAligner.cpp:249-252
        S = int(rng.integers(1, 7))
        lab = rng.integers(0, S, size=R).astype(np.int32)
        hp = rng.integers(0, 3, size=R)
        p1 = np.where(hp == 1, -1e-6, np.where(hp == 2, -1000.0, -rng.random(R) * 0.01))
        p2 = np.where(hp == 2, -1e-6, np.where(hp == 1, -1000.0, -rng.random(R) * 0.01))
        filt = (rng.random(S) < 0.15).astype(np.uint8)
        pools, pidx = synth.pool_reads(trimmed)
        loci.append(dict(blocks=blocks, haps=gray_seqs(blocks), pools=pools, pool_index=np.asarray(pidx, dtype=np.int32), S=S, lab=lab,
                         p1=p1, p2=p2, filt=filt, haploid=False))
    return loci


def pack(loci):
    """(PackedBatch, arguments of Plan.posteriors / Plan.genotype)."""
    batch = _abi.PackedBatch([(L["pools"], L["haps"]) for L in loci])
    lro = np.zeros(len(loci) + 1, dtype=np.int64)
    lro[1:] = np.cumsum([len(L["lab"]) for L in loci])
    cat = lambda k: np.concatenate([np.asarray(L[k]) for L in loci])
    return batch, dict(locus_read_off=lro, pool_index=cat("pool_index"), log_p1=cat("p1"), log_p2=cat("p2"), sample_label=cat("lab"),
                       n_samples=np.asarray([L["S"] for L in loci], dtype=np.int32))


def chain(L, M, posteriors, unused, haps_to_alleles, remap, remap_ll, haploid=False, prune=True, first=None):
    """posteriors -> unused alleles per block -> pruned blocks -> haplotype remap -> column remap -> posteriors, for one locus
    with per-read matrix M [R x H], out of the five functions given (the oracle's or the library's).  first: the first
    posteriors when they come from elsewhere (Plan.posteriors): dict(post, sample_total_ll, gts)."""
    S, blocks = L["S"], L["blocks"]
    if first is None:
        first = posteriors(M, L["p1"], L["p2"], L["lab"], S, haploid)
    else:
        first = dict(first, clamped_ll=np.where(M < -600.0, -600.0, M))      # genotyper.cpp:57-58
    H = M.shape[1]
    aligned = np.zeros(S, dtype=np.uint8)
    if L.get("seeds") is None:
        aligned[np.unique(L["lab"])] = 1                         # every read of an unmasked plan has a seed position: samples with a read
    else:                                                        # seed_positions_[read] >= 0, seq_stutter_genotyper.cpp:262-266
        aligned[np.unique(L["lab"][np.asarray(L["seeds"])[L["pool_index"]] >= 0])] = 1
    removed = [unused(first["gts"], haps_to_alleles(blocks, b), len(blk["alleles"]), aligned, L["filt"]) if len(blk["alleles"]) > 1 else []
               for b, blk in enumerate(blocks)]
    out = dict(first=first, removed=removed)
    if not prune or not any(removed):
        out.update(blocks=blocks, post=first["post"], sample_total_ll=first["sample_total_ll"], gts=first["gts"], read_ll=first["clamped_ll"],
                   new_to_old=np.arange(H, dtype=np.int32), allele_mapping=np.arange(H, dtype=np.int32), removed=removed if prune else [[] for _ in blocks])
        return out
    new_blocks = remove_alleles(blocks, removed)
    mapping, _ = remap(blocks, new_blocks)
    Hn = int(np.prod([len(b["alleles"]) for b in new_blocks]))
    second = posteriors(remap_ll(M, mapping, Hn), L["p1"], L["p2"], L["lab"], S, haploid)
    n2o = np.full(Hn, -1, dtype=np.int32)
    for j, k in enumerate(mapping):
        if k >= 0:
            n2o[k] = j
    out.update(blocks=new_blocks, post=second["post"], sample_total_ll=second["sample_total_ll"], gts=second["gts"], read_ll=second["clamped_ll"],
               new_to_old=n2o, allele_mapping=np.asarray(mapping, dtype=np.int32))
    return out


def oracle_chain(L, M, haploid=False, prune=True):
    def remap_ll(M, mapping, Hn):
        new = np.full((M.shape[0], Hn), -100000.0)
        for j, k in enumerate(mapping):
            if k >= 0:
                new[:, k] = M[:, j]
        return new
    return chain(L, M, lambda *a: ol.oracle_posteriors(a[0], a[1], a[2], a[3], a[4], haploid=a[5]), ol.oracle_unused_alleles,
                 ol.oracle_haps_to_alleles, ol.oracle_remap_haplotypes, remap_ll, haploid, prune)


def product_chain(ctx, L, M, first, haploid=False, prune=True):
    """The same out of the library's existing entry points (what a caller had to write before ltr_plan_genotype): first = the
    locus' part of Plan.posteriors."""
    return chain(L, M, lambda *a: ctx.posteriors(a[0], a[1], a[2], a[3], a[4], haploid=a[5]), _lib.unused_alleles, _lib.haps_to_alleles,
                 _lib.remap_haplotypes, _lib.remap_aln_probs, haploid, prune, first=first)


def near_tie(L, post, eps=1e-6):
    """Some sample WITH reads whose best and second-best diplotype lie within eps (a sample without reads holds the priors alone:
    its ties are exact on every implementation and resolve to the first maximum everywhere)."""
    for s in np.unique(L["lab"]):
        flat = np.sort(post[s].ravel())
        if flat.size > 1 and flat[-1] - flat[-2] < eps:
            return True
    return False


def per_read(batch, ll, l, L):
    """The scatter of seq_stutter_genotyper.cpp:526-538: pool rows -> read rows."""
    return batch.locus_matrix(ll, l)[L["pool_index"]]


def prune_stats(loci, chains):
    """(share of loci that lose an allele, share that lose none, loci that lose alleles in two blocks)."""
    lose = [sum(1 for r in c["removed"] if r) for c in chains]
    n = float(len(loci))
    return sum(1 for k in lose if k) / n, sum(1 for k in lose if not k) / n, sum(1 for k in lose if k >= 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
