"""Shared by test_gpu_sample_ploidy.py: small loci with random per-read log-likelihood matrices (no DP: ltr_ll_genotype* takes
them as they are), the ploidy patterns, the decoding of a result and the stitching of two uniform results into what a call with
a ploidy per (locus, sample) must give.  Unit (l, s) depends on the other samples of its locus only through pruning, so the
oracle is the library's own per-locus-ploidy calls; every comparison is == on bits, integers or text."""
import numpy as np

import genotype_util as gt
import vcf_fields_util as vu
from longtr_amd import _abi, _lib
from test_gpu_ll_genotype import WANT
from test_gpu_plan_fields import ALL_OPT, _describe
from test_gpu_plan_genotype import _big_locus

PER_SAMPLE = ("log_phased", "log_unphased", "hap_log_phased", "hap_log_unphased", "gl_diffs", "n_aligned", "n_snp", "n_s1", "n_s2")
TEN = "GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF"
SIX = "GT:GB:Q:DP:DFLANKINDEL:GLDIFF"
OPT = dict(output_pls=1, **ALL_OPT)                              # GL, PL, PHASEDGL, HQ / PHQ, FILTER


def make_loci(n_loci, seed, samples=None):
    """Locus l: S = 1 + l % 3 samples (or `samples`); l % 5 = 0..3: one multi-allelic block of V = 1..4 alleles, 4: two blocks,
    H = 2 x 3 = 6.  Sample s has (0, 1, 7)[(l + s) % 3] reads, interleaved; a third of the reads carry phasing priors
    (log_p1 != log_p2); a read prefers one allele of its sample's pair; a tenth of the scores lie below the -600 clamp."""
    rng = np.random.default_rng(seed)
    loci = []
    for l in range(n_loci):
        S, kind = (1 + l % 3) if samples is None else samples, l % 5
        L = _big_locus(rng, max(kind + 1, 2) if kind < 4 else 3, 4, S, kind == 4)
        if kind == 0:                                            # V = 1: a single allele everywhere
            L["blocks"][1]["alleles"] = L["blocks"][1]["alleles"][:1]
        L["haps"] = gt.gray_seqs(L["blocks"])
        H = len(L["haps"])
        lab = np.concatenate([np.full((0, 1, 7)[(l + s) % 3], s, dtype=np.int32) for s in range(S)] + [np.zeros(0, dtype=np.int32)])
        lab = rng.permutation(lab).astype(np.int32)
        R = len(lab)
        pair = rng.integers(0, H, size=(S, 2))
        want = pair[lab, rng.integers(0, 2, size=R)] if R else np.zeros(0, dtype=np.int64)
        M = -np.abs(rng.normal(0.0, 2.0, size=(R, H))) - 25.0 * rng.random((R, H)) * (np.arange(H)[None, :] != want[:, None])
        M[rng.random((R, H)) < 0.1] = -700.0
        hp = rng.integers(0, 3, size=R) * (rng.random(R) < 0.5)
        p1 = np.where(hp == 1, -1e-6, np.where(hp == 2, -1000.0, -0.005))
        p2 = np.where(hp == 2, -1e-6, np.where(hp == 1, -1000.0, -0.005))
        L.update(S=S, lab=lab, p1=p1.astype(np.float64), p2=p2.astype(np.float64), filt=np.zeros(S, dtype=np.uint8), M=np.ascontiguousarray(M),
                 pools=None, pool_index=None)
        loci.append(L)
    return loci


def case_of(loci):
    lro = np.zeros(len(loci) + 1, dtype=np.int64)
    lro[1:] = np.cumsum([len(L["lab"]) for L in loci])
    cat = lambda k, dt: np.concatenate([np.asarray(L[k], dtype=dt) for L in loci] + [np.zeros(0, dtype=dt)])
    return dict(loci=loci, blocks=[L["blocks"] for L in loci], mats=[L["M"] if len(L["lab"]) else None for L in loci],
                largs=dict(locus_read_off=lro, log_p1=cat("p1", np.float64), log_p2=cat("p2", np.float64), sample_label=cat("lab", np.int32),
                           n_samples=np.asarray([L["S"] for L in loci], dtype=np.int32)))


def pattern(loci, k):
    """Flags of run k: sample s of locus l is haploid when bit s of (k + l) % 8 is set -- over k = 0..7 a locus sees all 2^S patterns."""
    return [np.asarray([((k + l) % 8 >> s) & 1 for s in range(L["S"])], dtype=np.uint8) for l, L in enumerate(loci)]


def run(ctx, case, prune, blocks=None, mats=None, records=True, **ploidy):
    """One ltr_ll_genotype* call with every field asked for, decoded: per locus locus(), fields(), haploid(), the record text."""
    blocks = case["blocks"] if blocks is None else blocks
    with ctx.genotype_ll(case["mats"] if mats is None else mats, None, blocks, prune=bool(prune), want_read_ll=True, fields=WANT,
                         **ploidy, **case["largs"]) as res:
        n = res.n_loci
        out = dict(loci=[res.locus(l) for l in range(n)], fields=[res.fields(l) for l in range(n)], haploid=[res.haploid(l) for l in range(n)],
                   sample_haploid=[res.sample_haploid(l) for l in range(n)])
        if records:
            rng = np.random.default_rng(7)
            packed = [_abi.PackedVcfLocus(_describe(l, L, out["loci"][l], False, rng)) for l, L in enumerate(case["loci"])]
            out["lines"], out["pos"] = res.vcf_records(packed, _abi.vcf_options(**OPT))
    return out


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(vu.bits(a), vu.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))


def check_stitched(got, refs, flags, loci, what=""):
    """got: a result made with the flags; refs[p]: the uniform result of ploidy p on the SAME blocks and matrices.  Every number of
    unit (l, s) equals that of refs[flags[l][s]], with ==; the shape of a locus follows ltr_genotype_result_haploid."""
    for l, L in enumerate(loci):
        f, S = flags[l], L["S"]
        g, gf = got["loci"][l], got["fields"][l]
        assert np.array_equal(got["sample_haploid"][l], f) and np.array_equal(g["sample_haploid"], f) and np.array_equal(gf["sample_haploid"], f), (what, l)
        all_hap = bool(S) and bool(f.all())
        assert got["haploid"][l] == int(all_hap), (what, l)
        V = gf["V"]
        assert (gf["n_gl"], gf["n_pgl"]) == ((V, V) if all_hap else (V * (V + 1) // 2, V * V)), (what, l)
        for p in (0, 1):                                         # what no ploidy touches
            r = refs[p]["loci"][l]
            assert g["n_haps"] == r["n_haps"] and g["removed"] == r["removed"] and same(g["new_to_old"], r["new_to_old"]), (what, l)
            assert same(g["read_ll"], r["read_ll"]) and [b["alleles"] for b in g["blocks"]] == [b["alleles"] for b in r["blocks"]], (what, l)
        for s in range(S):
            p = int(f[s])
            r, rf = refs[p]["loci"][l], refs[p]["fields"][l]
            where = (what, l, s, p)
            assert same(g["post"][s], r["post"][s]) and same(g["sample_total_ll"][s], r["sample_total_ll"][s]) and same(g["gts"][s], r["gts"][s]), where
            assert same(gf["best_gts"][s], rf["best_gts"][s]), where
            for k in PER_SAMPLE:
                assert same(gf[k][s], rf[k][s]), where + (k,)
            mine = L["lab"] == s
            assert same(gf["read_allele"][mine], rf["read_allele"][mine]), where
            if p == 0 or all_hap:                                # a diploid row, or a locus in the haploid shape: the whole row
                for k in ("gls", "pls", "phased_gls"):
                    assert same(gf[k][s], rf[k][s]), where + (k,)
            else:                                                # a haploid sample of a mixed locus: V values, then 0; no phased genotypes
                for k in ("gls", "pls"):
                    assert same(gf[k][s][:V], rf[k][s]) and not gf[k][s][V:].any(), where + (k,)
                    assert gf[k][s][V:].tobytes() == bytes(gf[k][s][V:].nbytes), where + (k,)      # +0.0, not -0.0
                assert gf["phased_gls"][s].tobytes() == bytes(gf["phased_gls"][s].nbytes), where


def expected_after_pruning(ctx, case, flags, uniform0):
    """What prune = 1 must give for the flags, out of existing calls only: the stitched best pairs of the two uniform prune-0
    runs -> ltr_unused_alleles per block -> the pruned block lists -> ltr_remap_haplotypes -> ltr_remap_aln_probs -> the two uniform
    prune-0 runs on those.  Returns (refs of check_stitched, removed per locus and block)."""
    loci = case["loci"]
    blocks2, mats2, removed = [], [], []
    for l, L in enumerate(loci):
        gts = np.asarray([uniform0[int(flags[l][s])]["loci"][l]["gts"][s] for s in range(L["S"])], dtype=np.int32).reshape(L["S"], 2)
        aligned = np.zeros(L["S"], dtype=np.uint8)
        aligned[np.unique(L["lab"])] = 1
        rem = [_lib.unused_alleles(gts, _lib.haps_to_alleles(L["blocks"], b), len(blk["alleles"]), aligned, L["filt"]) if len(blk["alleles"]) > 1 else []
               for b, blk in enumerate(L["blocks"])]
        if len(L["haps"]) == 1:
            rem = [[] for _ in L["blocks"]]
        new = L["blocks"]
        for b, r in enumerate(rem):
            if r:
                new = _lib.prune_hap_blocks(new, b, r)
        assert [b["alleles"] for b in new] == [b["alleles"] for b in gt.remove_alleles(L["blocks"], rem)]
        mapping, _ = _lib.remap_haplotypes(L["blocks"], new)
        Hn = int(np.prod([len(b["alleles"]) for b in new]))
        blocks2.append(new)
        mats2.append(_lib.remap_aln_probs(L["M"], mapping, Hn) if len(L["lab"]) else None)
        removed.append(rem)
    refs = {p: run(ctx, case, 0, blocks=blocks2, mats=mats2, records=False, haploid=bool(p)) for p in (0, 1)}
    for p in (0, 1):                                             # in the terms of the ORIGINAL haplotypes, as a pruning call reports them
        for l, L in enumerate(loci):
            mapping, _ = _lib.remap_haplotypes(L["blocks"], blocks2[l])
            n2o = np.full(refs[p]["loci"][l]["n_haps"], -1, dtype=np.int32)
            for j, k in enumerate(mapping):
                if k >= 0:
                    n2o[k] = j
            refs[p]["loci"][l].update(removed=removed[l], new_to_old=n2o)
    return refs, removed
