"""-m gpu: ltr_build_haplotypes_consensus -- ltr_build_haplotypes_clustered with the partial-order-alignment consensus of a cluster where the
reference calls poa (HaplotypeGenerator.cpp:427; ltr_poa.hip) -- against the Python composition: oracle/ltr_oracle_prep.py's exact part as it is,
then tests/poa_util.py.  Twelve synthetic loci in one call under a lowered memory cap, and one two-allele locus through the whole chain: the
consensus alleles are called, and each is closer to its true allele than the medoid the older entry point gives for the same reads."""
import numpy as np
import pytest

import cluster_util as cu
import poa_util as pu
from longtr_amd import _lib
from test_gpu_cluster_haplotypes import _genotype, noisy_locus, op

pytestmark = pytest.mark.gpu
_CACHE = {}
CAP = 1 << 20          # 15 reads of 600 bases: 450 KB of graph arrays, and the rows of the second alignment, 601 x 601 x 2 = 722 KB, do not fit the rest

# name -> generator arguments.  What each is there for is asserted in test_the_loci_are_what_they_are_for from the restatement's trace.
LOCI = [
    ("exact, two alleles", dict(seed=1, ref_len=60, alleles=(60, 75), n_reads=20, err=0.0)),
    ("exact, three alleles", dict(seed=3, ref_len=120, alleles=(120, 100, 150), n_reads=30, err=0.0, n_samples=2)),
    ("noisy 3 %, one sample", dict(seed=4, ref_len=600, alleles=(300, 360), n_reads=30, err=0.03)),
    ("noisy 3 %, two samples", dict(seed=5, ref_len=200, alleles=(150, 180), n_reads=48, err=0.03, n_samples=2)),
    ("noisy 8 %, one sample", dict(seed=6, ref_len=330, alleles=(300, 360), n_reads=30, err=0.08)),
    ("noisy 4 %, one allele of 250", dict(seed=17, ref_len=300, alleles=(250,), n_reads=24, err=0.04)),
    ("one sample exact, one noisy", dict(seed=9, ref_len=200, alleles=(180, 220), n_reads=48, err=0.0, n_samples=2, sample_err=(0.0, 0.04))),
    ("fails: too near to the chromosome end", dict(seed=10, ref_len=60, alleles=(60, 75), n_reads=12, err=0.0)),
    ("noisy 5 %, one allele of 60", dict(seed=12, ref_len=80, alleles=(60,), n_reads=24, err=0.05)),
    ("two clusters, one consensus", dict(seed=33, ref_len=440, alleles=(400,), n_reads=28, err=0.02)),
    ("second sample finds the first's allele", dict(seed=22, ref_len=200, alleles=(150,), n_reads=40, err=0.03, n_samples=2)),
    ("over the cap", dict(seed=21, ref_len=700, alleles=(600, 660), n_reads=30, err=0.03)),
]


def _case(ctx):
    if "case" in _CACHE:
        return _CACHE["case"]
    data, sets, want, args, traces = [], [], [], [], []
    for name, kw in LOCI:
        d = noisy_locus(**kw)
        if "fails" in name:
            d["chrom_len"] = d["region"][1] + 20
        rs0, re0 = d["region"]
        rs = _lib.ReadSet(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])
        left = op.left_align_reads(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])[0]
        trace = []
        want.append(pu.build_haplotype_consensus(op, left, d["n_samples"], rs0, re0, d["period"], d["chrom"], d["chrom_start"], d["chrom_len"],
                                                 cap_bytes=CAP, trace=trace))
        data.append(d); sets.append(rs); traces.append(trace)
        args.append(dict(rs=rs, region_start=rs0, region_stop=re0, period=d["period"], chrom_seq_start=d["chrom_start"], chrom_len=d["chrom_len"]))
    try:
        ctx.set_debug("poa_group_cap_bytes", CAP)
        got = ctx.build_haplotypes_consensus(args)
    finally:
        ctx.set_debug("poa_group_cap_bytes", 0)
    _CACHE["case"] = dict(data=data, sets=sets, want=want, got=got, traces=traces, args=args)
    return _CACHE["case"]


def test_twelve_loci_equal_the_composition(gpu_ctx):
    c = _case(gpu_ctx)
    assert len(c["got"]) == 12
    for (name, kw), got, want in zip(LOCI, c["got"], c["want"]):
        print(name, want["cluster_threshold"], want["consensus_rounds"], want["medoid_kept"], want["inexact"], want["failure"])
        assert got == want, name


def test_the_loci_are_what_they_are_for(gpu_ctx):
    c = _case(gpu_ctx)
    names = [n for n, _ in LOCI]
    at = lambda n: names.index(n)
    events = lambda n: [e[0] for e in c["traces"][at(n)]]
    assert "merge" in events("noisy 3 %, one sample")                                   # the refinement merges greedy clusters
    assert "too many centroids" in events("noisy 8 %, one sample")                      # a threshold fails on its 16th centroid
    assert "same consensus" in events("two clusters, one consensus")                    # :432-434
    assert ("already a candidate", 1, "inexact") in c["traces"][at("second sample finds the first's allele")]
    second = c["got"][at("second sample finds the first's allele")]
    assert second["cluster_threshold"] == [20, 20] and sum(second["inexact"]) == 1
    for name, got in zip(names, c["got"]):                      # the medoid is kept over the cap, there only, and counted
        kept = sum(got["medoid_kept"])
        assert (kept > 0) == (name == "over the cap"), (name, got["medoid_kept"])
    over = c["got"][at("over the cap")]
    assert over["cluster_threshold"][0] > 0 and sum(over["inexact"]) == 2 and over["medoid_kept"] == [2]
    fails = c["got"][at("fails: too near to the chromosome end")]
    assert fails["blocks"] is None and fails["inexact"] is None and fails["consensus_rounds"] == [0]
    assert all(r > 0 for r in c["got"][at("noisy 3 %, two samples")]["consensus_rounds"])


def test_exact_only_loci_are_what_build_haplotype_gives(gpu_ctx):
    c = _case(gpu_ctx)
    n = 0
    for (name, kw), d, rs, got in zip(LOCI, c["data"], c["sets"], c["got"]):
        if got["samples_needing_clustering"] != 0:
            continue
        one = rs.build_haplotype(d["region"][0], d["region"][1], d["period"], d["chrom_start"], d["chrom_len"])
        assert {k: got[k] for k in one} == one, name
        assert got["cluster_threshold"] == [0] * d["n_samples"] and got["consensus_rounds"] == [0] * d["n_samples"]
        assert got["inexact"] is None or not any(got["inexact"])
        n += 1
    assert n >= 3


def test_the_library_cap_keeps_no_medoid_and_the_older_entry_point_is_unchanged(gpu_ctx):
    """Without the lowered cap the 600-base locus gets its consensus; ltr_build_haplotypes_clustered still answers with medoids."""
    c = _case(gpu_ctx)
    k = [n for n, _ in LOCI].index("over the cap")
    d = c["data"][k]
    got = gpu_ctx.build_haplotypes_consensus([c["args"][k]])[0]
    rs0, re0 = d["region"]
    left = op.left_align_reads(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])[0]
    assert got == pu.build_haplotype_consensus(op, left, d["n_samples"], rs0, re0, d["period"], d["chrom"], d["chrom_start"], d["chrom_len"])
    assert got["medoid_kept"] == [0]
    medoid = gpu_ctx.build_haplotypes_clustered([c["args"][k]])[0]
    flagged = [a for a, f in zip(medoid["blocks"][1]["alleles"], medoid["inexact"]) if f]
    assert len(flagged) == 2 and "consensus_rounds" not in medoid
    assert [a for a, f in zip(c["got"][k]["blocks"][1]["alleles"], c["got"][k]["inexact"]) if f] == flagged   # what the cap keeps are these medoids


def test_noisy_locus_end_to_end_consensus_is_closer_than_the_medoid(gpu_ctx):
    """Two alleles of 300 / 360 bases, 30 reads at 3 % error, no read equal to another, through build_haplotypes_consensus ->
    ltr_calc_hap_aln_probs -> ltr_ll_genotype: the called alleles have the true lengths, and each consensus allele is strictly closer to
    its true allele than the medoid ltr_build_haplotypes_clustered gives for the same reads (seed fixed on the CPU with the restatements:
    unit-cost distances 0 and 0 against the medoids' 5 and 4)."""
    c = _case(gpu_ctx)
    k = [n for n, _ in LOCI].index("noisy 3 %, one sample")
    d, rs, got = c["data"][k], c["sets"][k], c["got"][k]
    medoid = gpu_ctx.build_haplotypes_clustered([c["args"][k]])[0]
    b = got["blocks"]
    assert (b[1]["start"], b[1]["end"]) == (medoid["blocks"][1]["start"], medoid["blocks"][1]["end"])
    lo, hi = b[1]["start"] - d["chrom_start"], b[1]["end"] - d["chrom_start"]
    chrom = d["chrom"]
    motif_start = d["region"][0] - d["chrom_start"]
    period = d["period"]
    unit = chrom[motif_start:motif_start + period]

    def true_allele(L):                                         # the block's bases with a repeat of L bases in the reference repeat's place
        rep = (unit * (L // period + 2))[:L]
        full = chrom[:motif_start] + rep + chrom[motif_start + d["ref_len"]:]
        return full[lo:len(full) - (len(chrom) - hi)]

    cons = sorted((a for a, f in zip(b[1]["alleles"], got["inexact"]) if f), key=len)
    meds = sorted((a for a, f in zip(medoid["blocks"][1]["alleles"], medoid["inexact"]) if f), key=len)
    assert len(cons) == 2 and len(meds) == 2
    for L, a, m in zip(sorted(d["alleles"]), cons, meds):
        t = true_allele(L)
        print(L, len(t), len(a), len(m), cu.lev(a, t), cu.lev(m, t))
        assert len(a) == len(t)
        assert cu.lev(a, t) < cu.lev(m, t)
    gt, line, final = _genotype(gpu_ctx, d, rs, b, got["inexact"])
    assert gt == cons
    assert "INEXACT_ALLELE=1,1" in line.split("\t")[7].split(";")
