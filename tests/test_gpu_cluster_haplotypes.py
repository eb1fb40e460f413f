"""-m gpu: ltr_build_haplotypes_clustered -- ltr_build_haplotype for many loci with the clustering step of gen_candidate_seqs
(HaplotypeGenerator.cpp:376-472; distances on the GPU, ltr_editdist.hip) -- against the Python composition: oracle/ltr_oracle_prep.py's
exact part as it is, then tests/cluster_util.py.  Twelve synthetic loci in one call, and one locus through the whole chain: with noisy
reads the clustered alleles are called, without the step only the reference allele is there to call."""
import importlib.util
import os

import numpy as np
import pytest

import cluster_util as cu
from longtr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ltr_oracle_prep", os.path.join(ROOT, "oracle", "ltr_oracle_prep.py"))
op = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(op)
_CACHE = {}


def noisy_locus(seed, ref_len, alleles, n_reads, err, n_samples=1, period=5, flank=700, unrelated=False, sample_err=None):
    """A chromosome window with a repeat of ref_len bases at its centre and whole reads of the given allele lengths (read i carries
    allele i % len(alleles), sample (i // len(alleles)) % n_samples), aligner-style 'M' CIGARs, substitutions and 1-base indels at rate
    err all along the read (sample_err: the rate per sample).  unrelated: every read carries an insertion of its own random bases."""
    rng = np.random.default_rng(seed)
    motif = synth._rand_seq(rng, period)
    longest = max(list(alleles) + [ref_len])
    rep = np.tile(motif, longest // period + 2)
    rep0 = rep[:ref_len]
    lflank, rflank = synth._rand_seq(rng, flank), synth._rand_seq(rng, flank)
    chrom = np.concatenate([lflank, rep0, rflank])
    chrom_start = 50000
    region = (chrom_start + flank, chrom_start + flank + ref_len)
    raw = []
    for i in range(n_reads):
        L = alleles[i % len(alleles)]
        sample = (i // len(alleles)) % n_samples
        lo, hi = int(rng.integers(150, 250)), int(rng.integers(150, 250))
        common = min(L, ref_len)
        pieces = [("ref", np.concatenate([lflank[lo:], rep0[:common]]))]
        if unrelated:
            pieces.append(("ins", synth._rand_seq(rng, int(rng.integers(1500, 2500)))))
        elif L > ref_len:
            pieces.append(("ins", rep[ref_len:L]))
        elif L < ref_len:
            pieces.append(("del", rep0[common:]))
        pieces.append(("ref", rflank[:flank - hi]))
        e = err if sample_err is None else sample_err[sample]
        aln = synth._build_read(rng, pieces, e / 2, e / 2, chrom_start + lo)
        cig = []
        for t, n in aln["cigar"]:
            t = "M" if t in "=X" else t
            if cig and cig[-1][0] == t:
                cig[-1] = (t, cig[-1][1] + n)
            else:
                cig.append((t, n))
        raw.append(dict(pos=aln["start"], end_pos=aln["stop"] + 1, bases=aln["seq"], cigar=cig, sample=sample, hp=0))
    return dict(chrom=chrom.tobytes(), chrom_start=chrom_start, chrom_len=chrom_start + len(chrom) + 1000, region=region, raw=raw, period=period,
                n_samples=n_samples, ref_len=ref_len, alleles=list(alleles))


# name -> (generator arguments, what the restatement must find: per-sample thresholds, number of inexact alleles)
LOCI = [
    ("exact, two alleles", dict(seed=1, ref_len=60, alleles=(60, 75), n_reads=20, err=0.0), ([0], 0)),
    ("exact, one allele shorter than the reference", dict(seed=2, ref_len=90, alleles=(70,), n_reads=16, err=0.0, n_samples=2), ([0, 0], 0)),
    ("exact, three alleles", dict(seed=3, ref_len=120, alleles=(120, 100, 150), n_reads=30, err=0.0, n_samples=2), ([0, 0], 0)),
    ("noisy 3 %, one sample", dict(seed=4, ref_len=600, alleles=(300, 360), n_reads=30, err=0.03), None),
    ("noisy 3 %, two samples", dict(seed=5, ref_len=330, alleles=(300, 360), n_reads=60, err=0.03, n_samples=2), None),
    ("noisy 8 %, one sample", dict(seed=6, ref_len=330, alleles=(300, 360), n_reads=30, err=0.08), None),
    ("noisy 8 %, two samples", dict(seed=7, ref_len=330, alleles=(300, 360), n_reads=60, err=0.08, n_samples=2), None),
    ("noisy 3 %, 1 kb", dict(seed=8, ref_len=1050, alleles=(1000, 1100), n_reads=30, err=0.03), None),
    ("one sample exact, one noisy", dict(seed=9, ref_len=200, alleles=(180, 220), n_reads=48, err=0.0, n_samples=2, sample_err=(0.0, 0.04)), None),
    ("fails: too near to the chromosome end", dict(seed=10, ref_len=60, alleles=(60, 75), n_reads=12, err=0.0), "fail"),
    ("clustering finds nothing", dict(seed=11, ref_len=60, alleles=(60,), n_reads=12, err=0.0, unrelated=True), ([-1], 0)),
    ("noisy 5 %, one allele of 60", dict(seed=12, ref_len=80, alleles=(60,), n_reads=24, err=0.05), None),
]


def _case(ctx):
    """The twelve loci built once for the module: library result, read sets, the composition's result."""
    if "case" in _CACHE:
        return _CACHE["case"]
    data, sets, want, args = [], [], [], []
    for name, kw, _ in LOCI:
        d = noisy_locus(**kw)
        if "fails" in name:
            d["chrom_len"] = d["region"][1] + 20                     # REF_FLANK_LEN + pad does not fit
        rs0, re0 = d["region"]
        rs = _lib.ReadSet(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])
        left = op.left_align_reads(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])[0]
        want.append(cu.build_haplotype_clustered(op, left, d["n_samples"], rs0, re0, d["period"], d["chrom"], d["chrom_start"], d["chrom_len"]))
        data.append(d)
        sets.append(rs)
        args.append(dict(rs=rs, region_start=rs0, region_stop=re0, period=d["period"], chrom_seq_start=d["chrom_start"], chrom_len=d["chrom_len"]))
    got = ctx.build_haplotypes_clustered(args)
    _CACHE["case"] = dict(data=data, sets=sets, want=want, got=got)
    return _CACHE["case"]


def _true_len(d, blocks, L):
    """Length of a true allele of L repeat bases inside the repeat block as it was trimmed."""
    return (blocks[1]["end"] - blocks[1]["start"]) + (L - d["ref_len"])


def test_twelve_loci_equal_the_composition(gpu_ctx):
    c = _case(gpu_ctx)
    assert len(c["got"]) == 12
    for (name, kw, expect), d, got, want in zip(LOCI, c["data"], c["got"], c["want"]):
        print(name, want["cluster_threshold"], want["inexact"], want["failure"], want["unplaced_reads"], want["samples_needing_clustering"])
        assert got == want, name
        if expect == "fail":
            assert got["blocks"] is None and got["failure"] == "Haplotype blocks are too near to the chromosome ends" and got["inexact"] is None
        elif expect is not None:
            assert got["cluster_threshold"] == expect[0] and sum(got["inexact"]) == expect[1], name
    names = [n for n, _, _ in LOCI]
    nothing = c["got"][names.index("clustering finds nothing")]
    assert nothing["samples_needing_clustering"] == 1 and nothing["unplaced_reads"] == 12 and len(nothing["blocks"][1]["alleles"]) == 1
    mixed = c["got"][names.index("one sample exact, one noisy")]
    assert mixed["cluster_threshold"][0] == 0 and mixed["cluster_threshold"][1] > 0 and mixed["samples_needing_clustering"] == 1


def test_exact_only_loci_are_what_build_haplotype_gives(gpu_ctx):
    c = _case(gpu_ctx)
    n = 0
    for (name, kw, _), d, rs, got in zip(LOCI, c["data"], c["sets"], c["got"]):
        if got["samples_needing_clustering"] != 0:
            continue
        one = rs.build_haplotype(d["region"][0], d["region"][1], d["period"], d["chrom_start"], d["chrom_len"])
        assert {k: got[k] for k in one} == one, name
        assert got["cluster_threshold"] == [0] * d["n_samples"] and (got["inexact"] is None or not any(got["inexact"]))
        n += 1
    assert n >= 4                                                    # the three exact loci and the failing one


def test_two_allele_loci_recover_the_alleles(gpu_ctx):
    c = _case(gpu_ctx)
    n = 0
    for (name, kw, _), d, got in zip(LOCI, c["data"], c["got"]):
        if not name.startswith("noisy") or len(d["alleles"]) != 2:
            continue
        b = got["blocks"]
        inexact = sorted(len(a) for a, f in zip(b[1]["alleles"], got["inexact"]) if f)
        print(name, got["cluster_threshold"], inexact, [_true_len(d, b, L) for L in d["alleles"]])
        assert all(t > 0 for t in got["cluster_threshold"]), name
        assert len(inexact) >= 2, name
        for L in d["alleles"]:                                      # each true allele has an inexact allele within 3 % of its length
            assert min(abs(x - _true_len(d, b, L)) for x in inexact) <= 0.03 * L, (name, L, inexact)
        n += 1
    assert n == 5


def _genotype(ctx, d, rs, blocks, inexact):
    """calc_hap_aln_probs -> ltr_ll_genotype (pruning, fields) -> records, for one locus: (GT as allele sequences, record, final blocks)."""
    reads = [r for r in rs.reads if not r["deleted"]]
    alns = [dict(start=r["start"], stop=r["stop"], seq=r["seq"], cigar=r["cigar"]) for r in reads]
    lab = np.asarray([r["sample"] for r in reads], dtype=np.int32)
    zero = np.zeros(len(reads))
    res = ctx.calc_hap_aln_probs([(blocks, alns, None)])
    with ctx.genotype_ll([res[0][0]], [res[0][1]], [blocks], [0, len(reads)], zero, zero, lab, [d["n_samples"]], prune=True, fields={}) as result:
        g = result.locus(0)
        keep = [f for k, f in enumerate(inexact) if k not in g["removed"][1]]      # the flags of the alleles pruning left
        pv = _abi.PackedVcfLocus(dict(
            chrom="chrT", region_start=d["region"][0], region_stop=d["region"][1], name="T1", motif="N" * d["period"], period_str=str(d["period"]),
            chrom_seq=d["chrom"], chrom_seq_start=d["chrom_start"], blocks=g["blocks"], block=1, inexact_allele=np.asarray(keep, dtype=np.uint8),
            log_aln_probs=np.zeros(0), log_p1=zero, log_p2=zero, sample_label=lab, alns=alns, log_sample_posteriors=np.zeros(0),
            sample_total_ll=np.zeros(0), best_haplotypes=np.zeros(0, dtype=np.int32), n_p1s=rs.n_p1s, n_p2s=rs.n_p2s,
            sample_names=[f"S{s}" for s in range(d["n_samples"])]))
        lines, _ = result.vcf_records([pv])
    fields = lines[0].split("\t")
    gt = fields[9].split(":")[0].replace("|", "/").split("/")
    alleles = g["blocks"][1]["alleles"]
    return sorted(alleles[int(x)] for x in gt), lines[0], g["blocks"]


def test_noisy_locus_end_to_end_calls_the_clustered_alleles(gpu_ctx):
    """What the step is for.  Two alleles of 300 / 360 bases, 30 reads at 3 % error, no read equal to another: with clustering the
    genotype is the two cluster centres and the record says INEXACT_ALLELE=1,1; through ltr_build_haplotype alone the reference allele
    is the only candidate and the only call.  (The reference allele of this locus has 600 bases.  A medoid is a read and carries that
    read's errors; with a reference allele of 330 bases, one 30-base gap away from either true allele, this test came out as one cluster
    centre and the reference allele: under the default model some ten scattered errors cost more than one long gap.  A clean consensus
    would not have lost there; the medoid deviation does, and DESIGN section 5 says so.)"""
    c = _case(gpu_ctx)
    k = [n for n, _, _ in LOCI].index("noisy 3 %, one sample")
    d, rs, got = c["data"][k], c["sets"][k], c["got"][k]
    flagged = sorted(a for a, f in zip(got["blocks"][1]["alleles"], got["inexact"]) if f)
    assert len(flagged) == 2
    gt, line, final = _genotype(gpu_ctx, d, rs, got["blocks"], got["inexact"])
    print(line[:300])
    assert gt == flagged
    assert "INEXACT_ALLELE=1,1" in line.split("\t")[7].split(";")
    assert sorted(len(a) for a in final[1]["alleles"][1:]) == sorted(len(a) for a in flagged)
    alone = rs.build_haplotype(d["region"][0], d["region"][1], d["period"], d["chrom_start"], d["chrom_len"])
    assert len(alone["blocks"][1]["alleles"]) == 1 and alone["samples_needing_clustering"] == 1 and alone["unplaced_reads"] == 30
    gt0, line0, _ = _genotype(gpu_ctx, d, rs, alone["blocks"], [0])
    assert gt0 == [alone["blocks"][1]["alleles"][0]] * 2 and line0.split("\t")[4] == "."
