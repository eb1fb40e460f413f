"""-m gpu: longtr_amd.call.genotype_regions with phased_snps on seven loci of the bundled trio, set up as tests/test_gpu_call.py does.

No phased SNP VCF of the trio is bundled, so one is built from the reads' own bases: within 1000 bp of each locus and outside its
15-bp padding, every position at which the reads of HG002 or HG004 split between two bases (each on at least 4 reads, together
on 90 % of them) becomes a record with a phased heterozygous call for that sample.  HG003 is left out of the VCF, and the VCF has a
column of a sample no BAM holds.  The consumers of the priors are the existing posterior and fields kernels: checked is that the
priors reach GT, PQ, DSNP and PSNP through them -- every record equals its per-locus composition, with the priors taken from the
Python restatement (tests/snp_phasing_util.py) rather than from the library."""
import collections
import gzip
import os

import numpy as np
import pytest

import snp_phasing_util as U
import test_gpu_call as G
from longtr_amd import _abi, _filter, _lib, _snp, call

LOCI = ("Human_STR_211", "Human_STR_213", "Human_STR_222", "Human_STR_228", "Human_STR_237", "Human_STR_239", "Human_STR_244")
VCF_SAMPLES = ["HG002", "NA00001", "HG004"]
TOLERANCE = 1e-10                                                # mathops.cpp:12: a read counts in DSNP when |log_p1 - log_p2| exceeds it


def pile_up(read, lo, hi, out):
    """Count the read's base at every reference position of [lo, hi) it covers with an M, = or X."""
    pos, at = read["pos"], 0
    for op, n in read["cigar"]:
        if op in "M=X":
            for k in range(max(lo - pos, 0), min(hi - pos, n)):
                out[pos + k][read["seq"][at + k]] += 1
            pos, at = pos + n, at + n
        elif op in "DN":
            pos += n
        elif op in "IS":
            at += n


def split_sites(bam, rgs, reg):
    """{pos0: {sample: (most common base, second base)}} of the sites of a locus at which a sample's passing reads split."""
    recs = bam.fetch(reg["chrom"], max(0, reg["start"] - 1000), reg["stop"] + 1000, tags=("RG", "XA", "HP"))
    fr = _filter.filter_reads(recs, reg["start"], reg["stop"], read_groups=rgs)
    lo, hi = max(reg["start"] - 1000, 0), reg["stop"] + 1000
    sites = collections.defaultdict(dict)
    for s, name in enumerate(fr["samples"]):
        if name not in VCF_SAMPLES:
            continue
        counts = collections.defaultdict(collections.Counter)
        for i, k, _ in fr["passing"]:
            if k == s:
                pile_up(recs[i], lo, hi, counts)
        depth = sum(1 for _, k, _ in fr["passing"] if k == s)
        for pos, c in counts.items():
            top = c.most_common(2)
            if reg["start"] - 15 <= pos + 1 <= reg["stop"] + 15 or len(top) < 2:
                continue
            if top[1][1] >= 4 and top[0][1] + top[1][1] >= 0.9 * depth:
                sites[pos][name] = (top[0][0], top[1][0])
    return sites


def write_vcf(path, records):
    w = _lib.VcfWriter(path)
    w.header("##fileformat=VCFv4.2\n" + U.HEADER + "\t" + "\t".join(VCF_SAMPLES) + "\n")
    for chrom, pos, text in records:
        w.add_record(chrom, pos, text)
    w.close()
    _lib.vcf_index(path)
    with gzip.open(path, "rt") as fh:
        return [t.rstrip("\n") for t in fh if not t.startswith("#")]


@pytest.fixture(scope="module")
def seven(tmp_path_factory):
    """The seven loci, their reference windows, and two VCFs of the same sites: phased calls, and the same calls unphased."""
    d = tmp_path_factory.mktemp("snp_call")
    bed = str(d / "all.bed")
    G.rt.convert_bed(os.path.join(G.DATA, "test_regions_hg38.bed"), bed)
    regions = [r for r in _lib.read_regions(bed, order=True)[0] if r["name"] in LOCI]
    assert len(regions) == len(LOCI)
    bam = _lib.Bam(G.BAMS, merge_by_position=False)
    phased, unphased = [], []
    try:
        rgs = bam.read_groups()
        for reg in regions:
            sites = split_sites(bam, rgs, reg)
            # one call inside the padding too: the record filter removes it, in the library and in the restatement alike
            sites[reg["start"]] = {"HG004": ("A", "C")}
            for pos in sorted(sites):
                ref, alt = next(iter(sites[pos].values()))
                calls = []
                for name in VCF_SAMPLES:
                    pair = sites[pos].get(name)
                    het = pair is not None and set(pair) == {ref, alt}
                    calls.append(("0|1" if pair[0] == ref else "1|0") if het else "0|0" if pos % 3 else "1|1")
                head = [reg["chrom"], str(pos + 1), ".", ref, alt, ".", "PASS", ".", "GT"]
                phased.append((reg["chrom"], pos + 1, "\t".join(head + calls)))
                unphased.append((reg["chrom"], pos + 1, "\t".join(head + [c.replace("|", "/") if c[0] != c[2] else c for c in calls])))
    finally:
        bam.close()
    lines = write_vcf(str(d / "phased.vcf.gz"), phased)
    write_vcf(str(d / "unphased.vcf.gz"), unphased)
    return dict(dir=d, bed=regions, regions=regions, ref=G.ReadsReference(regions), vcf=str(d / "phased.vcf.gz"), empty_vcf=str(d / "unphased.vcf.gz"),
                header=U.HEADER + "\t" + "\t".join(VCF_SAMPLES), lines=lines)


@pytest.fixture(scope="module")
def plain(gpu_ctx, seven):
    report, out = G.run(gpu_ctx, seven, "plain", chunk_loci=None)
    return report, out, G.data_lines(out)


@pytest.fixture(scope="module")
def with_snps(gpu_ctx, seven):
    report, out = G.run(gpu_ctx, seven, "with_snps", chunk_loci=None, phased_snps=seven["vcf"])
    print(f"phased_snps on {len(seven['regions'])} loci: snp_seconds={report['timing']['snp_seconds']:.4f} wall_seconds={report['timing']['wall_seconds']:.4f}")
    return report, out, G.data_lines(out)


def restated_priors(seven, reg, raw, sample_names, tables):
    """(log_p1, log_p2 of the raw reads, the restatement's set) from the VCF's lines, without the library."""
    lo, hi = (0 if reg["start"] <= 1000 else reg["start"] - 1001), reg["stop"] + 1000
    mine = [t for t in seven["lines"] if t.split("\t")[0] == reg["chrom"] and lo <= int(t.split("\t")[1]) - 1 < hi]
    ref_set = U.build_set(seven["header"], mine, [(reg["start"], reg["stop"])], 15)
    p1, p2 = np.zeros(len(raw)), np.zeros(len(raw))
    for k, name in enumerate(sample_names):
        idx = [j for j, r in enumerate(raw) if r["sample"] == k]
        p1[idx], p2[idx], _ = U.priors(ref_set, ref_set["index"].get(name, -1), [raw[j] for j in idx], tables)
    return p1, p2, ref_set


def compose(ctx, seven, bam, rgs, reg, tables):
    """The record of one region through the entry points that existed before the driver (the composer of tests/test_gpu_call.py), with
    the restated priors of the raw reads carried to the left-aligned reads."""
    ref = seven["ref"]
    recs = bam.fetch(reg["chrom"], max(0, reg["start"] - 1000), reg["stop"] + 1000, tags=("RG", "XA", "HP"))
    fr = _filter.filter_reads(recs, reg["start"], reg["stop"], read_groups=rgs)
    chrom_len = ref.length(reg["chrom"])
    lo, hi = max(reg["start"] - call.REF_PAD, 0), min(reg["stop"] + call.REF_PAD, chrom_len)
    window = ref.fetch(reg["chrom"], lo, hi - 1).encode()
    raw = [dict(pos=recs[i]["pos"], end_pos=recs[i]["end_pos"], bases=recs[i]["seq"].encode(), cigar=recs[i]["cigar"], sample=s, hp=int(recs[i].get("HP", 0)),
                quals=recs[i]["qual"].encode("latin-1"), reverse=int(bool(recs[i]["flag"] & 16)), use_for_hap_generation=int(pf))
           for i, s, pf in fr["passing"]]
    raw_p1, raw_p2, ref_set = restated_priors(seven, reg, raw, fr["samples"], tables)
    S = len(fr["samples"])
    rs = _lib.ReadSet(raw, S, reg["start"], reg["stop"], window, lo)
    try:
        hb = rs.build_haplotype(reg["start"], reg["stop"], reg["period"], lo, chrom_len)
        assert hb["blocks"] is not None, hb["failure"]
        reads = rs.reads
        alns = [dict(start=r["start"], stop=r["stop"], seq=r["seq"], cigar=r["cigar"]) for r in reads]
        sample = [r["sample"] for r in reads]
        source = [r["source"] for r in reads]
        p1, p2 = raw_p1[source], raw_p2[source]
        (ll, seeds), = ctx.calc_hap_aln_probs([(hb["blocks"], alns, None)])
        with ctx.genotype_ll([ll], [seeds], [hb["blocks"]], [0, len(reads)], p1, p2, sample, [S], prune=True, fields={}, locus_haploid=[False]) as result:
            g = result.locus(0)
            none = np.zeros(0)
            pv = _abi.PackedVcfLocus(dict(
                chrom=reg["chrom"], region_start=reg["start"], region_stop=reg["stop"], name=reg["name"], motif=reg["motif"],
                period_str=reg["period_str"], chrom_seq=window, chrom_seq_start=lo, blocks=g["blocks"], block=1,
                inexact_allele=np.zeros(len(g["blocks"][1]["alleles"]), dtype=np.uint8), log_aln_probs=none, log_p1=p1, log_p2=p2,
                sample_label=np.asarray(sample, dtype=np.int32), alns=alns, aln_deleted=[r["deleted"] for r in reads],
                log_sample_posteriors=none, sample_total_ll=none, best_haplotypes=np.zeros(0, dtype=np.int32), n_p1s=rs.n_p1s, n_p2s=rs.n_p2s,
                sample_names=fr["samples"], haploid=False, out_sample_names=sorted(G.SAMPLES)))
            lines, _ = result.vcf_records([pv], None)
        differ = np.abs(p1 - p2) > TOLERANCE
        per_sample = {name: (int((differ & (np.asarray(sample) == k)).sum()), int(((p1 > p2) & differ & (np.asarray(sample) == k)).sum()))
                      for k, name in enumerate(fr["samples"])}
        info = dict(n_valid_snps=ref_set["n_valid"], samples_in_vcf=sum(1 for n in fr["samples"] if n in ref_set["index"]),
                    phased_reads=int((raw_p1 != raw_p2).sum()), phased_samples=len({raw[j]["sample"] for j in np.flatnonzero(raw_p1 != raw_p2)}))
        return lines[0], per_sample, info
    finally:
        rs.close()


def sample_fields(line, columns):
    """{sample: {FORMAT key: value}} of the columns of a record that hold a call."""
    c = line.split("\t")
    keys = c[8].split(":")
    return {name: dict(zip(keys, col.split(":"))) for name, col in zip(columns, c[9:]) if col != "."}


@pytest.mark.gpu
def test_a_vcf_without_phased_het_calls_changes_no_record(gpu_ctx, seven, plain):
    report, out = G.run(gpu_ctx, seven, "empty", chunk_loci=None, phased_snps=seven["empty_vcf"])
    lines, _ = G.data_lines(out)
    assert lines == plain[2][0] and len(lines) == len(LOCI)
    assert [t for t in open(out).read().splitlines() if not t.startswith("#")] == [t for t in open(plain[1]).read().splitlines() if not t.startswith("#")]
    for e in report["loci"]:
        assert e["snp_info"]["phased_reads"] == e["snp_info"]["phased_samples"] == 0
        assert e["snp_info"]["samples_in_vcf"] == 2 and e["snp_info"]["n_valid_snps"] >= 0
    assert sum(e["snp_info"]["n_valid_snps"] for e in report["loci"]) > 0        # the sites were read and counted; none is a phased het
    assert report["counters"]["snp_match"] == report["counters"]["snp_mismatch"] == 0
    assert all("snp_info" not in e for e in plain[0]["loci"]) and "snp_seconds" not in plain[0]["timing"]
    assert {k: v for k, v in report["counters"].items() if not k.startswith("snp_")} == plain[0]["counters"]


@pytest.mark.gpu
def test_every_record_equals_its_composition_with_restated_priors(gpu_ctx, seven, plain, with_snps):
    report, out, (lines, _) = with_snps
    tables = _snp.quality_tables()
    columns = report["columns"]
    assert columns == sorted(G.SAMPLES) and len(lines) == len(LOCI) and report["timing"]["snp_seconds"] > 0
    bam = _lib.Bam(G.BAMS, merge_by_position=False)
    two_sided = changed = swapped = 0
    try:
        rgs = bam.read_groups()
        by_key = {(r["chrom"], r["start"] + 1, r["stop"]): r for r in seven["regions"]}
        for e in report["loci"]:
            assert e["status"] == "ok", e
            line, per_sample, info = compose(gpu_ctx, seven, bam, rgs, by_key[G.key_of(e)], tables)
            assert line == lines[G.key_of(e)], e["name"]
            assert e["snp_info"] == info, e["name"]
            got, before = sample_fields(line, columns), sample_fields(plain[2][0][G.key_of(e)], columns)
            for name, f in got.items():
                n_snp, n_one = per_sample[name]
                print(e["name"], name, "GT", f["GT"], "PQ", f["PQ"], "DSNP", f["DSNP"], "PSNP", f["PSNP"], "| unphased PQ", before[name]["PQ"])
                assert int(f["DSNP"]) == n_snp and f["PSNP"] == f"{n_one}|{n_snp - n_one}", (e["name"], name)
                assert before[name]["DSNP"] == "0" and before[name]["PSNP"] == "0|0"
                if name == "HG003":                              # not in the VCF: no prior
                    assert n_snp == 0
                two_sided += min(n_one, n_snp - n_one) > 0
                gt, gt_before = [int(x) for x in f["GT"].split("|")], [int(x) for x in before[name]["GT"].split("|")]
                assert gt_before[0] <= gt_before[1]              # without priors: row-major order
                swapped += gt[0] > gt[1]
                changed += f["PQ"] != before[name]["PQ"] or f["PSNP"] != before[name]["PSNP"]
    finally:
        bam.close()
    assert two_sided >= 1 and changed >= 1                       # reads on both haplotypes of a sample, and a call that moved
    assert swapped >= 1                                          # a het GT in the order of its SNPs' haplotypes, which row-major order never gives
    assert report["counters"]["snp_match"] > 0 and report["counters"]["snp_mismatch"] >= 0
    assert {k: v for k, v in report["counters"].items() if not k.startswith("snp_")} == plain[0]["counters"]


@pytest.mark.gpu
@pytest.mark.parametrize("name, options", [("one_locus_chunks", dict(chunk_loci=1)), ("no_overlap", dict(chunk_loci=None, overlap=False))])
def test_chunking_and_overlap_change_nothing_with_snps(gpu_ctx, seven, with_snps, name, options):
    report, out = G.run(gpu_ctx, seven, name, phased_snps=seven["vcf"], **options)
    assert open(out, "rb").read() == open(with_snps[1], "rb").read()
    assert G.strip_timing(report) == G.strip_timing(with_snps[0])
    assert report["timing"]["chunks"] == (len(LOCI) if options["chunk_loci"] == 1 else 1)
