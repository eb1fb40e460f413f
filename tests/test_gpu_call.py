"""-m gpu: longtr_amd.call.genotype_regions on the bundled trio (three HiFi BAMs, the 40 regions of the bundled BED, all on chr1).

hg38 is not bundled, so the reference is an object whose windows are rebuilt from the reads' '=' runs, as examples/real_reads_trio.py
does.  Under the reference's default filters every locus keeps 38 to 117 reads (one locus, 2916 bp long, is removed by --max-tr-len
before its reads are looked at), so min_reads stays at its default of 10.

Checked: the VCF does not depend on how the loci are cut into chunks or on the producer thread; every record equals the one built
locus by locus through the entry points that existed before the driver (ReadSet -> build_haplotype -> calc_hap_aln_probs of that
locus -> genotype_ll -> its one record); gated loci are reported and write nothing; the haploid, phased, consensus and panel paths
write the records their per-locus composition gives."""
import importlib.util
import os

import numpy as np
import pytest

from longtr_amd import _abi, _filter, _lib, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "bam")
SAMPLES = ["HG002", "HG003", "HG004"]
BAMS = [os.path.join(DATA, f"{s}_sample_reads.bam") for s in SAMPLES]
_spec = importlib.util.spec_from_file_location("real_reads_trio", os.path.join(ROOT, "examples", "real_reads_trio.py"))
rt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rt)


class ReadsReference:
    """fetch / length / contig_lines over windows rebuilt from the reads (rt.rebuild_reference), one per region."""

    path = "(no hg38 FASTA bundled: windows rebuilt from the reads' = runs)"

    def __init__(self, regions):
        bam = _lib.Bam(BAMS)
        self.lengths = dict(bam.refs())
        self.windows = {}
        for reg in regions:
            lo, hi = max(reg["start"] - call.REF_PAD, 0), min(reg["stop"] + call.REF_PAD, self.lengths[reg["chrom"]])
            recs = [r for r in bam.fetch(reg["chrom"], reg["start"], reg["stop"]) if r["mapq"] >= 20 and not (r["flag"] & 0x704)]
            self.windows[(reg["chrom"], lo, hi - 1)] = rt.rebuild_reference(recs, lo, hi).decode()
        bam.close()

    def fetch(self, chrom, start, end):
        return self.windows[(chrom, start, end)]

    def length(self, chrom):
        return self.lengths.get(chrom, -1)

    def contig_lines(self):
        return ""


def data_lines(path):
    """{(chrom, INFO START, INFO END): line} of a plain-text VCF, and its text."""
    text = open(path).read()
    out = {}
    for t in text.splitlines():
        if not t.startswith("#"):
            c = t.split("\t")
            info = dict(kv.split("=", 1) for kv in c[7].split(";") if "=" in kv)
            out[(c[0], int(info["START"]), int(info["END"]))] = t
    return out, text


def strip_timing(report):
    return {k: v for k, v in report.items() if k != "timing"}


@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    d = tmp_path_factory.mktemp("call")
    bed = str(d / "regions.bed")
    rt.convert_bed(os.path.join(DATA, "test_regions_hg38.bed"), bed)
    regions, _ = _lib.read_regions(bed, order=True)
    return dict(dir=d, bed=bed, regions=regions, ref=ReadsReference(regions))


def run(gpu_ctx, trio, name, **options):
    out = str(trio["dir"] / f"{name}.vcf")
    report = call.genotype_regions(gpu_ctx, BAMS, trio["ref"], trio["bed"], out, **options)
    assert report["error"] is None, report["error"]
    return report, out


@pytest.fixture(scope="module")
def base(gpu_ctx, trio):
    """The default run: every locus in one chunk, the producer thread on."""
    report, out = run(gpu_ctx, trio, "base", chunk_loci=None)
    return report, out, data_lines(out)


class Composer:
    """Per-locus composition with the entry points that existed before the driver.  The reads are the driver's own: the library's
    filter on the records of the region, fetched file by file, in the filter's output order."""

    def __init__(self, ctx, trio):
        self.ctx, self.trio = ctx, trio
        self.bam = _lib.Bam(BAMS, merge_by_position=False)
        self.rgs = self.bam.read_groups()
        self.columns = sorted(SAMPLES)

    def close(self):
        self.bam.close()

    def locus(self, reg, phased=False, haploid=False, alleles="exact", panel=None, fields=None, vopt=None):
        """(VCF line, fields image, failure text) of one region."""
        ctx, ref = self.ctx, self.trio["ref"]
        recs = self.bam.fetch(reg["chrom"], max(0, reg["start"] - 1000), reg["stop"] + 1000, tags=("RG", "XA", "HP"))
        fr = _filter.filter_reads(recs, reg["start"], reg["stop"], read_groups=self.rgs)
        chrom_len = ref.length(reg["chrom"])
        lo, hi = max(reg["start"] - call.REF_PAD, 0), min(reg["stop"] + call.REF_PAD, chrom_len)
        window = ref.fetch(reg["chrom"], lo, hi - 1).encode()
        raw = [dict(pos=recs[i]["pos"], end_pos=recs[i]["end_pos"], bases=recs[i]["seq"].encode(), cigar=recs[i]["cigar"], sample=s,
                    hp=int(recs[i].get("HP", 0)), quals=recs[i]["qual"].encode("latin-1"), reverse=int(bool(recs[i]["flag"] & 16)),
                    use_for_hap_generation=int(pf)) for i, s, pf in fr["passing"]]
        S = len(fr["samples"])
        rs = _lib.ReadSet(raw, S, reg["start"], reg["stop"], window, lo)
        try:
            inexact = None
            if panel is not None:
                rec = panel.alleles(reg["chrom"], reg["start"], reg["stop"])
                if rec is None:
                    return None, None, "no panel record"
                hb = rs.build_vcf_haplotype(rec[0], rec[1], reg["period"], lo, chrom_len)
            elif alleles == "consensus":
                hb = ctx.build_haplotypes_consensus([dict(rs=rs, region_start=reg["start"], region_stop=reg["stop"], period=reg["period"],
                                                          chrom_seq_start=lo, chrom_len=chrom_len)])[0]
                inexact = hb["inexact"]
            else:
                hb = rs.build_haplotype(reg["start"], reg["stop"], reg["period"], lo, chrom_len)
            if hb["blocks"] is None:
                return None, None, hb["failure"]
            reads = rs.reads
            alns = [dict(start=r["start"], stop=r["stop"], seq=r["seq"], cigar=r["cigar"]) for r in reads]
            sample = [r["sample"] for r in reads]
            if phased:
                p1, p2, _ = _lib.phasing_priors(sample, [raw[r["source"]]["hp"] if raw[r["source"]]["hp"] in (1, 2) else -1 for r in reads], S)
            else:
                p1, p2 = np.zeros(len(reads)), np.zeros(len(reads))
            (ll, seeds), = ctx.calc_hap_aln_probs([(hb["blocks"], alns, None)])
            with ctx.genotype_ll([ll], [seeds], [hb["blocks"]], [0, len(reads)], p1, p2, sample, [S], prune=panel is None, fields=fields or {},
                                 locus_haploid=[haploid]) as result:
                g, f = result.locus(0), result.fields(0)
                final = g["blocks"][1]["alleles"]
                ix = np.zeros(len(final), dtype=np.uint8) if inexact is None else \
                    np.asarray([x for a, x in enumerate(inexact) if a not in set(g["removed"][1])], dtype=np.uint8)
                none = np.zeros(0)
                pv = _abi.PackedVcfLocus(dict(
                    chrom=reg["chrom"], region_start=reg["start"], region_stop=reg["stop"], name=reg["name"], motif=reg["motif"],
                    period_str=reg["period_str"], chrom_seq=window, chrom_seq_start=lo, blocks=g["blocks"], block=1, inexact_allele=ix,
                    log_aln_probs=none, log_p1=p1, log_p2=p2, sample_label=np.asarray(sample, dtype=np.int32), alns=alns,
                    aln_deleted=[r["deleted"] for r in reads], log_sample_posteriors=none, sample_total_ll=none,
                    best_haplotypes=np.zeros(0, dtype=np.int32), n_p1s=rs.n_p1s, n_p2s=rs.n_p2s, sample_names=fr["samples"], haploid=haploid,
                    out_sample_names=self.columns))
                lines, _ = result.vcf_records([pv], vopt)
                from_fields, _ = _lib.vcf_record_from_fields(pv, f, vopt)
            return lines[0], dict(f, samples=fr["samples"], from_fields=from_fields, haploid=haploid), None
        finally:
            rs.close()


@pytest.fixture(scope="module")
def composer(gpu_ctx, trio):
    c = Composer(gpu_ctx, trio)
    yield c
    c.close()


def key_of(entry):
    return (entry["chrom"], entry["start"] + 1, entry["stop"])


@pytest.mark.gpu
def test_the_default_run_genotypes_every_chromosome(base, trio):
    report, out, (lines, text) = base
    ok = [e for e in report["loci"] if e["status"] == "ok"]
    assert len(report["loci"]) == len(trio["regions"]) == 40
    assert {e["chrom"] for e in ok} == {r["chrom"] for r in trio["regions"]}     # at least one locus of every chromosome of the BED
    assert len(ok) >= 35 and sorted(lines) == sorted(key_of(e) for e in ok)      # a record for every genotyped locus and no other
    assert report["counters"]["genotype_success"] == len(ok) and report["columns"] == sorted(SAMPLES)
    head = [t for t in text.splitlines() if t.startswith("#")]
    assert head[0].startswith("##fileformat=VCF") and head[-1].split("\t")[9:] == sorted(SAMPLES)
    pos = [int(t.split("\t")[1]) for t in text.splitlines() if not t.startswith("#")]
    assert pos == sorted(pos)
    assert set(report["timing"]["stage_seconds"]) == set(call.STAGES) and all(v > 0 for v in report["timing"]["stage_seconds"].values())
    assert report["timing"]["timers"]["hap_aln_calls"] >= 1 and report["timing"]["chunks"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_loci, overlap", [(1, True), (7, True), (None, False), (1, False), (7, False)])
def test_chunking_and_overlap_change_nothing(gpu_ctx, trio, base, chunk_loci, overlap):
    report, out = run(gpu_ctx, trio, f"chunks_{chunk_loci}_{overlap}", chunk_loci=chunk_loci, overlap=overlap)
    assert open(out, "rb").read() == open(base[1], "rb").read()
    assert strip_timing(report) == strip_timing(base[0])
    assert report["timing"]["chunks"] == (len(trio["regions"]) + (chunk_loci or 40) - 1) // (chunk_loci or 40)


@pytest.mark.gpu
def test_a_byte_limit_closes_chunks_too(gpu_ctx, trio, base):
    report, out = run(gpu_ctx, trio, "bytes", chunk_loci=None, chunk_read_bytes=50000)
    assert open(out, "rb").read() == open(base[1], "rb").read() and strip_timing(report) == strip_timing(base[0])
    assert 1 < report["timing"]["chunks"] < len(trio["regions"])


@pytest.mark.gpu
def test_every_record_equals_its_per_locus_composition(base, trio, composer):
    report, out, (lines, _) = base
    by_key = {(r["chrom"], r["start"] + 1, r["stop"]): r for r in trio["regions"]}
    compared = 0
    for e in report["loci"]:
        if e["status"] != "ok":
            continue
        line, f, failure = composer.locus(by_key[key_of(e)])
        assert failure is None and line == lines[key_of(e)], e["name"]
        assert f["samples"] == e["samples"] and int(f["n_aligned"].sum()) <= e["n_reads"]
        compared += 1
    assert compared == len(lines) >= 35                          # no locus left out


@pytest.mark.gpu
def test_gated_loci_are_reported_and_write_nothing(gpu_ctx, trio, base, composer):
    regions = {(r["chrom"], r["start"] + 1, r["stop"]): r for r in trio["regions"]}
    long_one = [e for e in base[0]["loci"] if e["stop"] - e["start"] > 1000]
    assert len(long_one) == 1 and long_one[0]["gate"] == "too_long" and key_of(long_one[0]) not in base[2][0]     # the defaults remove the 2916-bp region
    for name, options, gate in (("tr_len", dict(max_tr_len=10), "too_long"), ("reads", dict(min_reads=10 ** 6), "too_few_reads"),
                                ("haps", dict(max_haps=1), "too_many_haps")):
        report, out = run(gpu_ctx, trio, "gate_" + name, **options)
        lines, _ = data_lines(out)
        gated = [e for e in report["loci"] if e["gate"] == gate]
        assert gated and report["counters"][gate] == len(gated)
        for e in gated:
            assert e["status"] != "ok" and key_of(e) not in lines
            if gate == "too_long":
                assert e["stop"] - e["start"] > 10 and e["n_records"] == 0           # removed before any read is fetched
            if gate == "too_few_reads":
                assert e["n_reads"] < 10 ** 6 and e["filter_counters"]["passed"] == e["n_reads"]
        if gate == "too_long":
            assert {e["stop"] - e["start"] for e in report["loci"] if e["gate"] is None} <= set(range(11)) and not lines
        if gate == "too_few_reads":
            assert len(gated) == 39 and not lines
        if gate == "too_many_haps":                              # a locus with one haplotype is still genotyped, and as before
            kept = [e for e in report["loci"] if e["status"] == "ok"]
            assert len(kept) + len(gated) == len([e for e in base[0]["loci"] if e["status"] == "ok"])
            for e in kept:
                assert lines[key_of(e)] == base[2][0][key_of(e)]
            assert report["counters"]["genotype_fail"] >= len(gated)
    # the hap-failure gate carries the text of ltr_hap_result_failure: whatever the composition reports for such a locus
    for e in base[0]["loci"]:
        if e["gate"] == "hap_failed":
            assert composer.locus(regions[key_of(e)])[2] == e["status"]


def check_well_formed(line, f, columns):
    c = line.split("\t")
    assert len(c) == 9 + len(columns)
    keys = c[8].split(":")
    assert keys[0] == "GT" and "DP" in keys and "Q" in keys
    for name, col in zip(columns, c[9:]):
        if name not in f["samples"] or col == ".":
            continue
        s = f["samples"].index(name)
        vals = col.split(":")
        assert len(vals) == len(keys), line
        assert int(vals[keys.index("DP")]) == int(f["n_aligned"][s])
        assert 0.0 <= float(vals[keys.index("Q")]) <= 1.0
        sep = "|" if "|" in vals[0] else "/"
        assert len(vals[0].split(sep)) == (1 if f["haploid"] else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name, options, compose", [
    ("haploid", dict(haploid_chrs="chr1"), dict(haploid=True)),
    ("phased", dict(phased_bam=True), dict(phased=True)),
    ("consensus", dict(alleles="consensus"), dict(alleles="consensus")),
    ("gls", dict(output_gls=True, output_pls=True, output_phased_gls=True),
     dict(fields=dict(want_gls=True, want_pls=True, want_phased_gls=True), vopt=_abi.vcf_options(output_gls=1, output_pls=1, output_phased_gls=1))),
])
def test_other_paths_equal_their_composition(gpu_ctx, trio, base, composer, name, options, compose):
    report, out = run(gpu_ctx, trio, name, **options)
    lines, _ = data_lines(out)
    regions = {(r["chrom"], r["start"] + 1, r["stop"]): r for r in trio["regions"]}
    ok = [e for e in report["loci"] if e["status"] == "ok"]
    assert len(ok) >= 35 and sorted(lines) == sorted(key_of(e) for e in ok)
    for e in ok[::3]:                                            # every third locus: the default run compares them all
        line, f, failure = composer.locus(regions[key_of(e)], **compose)
        if name == "gls":
            assert {"GL", "PL", "PHASEDGL"} <= set(lines[key_of(e)].split("\t")[8].split(":"))
        assert failure is None and lines[key_of(e)] == line == f["from_fields"], e["name"]
        check_well_formed(lines[key_of(e)], f, report["columns"])
        if name == "haploid":
            # the haploid FORMAT (no PQ / DSNP / PDP / PSNP); ALLREADS and MALLREADS are on by default, as in the reference
            assert lines[key_of(e)].split("\t")[8] == "GT:GB:Q:DP:DFLANKINDEL:GLDIFF:ALLREADS:MALLREADS"
    if name == "phased":
        assert open(out).read() != open(base[1]).read()          # the HP tags move the posteriors
    if name == "haploid":
        assert open(out).read() != open(base[1]).read()


@pytest.mark.gpu
def test_ref_vcf_panel(gpu_ctx, trio, composer):
    """The panel tests/test_gpu_vcf_panel.py uses, built the way that test builds it: the example's discovery VCF, indexed."""
    d = trio["dir"]
    vcf = str(d / "discovery.vcf.gz")
    rt.run(gpu_ctx, vcf, tmp_dir=str(d))
    _lib.vcf_index(vcf)
    report, out = run(gpu_ctx, trio, "panel", ref_vcf=vcf)
    lines, _ = data_lines(out)
    regions = {(r["chrom"], r["start"] + 1, r["stop"]): r for r in trio["regions"]}
    ok = [e for e in report["loci"] if e["status"] == "ok"]
    assert len(ok) >= 30 and sorted(lines) == sorted(key_of(e) for e in ok)
    panel = _lib.VcfPanel(vcf)
    try:
        for e in report["loci"]:
            if e["gate"] == "hap_failed":
                assert composer.locus(regions[key_of(e)], panel=panel)[2] == e["status"]
        for e in ok[::3]:
            line, f, failure = composer.locus(regions[key_of(e)], panel=panel)
            assert failure is None and lines[key_of(e)] == line == f["from_fields"], e["name"]
            check_well_formed(line, f, report["columns"])
            rec = panel.alleles(e["chrom"], e["start"], e["stop"])
            c = line.split("\t")
            assert int(c[1]) == rec[0] + 1 and c[3] == rec[1][0] and sorted(c[4].split(",")) == sorted(rec[1][1:] or ["."])    # nothing pruned
    finally:
        panel.close()
