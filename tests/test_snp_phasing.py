"""libltr_snp.so (include/ltr_snp.h) against the Python restatement of the same reference lines (tests/snp_phasing_util.py): bit for
bit, since both add the same doubles in the same order.  The two base-quality tables are pinned to oracle_lib's base_quality (the
compiled reference where oracle/_ref is built, the oracle restatement otherwise).  Then PhasedSnps over a BGZF VCF written by
VcfWriter and indexed by ltr_vcf_index, and the driver's options.  No GPU."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import snp_phasing_util as U
from longtr_amd import _abi, _lib, _snp, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "bam")
TABLES = _snp.quality_tables()
READ_CASES, RECORD_CASES = U.read_cases(), U.record_cases()


def same_bits(a, b):
    return np.array_equal(U.bits(a), U.bits(b))


def test_quality_tables_equal_the_reference_s():
    _, _, bq, _ = ol.stutter_scalars("ref" if ol.have_ref() else "oracle", _abi.default_stutter_params())
    correct, error = TABLES
    assert len(correct) == len(error) == ord("J") - ord("!") + 1 == _snp.N_QUALITIES
    assert correct[0] == -100.0 and error[0] == 0.0
    for byte in range(256):
        e, c = bq(byte)
        i = U.quality_index(byte)
        assert (float(error[i]).hex(), float(correct[i]).hex()) == (e.hex(), c.hex()), byte
    assert [U.quality_index(b) for b in (0x20, 0x21, 0x22, 0x4a, 0x4b, 0x7f, 0x80, 0xff)] == [0, 0, 1, 41, 41, 41, 0, 0]


@pytest.mark.parametrize("name, snps, reads, want", READ_CASES, ids=[c[0] for c in READ_CASES])
def test_one_read_per_branch(name, snps, reads, want):
    status, counts = want
    ref_set = U.build_set(U.HEADER + "\tS", U.snp_lines(snps))
    assert ref_set["snps"] == [sorted(snps, key=lambda s: s[0])]
    with _snp.SnpSet(U.HEADER + "\tS", U.snp_lines(snps)) as s:
        assert s.snps(0) == ref_set["snps"][0] and s.sample_index("S") == 0
        got_counts = np.array([5, 6, 7], dtype=np.int32)
        if status != U.OK:
            with pytest.raises(U.SnpDie) as e:
                U.priors(ref_set, 0, reads, TABLES)
            assert e.value.code == status
            with pytest.raises(_lib.LtrError) as e:
                s.priors(0, reads, got_counts)
            assert e.value.code == status and "read 0" in str(e.value)
            assert list(got_counts) == [5, 6, 7]                 # nothing is added on an error
            return
        p1, p2, n = U.priors(ref_set, 0, reads, TABLES)
        g1, g2 = s.priors(0, reads, got_counts)
        assert same_bits(g1, p1) and same_bits(g2, p2), (g1, p1, g2, p2)
        assert n == counts and list(got_counts) == [5 + n[0], 6 + n[1], 7 + n[2]]     # both say what the case was made to show; counts are added to
        assert (np.asarray(p1) != 0).any() == (sum(n) > 0)
        z1, z2 = s.priors(-1, reads)                             # a sample the VCF does not hold
        assert not z1.any() and not z2.any() and len(z1) == len(reads)


def test_ties_in_position_decide_the_last_bit():
    """The case two_at_one_position is made so that the other order of its two SNPs gives another sum: the order is part of the contract."""
    name, snps, reads, _ = next(c for c in READ_CASES if c[0] == "two_at_one_position")
    a = U.priors(U.build_set(U.HEADER + "\tS", U.snp_lines(snps)), 0, reads, TABLES)
    b = U.priors(U.build_set(U.HEADER + "\tS", U.snp_lines([snps[0], snps[2], snps[1]])), 0, reads, TABLES)
    assert not (same_bits(a[0], b[0]) and same_bits(a[1], b[1]))


@pytest.mark.parametrize("name, header, lines, skip, want", RECORD_CASES, ids=[c[0] for c in RECORD_CASES])
def test_one_record_per_rule(name, header, lines, skip, want):
    if want[0] != U.OK:
        with pytest.raises(U.SnpDie) as e:
            U.build_set(header, lines, skip)
        assert e.value.code == want[0]
        with pytest.raises(_lib.LtrError) as e:
            _snp.SnpSet(header, lines, skip)
        assert e.value.code == want[0] and f"POS {want[1]}" in str(e.value)
        return
    ref = U.build_set(header, lines, skip)
    with _snp.SnpSet(header, lines, skip) as s:
        got = [s.snps(c) for c in range(len(s.samples))]
        assert s.samples == ref["samples"] and s.n_valid_snps == ref["n_valid"] and got == ref["snps"]
        assert (ref["n_valid"], ref["snps"]) == want[1:]
        for sample in set(ref["samples"]):
            assert s.sample_index(sample) == ref["index"][sample]
        assert s.sample_index("absent") == -1
        with pytest.raises(_lib.LtrError):
            s.snps(len(s.samples))
    if name == "duplicate_sample_name":
        assert ref["index"] == {"S1": 1}                         # the last column of a name wins


def test_bad_arguments_are_refused():
    with pytest.raises(_lib.LtrError):
        _snp.SnpSet("chr1\t1\t.\tA\tC", [])                      # not a #CHROM line
    with _snp.SnpSet(U.HEADER + "\tS", []) as s:
        with pytest.raises(_lib.LtrError):
            s.priors(1, [U.make_read(100, "4M")])                # no such column
        with pytest.raises(_lib.LtrError):
            s.priors(0, [], counts=np.zeros(3))                  # counts is int32
    L = _snp.snp_lib()
    h = C.c_void_p()
    assert L.ltr_snp_set_create(None, b"", 0, None, None, 0, 15, C.byref(h), None, 0) == -1 and not h
    assert L.ltr_snp_set_n_samples(None) == 0 and L.ltr_snp_set_n_snps(None, 0) == -1 and L.ltr_snp_set_sample_index(None, b"x") == -1
    L.ltr_snp_set_free(None)


def test_signature_table_matches_the_header():
    """Every function include/ltr_snp.h declares is in _abi.SNP_SIGNATURES with as many parameters, and is exported; nothing of it
    is in libltr_gpu.so's tables."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_snp.h")).read(), flags=re.S)
    decls = {m.group(1): [p for p in m.group(2).split(",") if p.strip() not in ("", "void")]
             for m in re.finditer(r"\b(ltr_snp_\w+)\s*\(([^()]*)\)\s*;", src)}
    assert set(decls) == set(_abi.SNP_SIGNATURES) and len(decls) == 10
    L = _snp.snp_lib()
    for name, params in decls.items():
        restype, argtypes = _abi.SNP_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for p, ct in zip(params, argtypes):
            assert ("*" in p) == (ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer)), (name, p)
        assert getattr(L, name).argtypes == argtypes
    fields = re.search(r"typedef struct ltr_snp_read \{(.*?)\}", src, flags=re.S).group(1)
    names = [n for decl in fields.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in _abi.SnpRead._fields_]
    assert not set(_abi.SNP_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.HOOK_SIGNATURES) | set(_abi.PLOIDY_SIGNATURES) | set(_lib.EXPORTS))
    assert _lib.lib().ltr_abi_version() == 6
    assert (_snp.SKIP_PADDING, _snp.N_QUALITIES) == tuple(int(re.search(rf"#define {k}\s+(\d+)", src).group(1))
                                                          for k in ("LTR_SNP_SKIP_PADDING", "LTR_SNP_N_QUALITIES"))


# ---- seeded differential through a BGZF VCF -------------------------------------------------------------------------------------
def random_cigar(rng, n_ref):
    """A CIGAR over about n_ref reference bases: soft clips at the ends, M / = / X runs with I and D between them."""
    ops = [("S", int(rng.integers(1, 30)))] if rng.random() < 0.3 else []
    left = n_ref
    while left > 0:
        n = int(min(left, rng.integers(1, 60)))
        ops.append((str(rng.choice(["M", "=", "X"], p=[0.5, 0.4, 0.1])), n))
        left -= n
        if left > 0 and rng.random() < 0.6:
            op = str(rng.choice(["I", "D"]))
            n = int(rng.integers(1, 12))
            ops.append((op, n))
            left -= n if op == "D" else 0
    if rng.random() < 0.3:
        ops.append(("S", int(rng.integers(1, 30))))
    if rng.random() < 0.1:
        ops = [("H", 5)] + ops + [("H", 7)]
    return ops


def random_read(rng, lo, hi):
    pos = int(rng.integers(lo, hi))
    cigar = random_cigar(rng, int(rng.integers(20, 900)))
    n_query = sum(n for op, n in cigar if op in "M=XIS")
    return dict(pos=pos, end_pos=pos + sum(n for op, n in cigar if op in "M=XD"), cigar=cigar,
                bases=bytes(rng.choice(list(b"ACGT"), size=n_query).astype(np.uint8)),
                quals=bytes(rng.integers(0x21, 0x60, size=n_query).astype(np.uint8)))


@pytest.fixture(scope="module")
def snp_vcf(tmp_path_factory):
    """A VCF of three samples (one name twice) over chr1 0 .. 6000 and a few records on chr2, written and indexed by the library."""
    rng = np.random.default_rng(20240611)
    path = str(tmp_path_factory.mktemp("snp") / "phased.vcf.gz")
    header = U.HEADER + "\tNA1\tNA2\tNA1"
    gts = ["0|1", "1|0", "0/1", "1|1", "0|0", ".|.", ".", "1", "0|1", "1|0"]
    lines = []
    for chrom, n in (("chr1", 700), ("chr2", 5)):
        for pos in sorted(int(p) for p in rng.integers(1, 6000, size=n)):          # positions repeat now and then
            ref, alt = (str(x) for x in rng.choice(list("ACGT"), size=2, replace=False))
            kind = rng.random()
            if kind < 0.08:
                alt = str(rng.choice(["AT", "*", "<DEL>", ref + "," + alt, "."]))
                if alt == "AT" and rng.random() < 0.5:
                    ref, alt = "AT", "A"
            calls = [str(rng.choice(gts)) for _ in range(3)]
            if alt == ".":
                calls = [c.replace("1", "0") for c in calls]
            fmt, calls = ("GT", calls) if rng.random() < 0.8 else ("DP:GT", [f"{int(rng.integers(1, 60))}:{c}" for c in calls])
            lines.append("\t".join([chrom, str(pos), ".", ref, alt, ".", "PASS", ".", fmt] + calls))
    w = _lib.VcfWriter(path)
    w.header("##fileformat=VCFv4.2\n" + header + "\n")
    for t in lines:
        w.add_record(t.split("\t")[0], int(t.split("\t")[1]), t)
    w.close()
    _lib.vcf_index(path)
    with gzip.open(path, "rt") as fh:                            # the writer orders by position: records at one position in ITS order
        written = [t.rstrip("\n") for t in fh if not t.startswith("#")]
    assert sorted(written) == sorted(lines)
    return dict(path=path, header=header, lines=written)


def in_window(line, chrom, lo, hi):
    """A tabix query: the record's interval [POS - 1, POS - 1 + len(REF)) overlaps the 0-based half-open [lo, hi)."""
    c = line.split("\t")
    return c[0] == chrom and int(c[1]) - 1 < hi and int(c[1]) - 1 + len(c[3]) > lo


@pytest.mark.parametrize("start, stop", [(400, 460), (1000, 1030), (1001, 1020), (3000, 3100)])
def test_seeded_reads_through_a_bgzf_vcf(snp_vcf, start, stop):
    """The window rule either side of start = 1000 (snp_bam_processor.cpp:61): the query starts at 0 up to there, at start - 1001 + 1 after."""
    lo, hi = (0 if start <= 1000 else start - 1001), stop + 1000
    assert _snp.snp_window(start, stop) == (lo, hi)
    mine = [t for t in snp_vcf["lines"] if in_window(t, "chr1", lo, hi)]
    ref = U.build_set(snp_vcf["header"], mine, [(start, stop)], 15)
    assert ref["n_valid"] > 50 and all(len(v) > 10 for v in ref["snps"])
    assert not [s for v in ref["snps"] for s in v if start - 15 <= s[0] + 1 <= stop + 15]
    rng = np.random.default_rng(start)
    reads = [random_read(rng, max(lo - 300, 1), hi) for _ in range(100)]
    snps = _lib.PhasedSnps(snp_vcf["path"])
    try:
        assert snps.samples == ["NA1", "NA2", "NA1"] and snps.chromosomes == ["chr1", "chr2"]
        assert snps.has_chromosome("chr2") and not snps.has_chromosome("1")
        with snps.window("chr1", start, stop) as s:
            assert s.n_valid_snps == ref["n_valid"] and [s.snps(c) for c in range(3)] == ref["snps"]
            assert s.sample_index("NA1") == 2 and ref["index"] == {"NA1": 2, "NA2": 1}
            total, want_total = np.zeros(3, dtype=np.int32), [0, 0, 0]
            for name in ("NA1", "NA2", "NA3"):
                column = ref["index"].get(name, -1)
                p1, p2, n = U.priors(ref, column, reads, TABLES)
                g1, g2 = snps.priors(s, name, reads, total)
                want_total = [a + b for a, b in zip(want_total, n)]
                assert same_bits(g1, p1) and same_bits(g2, p2), name
                assert (column < 0) == (not p1.any())
                if column >= 0:
                    assert (p1 != p2).sum() > 30 and min(n) > 5   # reads on both sides and mismatches: every branch of the sums ran
            assert list(total) == want_total
    finally:
        snps.close()


# ---- the driver's options -------------------------------------------------------------------------------------------------------
BASE = ["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf"]


def test_phased_snps_is_an_option_and_snp_vcf_is_still_refused(capsys):
    o = call.options_from_args(call.make_parser().parse_args(BASE + ["--phased-snps", "p.vcf.gz"]))
    assert o["phased_snps"] == "p.vcf.gz" and call.DEFAULTS["phased_snps"] is None
    assert call.options_from_args(call.make_parser().parse_args(BASE))["phased_snps"] is None
    assert "--phased-snps <phased_snps.vcf.gz>" in call.make_parser().format_help()
    with pytest.raises(_lib.LtrError) as e:
        call.options_from_args(call.make_parser().parse_args(BASE + ["--snp-vcf", "p.vcf.gz"]))
    assert call.REFUSED["snp_vcf"] in str(e.value) and "--phased-snps" in call.REFUSED["snp_vcf"] and call.REFUSED["snp_vcf"].count(".") == 1
    with pytest.raises(_lib.LtrError):
        call.options_from_args(call.make_parser().parse_args(BASE + ["--phased-snps", "p.vcf.gz", "--fam", "x.fam"]))


class NoGpu:
    """A context for runs in which every locus is gated before the GPU is asked anything."""

    params = _abi.default_params()

    def set_params(self, p):
        pass

    def timers(self):
        return {}


class Lengths:
    path = ""

    def length(self, chrom):
        return 250000000 if chrom in ("chr1", "chr5") else -1

    def contig_lines(self):
        return ""


BAMS = [os.path.join(DATA, f"{s}_sample_reads.bam") for s in ("HG002", "HG003", "HG004")]
LONG = dict(start=100000, stop=105000, name="too_long", motif="A", period=1, period_str="1")         # removed by --max-tr-len: no read is fetched


def small_vcf(d, name, chroms):
    path = str(d / name)
    w = _lib.VcfWriter(path)
    w.header("##fileformat=VCFv4.2\n" + U.HEADER + "\tHG002\n")
    for c in chroms:
        w.add_record(c, 100, f"{c}\t100\t.\tA\tC\t.\t.\t.\tGT\t0|1")
    w.close()
    _lib.vcf_index(path)
    return path


def test_a_chromosome_missing_from_the_snp_vcf_raises_before_any_output(tmp_path):
    out = str(tmp_path / "out.vcf")
    regions = [dict(LONG, chrom="chr1"), dict(LONG, chrom="chr5")]
    with pytest.raises(_lib.LtrError) as e:
        call.genotype_regions(NoGpu(), BAMS, Lengths(), regions, out, phased_snps=small_vcf(tmp_path, "a.vcf.gz", ["5", "chr1", "chr7"]))
    assert e.value.code == _abi.LTR_ERR_INVALID and not os.path.exists(out)
    assert "No entries for chromosome chr5 found in the SNP VCF file" in str(e.value)
    assert "Please ensure that the chromosome names in your BED file match those in your SNP VCF file" in str(e.value)
    assert "NOTE: Found chromosome 5 in the VCF, but not chromosome chr5" in str(e.value)
    with pytest.raises(_lib.LtrError) as e:                      # the other hint: the VCF says chr1 where the regions say 1
        call.verify_vcf_chromosomes(_lib.PhasedSnps(small_vcf(tmp_path, "b.vcf.gz", ["chr1"])), ["1"])
    assert "NOTE: Found chromosome chr1 in the VCF, but not chromosome 1" in str(e.value)
    with pytest.raises(_lib.LtrError):                           # a file that cannot be opened raises too
        call.genotype_regions(NoGpu(), BAMS, Lengths(), regions[:1], out, phased_snps=str(tmp_path / "absent.vcf.gz"))
    assert not os.path.exists(out)
    # with both chromosomes there the run goes through (both loci gated) and reports the option's keys
    report = call.genotype_regions(NoGpu(), BAMS, Lengths(), regions, out, phased_snps=small_vcf(tmp_path, "c.vcf.gz", ["chr1", "chr5"]))
    assert report["error"] is None and [e["gate"] for e in report["loci"]] == ["too_long", "too_long"]
    assert report["counters"]["snp_match"] == report["counters"]["snp_mismatch"] == 0 and report["timing"]["snp_seconds"] == 0.0
    assert "phased_snps" not in report and set(report["timing"]["stage_seconds"]) == set(call.STAGES)


def test_phased_bam_wins_and_the_snp_file_is_never_opened(tmp_path):
    out = str(tmp_path / "out.vcf")
    absent = str(tmp_path / "absent.vcf.gz")
    report = call.genotype_regions(NoGpu(), BAMS, Lengths(), [dict(LONG, chrom="chr1")], out, phased_snps=absent, phased_bam=True)
    assert report["error"] is None and "--phased-snps will be ignored" in report["phased_snps"]
    assert "snp_seconds" not in report["timing"] and "snp_match" not in report["counters"]
    plain = call.genotype_regions(NoGpu(), BAMS, Lengths(), [dict(LONG, chrom="chr1")], out)
    assert set(plain) == {"loci", "counters", "columns", "error", "timing"} and set(plain["counters"]) == set(call.COUNTERS)
    assert set(plain["timing"]) == {"stage_seconds", "timers", "wall_seconds", "chunks"} and "snp_info" not in plain["loci"][0]
