"""The host side of longtr_amd.call: the command line, the refused options, the gate order, the chunk planner, the reference
forms and the sample columns.  No GPU."""
import os
import subprocess
import sys

import pytest

from longtr_amd import _lib, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "bam")

OPTIONS = ["--bams", "--fasta", "--regions", "--tr-vcf", "--chrom", "--phased-bam", "--haploid-chrs", "--bam-samps", "--bam-libs", "--ref-vcf",
           "--min-mapq", "--min-mean-qual", "--max-tr-len", "--min-reads", "--max-reads", "--max-haps", "--indel-flank-len",
           "--alignment-params", "--stutter-align-len", "--output-gls", "--output-pls", "--output-phased-gls", "--output-filters", "--alleles"]


def test_help_lists_every_option():
    """The module runs as a command (this is what the test is about: one child process, no GPU touched by --help)."""
    r = subprocess.run([sys.executable, "-m", "longtr_amd.call", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in OPTIONS:
        assert opt in r.stdout, opt
    assert call.make_parser().format_help() == r.stdout


def test_defaults_are_the_reference_s():
    a = call.make_parser().parse_args(["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf"])
    o = call.options_from_args(a)
    assert (o["min_mapq"], o["min_mean_qual"], o["max_tr_len"], o["min_reads"], o["max_reads"], o["max_haps"]) == (20, 30.0, 1000, 10, 1000000, 1000)
    assert (o["indel_flank_len"], o["stutter_align_len"], o["alleles"], o["phased_bam"], o["haploid_chrs"], o["ref_vcf"]) == (5, 0, "exact", False, (), None)
    assert set(o) <= set(call.DEFAULTS) and {k: call.DEFAULTS[k] for k in o if k != "overlap"} == {k: v for k, v in o.items() if k != "overlap"}


BASE = ["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf"]


@pytest.mark.parametrize("extra, key", [(["--snp-vcf", "s.vcf.gz"], "snp_vcf"), (["--fam", "x.fam"], "fam"), (["--pass-bam", "p.bam"], "pass_bam"),
                                        (["--filt-bam", "f.bam"], "filt_bam"), (["--viz-out", "v.gz"], "viz_out")])
def test_refused_options_give_their_sentence(extra, key, capsys):
    args = call.make_parser().parse_args(BASE + extra)
    with pytest.raises(_lib.LtrError) as e:
        call.options_from_args(args)
    assert call.REFUSED[key] in str(e.value) and call.REFUSED[key].count(".") == 1
    with pytest.raises(SystemExit):                              # and the command ends with it, before any GPU is opened
        call.main(BASE + extra)
    assert call.REFUSED[key] in capsys.readouterr().err
    with pytest.raises(_lib.LtrError) as e:                      # the function refuses the same keyword
        call.genotype_regions(None, ["a.bam"], "f.fa", "r.bed", "o.vcf", **{key: extra[1]})
    assert call.REFUSED[key] in str(e.value)


def test_cram_is_refused():
    args = call.make_parser().parse_args(["--bams", "a.bam,b.cram"] + BASE[2:])
    with pytest.raises(_lib.LtrError) as e:
        call.options_from_args(args)
    assert call.CRAM_REFUSAL in str(e.value)
    with pytest.raises(_lib.LtrError) as e:
        call.genotype_regions(None, ["b.CRAM"], "f.fa", "r.bed", "o.vcf")
    assert call.CRAM_REFUSAL in str(e.value)


def test_unknown_option_is_an_error():
    with pytest.raises(TypeError):
        call.genotype_regions(None, ["a.bam"], "f.fa", "r.bed", "o.vcf", min_map_q=3)
    with pytest.raises(_lib.LtrError):
        call.genotype_regions(None, ["a.bam"], "f.fa", "r.bed", "o.vcf", alleles="poa")


# ---- gates: one made-up locus per gate, each of which also fails every LATER gate -------------------------------------------------
FINE = dict(start=10000, stop=10040, chrom_len=100000, n_reads=30, too_many_reads=False, hap_built=True, hap_failure="", n_haps=4, missing_pair=False)
BREAK = [("too_long", dict(stop=10000 + 1001)), ("contig_end", dict(chrom_len=10040 + 50)), ("too_few_reads", dict(n_reads=9)),
         ("too_many_reads", dict(too_many_reads=True)), ("hap_failed", dict(hap_built=False, hap_failure="the text of ltr_hap_result_failure")),
         ("too_many_haps", dict(n_haps=1001)), ("no_optimal_pair", dict(missing_pair=True))]


def test_gate_order():
    assert [g[0] for g in call.GATES] == [b[0] for b in BREAK]
    assert call.apply_gates(FINE, {}) is None
    for k, (name, change) in enumerate(BREAK):
        assert call.apply_gates(dict(FINE, **change), {})[0] == name          # the gate alone
        facts = dict(FINE)
        for _, later in BREAK[k:]:
            facts.update(later)
        assert call.apply_gates(facts, {})[0] == name                         # and in front of every later gate
    assert call.apply_gates(dict(FINE, hap_built=False, hap_failure="the text of ltr_hap_result_failure"), {})[1] == "the text of ltr_hap_result_failure"


def test_gate_boundaries():
    ok = lambda **kw: call.apply_gates(dict(FINE, **{k: v for k, v in kw.items() if k in FINE}), {k: v for k, v in kw.items() if k not in FINE})
    assert ok(stop=10000 + 1000) is None and ok(stop=10000 + 1001)[0] == "too_long"       # stop - start > MAX_STR_LENGTH
    assert ok(start=50, stop=60) is None and ok(start=49, stop=60)[0] == "contig_end"     # start < 50
    assert ok(chrom_len=10040 + 51) is None and ok(chrom_len=10040 + 50)[0] == "contig_end"    # stop + 50 >= size
    assert ok(n_reads=10) is None and ok(n_reads=9)[0] == "too_few_reads"                 # total < MIN_TOTAL_READS
    assert ok(n_haps=1000) is None and ok(n_haps=1001)[0] == "too_many_haps"              # num_combs > max
    assert ok(n_reads=3, min_reads=3) is None and ok(max_tr_len=39)[0] == "too_long" and ok(max_haps=3)[0] == "too_many_haps"


def test_gates_wait_for_their_facts():
    """A locus that has no reads yet has passed the gates before the read gates and no other."""
    assert call.apply_gates(dict(start=10000, stop=10040, chrom_len=100000), {}) is None
    assert call.apply_gates(dict(start=10000, stop=10040, chrom_len=100000, n_reads=2, too_many_reads=False), {})[0] == "too_few_reads"
    assert call.apply_gates(dict(start=10000, stop=12000), {})[0] == "too_long"


# ---- chunks -------------------------------------------------------------------------------------------------------------------------
def test_chunk_planner():
    sizes = [10, 10, 10, 10, 10, 10, 10]
    assert call.plan_chunks(sizes, 3, None) == [(0, 3), (3, 6), (6, 7)]                   # the locus limit
    assert call.plan_chunks(sizes, None, 25) == [(0, 3), (3, 6), (6, 7)]                  # the byte limit (closes once reached)
    assert call.plan_chunks(sizes, 2, 1000) == [(0, 2), (2, 4), (4, 6), (6, 7)]           # whichever comes first
    assert call.plan_chunks(sizes, 5, 20) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert call.plan_chunks(sizes, None, None) == [(0, 7)] and call.plan_chunks(sizes, 0, 0) == [(0, 7)]
    assert call.plan_chunks([5, 500, 5], 10, 100) == [(0, 2), (2, 3)]                     # a locus larger than the limit is not split
    assert call.plan_chunks([500, 500], 10, 100) == [(0, 1), (1, 2)]
    assert call.plan_chunks([0, 0, 0], 2, 100) == [(0, 2), (2, 3)]                        # loci a gate emptied still count as loci
    assert call.plan_chunks([], 4, 4) == []
    for cl, cb in ((1, None), (3, 17), (None, 1), (4, 10 ** 9)):
        plan = call.plan_chunks(list(range(40)), cl, cb)
        assert [a for a, _ in plan] == [0] + [b for _, b in plan[:-1]] and plan[-1][1] == 40 and all(a < b for a, b in plan)


# ---- the reference: a FASTA path and an object give the same windows -----------------------------------------------------------------
def test_fasta_path_equals_dict_reference(tmp_path):
    import random
    rnd = random.Random(5)
    seqs = {"chrA": "".join(rnd.choice("ACGT") for _ in range(2345)), "chrB": "".join(rnd.choice("ACGT") for _ in range(777))}
    fa, width, fai, off = tmp_path / "two.fa", 60, [], 0
    with open(fa, "w") as f:
        for name, s in seqs.items():
            head = f">{name}\n"
            f.write(head)
            off += len(head)
            fai.append(f"{name}\t{len(s)}\t{off}\t{width}\t{width + 1}\n")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")
                off += len(s[i:i + width]) + 1
    open(str(fa) + ".fai", "w").write("".join(fai))
    a, b = call.FastaReference(str(fa)), call.DictReference(seqs)
    try:
        for chrom, s in seqs.items():
            assert a.length(chrom) == b.length(chrom) == len(s)
            for start, stop in ((500, 540), (60, 120), (10, 30), (len(s) - 100, len(s) - 60), (0, len(s))):
                wa, wb = call.reference_window(a, chrom, start, stop, a.length(chrom)), call.reference_window(b, chrom, start, stop, b.length(chrom))
                lo, hi = max(start - call.REF_PAD, 0), min(stop + call.REF_PAD, len(s))
                assert wa == wb == (lo, s[lo:hi].encode())
        assert a.length("chrC") == b.length("chrC") == -1
        assert a.contig_lines() == b.contig_lines() and a.contig_lines().count("##contig") == 2
    finally:
        a.close()


# ---- samples --------------------------------------------------------------------------------------------------------------------------
def test_sample_columns_from_read_groups_and_bam_samps():
    files = [os.path.join(DATA, f"{s}_sample_reads.bam") for s in ("HG004", "HG002", "HG003")]       # three files, not in name order
    bam = _lib.Bam(files, merge_by_position=False)
    rgs = bam.read_groups()
    bam.close()
    assert [g["sample"] for g in sorted(rgs, key=lambda g: g["file"])] == ["HG004", "HG002", "HG003"]
    assert call.sample_columns(rgs, None, 3) == ["HG002", "HG003", "HG004"]                          # a std::set: sorted, unique
    assert call.sample_columns(rgs + rgs, None, 3) == ["HG002", "HG003", "HG004"]
    assert call.sample_columns(rgs, ["zz", "b", "b"], 3) == ["b", "zz"]                              # --bam-samps: the given names, RGs unused
    assert call.sample_columns(rgs, ["B", "a", "C"], 3) == ["B", "C", "a"]                           # byte order, like std::string
    with pytest.raises(_lib.LtrError) as e:
        call.sample_columns(rgs, ["a", "b"], 3)
    assert "must match" in str(e.value)
    with pytest.raises(_lib.LtrError) as e:
        call.sample_columns([g for g in rgs if g["file"] != 1], None, 3)
    assert "don't contain read groups" in str(e.value)


# ---- the producer thread ----------------------------------------------------------------------------------------------------------------
class _Item:
    rs = None

    def __init__(self, k):
        self.k = k


def _producers():
    import threading
    return [t for t in threading.enumerate() if t.name == "ltr-call-producer"]


def test_producer_hands_chunks_over_in_order_and_stops_when_dropped():
    chunks = [[_Item(3 * c + i) for i in range(3)] for c in range(5)]
    assert [[p.k for p in c] for c in call._ahead(iter(chunks))] == [[p.k for p in c] for c in chunks]
    assert not _producers()
    gen = call._ahead(iter(chunks))
    assert [p.k for p in next(gen)] == [0, 1, 2]
    gen.close()                                                  # the consumer gives up: the thread ends, nothing is left waiting on the queue
    assert not _producers()


def test_producer_error_reaches_the_caller():
    def failing():
        yield [_Item(0)]
        raise ValueError("the BAM ended early")
    gen = call._ahead(failing())
    assert [p.k for p in next(gen)] == [0]
    with pytest.raises(ValueError, match="the BAM ended early"):
        next(gen)
    assert not _producers()
