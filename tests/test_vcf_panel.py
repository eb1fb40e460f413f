"""--ref-vcf input without htslib (longtr_amd/csrc/ltr_vcf_in.cpp, ltr_build_vcf_haplotype): the tabix index writer and
reader against a linear scan of the same BGZF file, the fixed header of a real htslib index, the record rules of
read_vcf_alleles (src/vcf_input.cpp:21-50) and the panel haplotype of add_vcf_haplotype_block + fuse_haplotype_blocks.
CPU only.  Parity with the reference itself is UNPINNED: its VCF reader is htslib."""
import gzip
import os
import random
import shutil
import struct

import pytest

from longtr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HTSLIB_TBI = os.path.join(ROOT, "tests", "golden", "1kg.chr1.imputed.vcf.gz.tbi")
HEADER = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"


def _write_vcf(path, records, header=HEADER, index=True):
    """records: (chrom, pos, ref, alt, info) with pos 1-based, in the order the writer gets them."""
    w = _lib.VcfWriter(str(path))
    w.header(header)
    for chrom, pos, ref, alt, info in records:
        w.add_record(chrom, pos, f"{chrom}\t{pos}\t.\t{ref}\t{alt}\t.\t.\t{info}\tGT\t0/0")
    w.close()
    if index:
        _lib.vcf_index(str(path))
    return str(path)


def _interval(line):
    c = line.split("\t")
    beg = int(c[1]) - 1
    end = beg + len(c[3])
    for kv in c[7].split(";"):
        if kv.startswith("END="):
            end = max(end, int(kv[4:]))
    return c[0], beg, end


# ---- 1. index round trip ------------------------------------------------------------------------------------
def test_index_round_trip_matches_linear_scan(tmp_path):
    rng = random.Random(7)
    contigs = [("chrA", 5_000_000), ("chr2", 1_500_000), ("chrX_random", 40_000)]
    records = []
    for chrom, length in contigs:
        pos = rng.randint(1, 300)
        while pos < length:
            ref = "".join(rng.choice("ACGT") for _ in range(rng.choice((1, 2, 5, 30, 120))))
            alt = ",".join("".join(rng.choice("ACGT") for _ in range(rng.randint(1, 60))) for _ in range(rng.randint(1, 3)))
            r = rng.random()
            if r < 0.05:
                end = pos + rng.randint(20_000, 400_000)                 # far beyond POS: spans bins and linear windows
            elif r < 0.6:
                end = pos - 1 + len(ref) + rng.randint(0, 300)
            else:
                end = None
            info = f"PAD={rng.getrandbits(rng.choice((8, 64, 256))):x};START={pos + 1}" + (f";END={end}" if end else "")
            records.append((chrom, pos, ref, alt, info))
            pos += rng.choice((1, 3, 40, 200, 1500, 4000))
    vcf = _write_vcf(tmp_path / "big.vcf.gz", records)
    assert os.path.getsize(vcf) > 300_000
    text = gzip.decompress(open(vcf, "rb").read()).decode()
    lines = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert len(lines) == len(records)
    parsed = [(_interval(ln), ln) for ln in lines]
    idx = _lib.tbi_parse(vcf + ".tbi")
    assert idx["names"] == [c for c, _ in contigs]
    assert all(b > 10 for b in idx["bins"][:2])                        # several 16 kb bins per long contig
    panel = _lib.VcfPanel(vcf)
    for _ in range(2000):
        chrom, length = rng.choice(contigs + [("chrUnknown", 1000)])
        beg = rng.randint(0, length + 1000)
        end = beg + rng.choice((1, 10, 500, 20_000, 200_000))
        want = [ln for (c, b, e), ln in parsed if c == chrom and b < end and e > beg]
        assert panel.query_lines(chrom, beg, end) == want, (chrom, beg, end)
    panel.close()


# ---- 2. a real htslib index ----------------------------------------------------------------------------------
def test_written_index_header_matches_htslib(tmp_path):
    vcf = _write_vcf(tmp_path / "one.vcf.gz", [("1", 100, "AC", "A", "START=100;END=101")])
    mine = gzip.decompress(open(vcf + ".tbi", "rb").read())
    theirs = gzip.decompress(open(HTSLIB_TBI, "rb").read())
    assert mine[:4] == theirs[:4] == b"TBI\x01"
    assert mine[8:32] == theirs[8:32]                                  # format, col_seq, col_beg, col_end, meta, skip
    assert struct.unpack("<6i", theirs[8:32]) == (2, 1, 2, 0, ord("#"), 0)


def test_reader_parses_htslib_index():
    d = _lib.tbi_parse(HTSLIB_TBI)                                     # (rejects a chunk whose start lies after its end)
    assert (d["format"], d["col_seq"], d["col_beg"], d["col_end"], d["meta"], d["skip"]) == (2, 1, 2, 0, ord("#"), 0)
    assert d["names"] == ["1"]
    assert d["bins"][0] > 0 and d["chunks"][0] >= d["bins"][0]


def test_open_errors(tmp_path):
    vcf = _write_vcf(tmp_path / "noidx.vcf.gz", [("1", 100, "AC", "A", "START=100;END=101")], index=False)
    with pytest.raises(_lib.LtrError, match="tabix index"):
        _lib.VcfPanel(vcf)
    with pytest.raises(_lib.LtrError, match="Failed to open"):
        _lib.VcfPanel(str(tmp_path / "missing.vcf.gz"))
    plain = _write_vcf(tmp_path / "plain.vcf", [("1", 100, "AC", "A", "START=100;END=101")], index=False)
    shutil.copy(vcf + ".tbi" if os.path.exists(vcf + ".tbi") else HTSLIB_TBI, plain + ".tbi")
    with pytest.raises(_lib.LtrError, match="bgzip"):
        _lib.VcfPanel(plain)


# ---- 3. read_vcf_alleles ---------------------------------------------------------------------------------------
def _panel(tmp_path, records, name="p.vcf.gz"):
    return _lib.VcfPanel(_write_vcf(tmp_path / name, records))


def test_record_without_start_end_is_skipped(tmp_path):
    p = _panel(tmp_path, [("c1", 1000, "ACACAC", "AC", "END=1005"), ("c1", 1001, "CACACAC", "C", "START=1001")])
    assert p.alleles("c1", 1000, 1005) is None
    p2 = _panel(tmp_path, [("c1", 1000, "ACACAC", "AC", "END=1005"), ("c1", 1000, "ACACAC", "ACAC", "START=1001;END=1005")], "p2.vcf.gz")
    assert p2.alleles("c1", 1000, 1005) == (999, ["ACACAC", "ACAC"])


def test_start_end_mismatch_is_not_found(tmp_path):
    p = _panel(tmp_path, [("c1", 1000, "ACACAC", "AC", "START=1001;END=1006")])
    assert p.alleles("c1", 1000, 1005) is None
    assert p.alleles("c1", 999, 1006) is None
    assert p.alleles("c1", 1000, 1006) == (999, ["ACACAC", "AC"])


def test_matching_record_is_picked_among_several(tmp_path):
    p = _panel(tmp_path, [("c1", 980, "GT", "G", "START=980;END=981"), ("c1", 1000, "ACACAC", "AC", "START=1000;END=1005"),
                          ("c1", 1001, "CACAC", "CAC,C", "START=1002;END=1005"), ("c1", 1010, "TTTT", "T", "START=1002;END=1005")])
    assert p.alleles("c1", 1001, 1005) == (1000, ["CACAC", "CAC", "C"])


def test_record_past_start_plus_50_ends_the_scan(tmp_path):
    # the first record past region_start + 50 (POS 1051 > 1000 + 50) ends the scan before the matching one at POS 1052
    p = _panel(tmp_path, [("c1", 1051, "AA", "A", "START=1;END=2"), ("c1", 1052, "CACAC", "C", "START=1001;END=1005")])
    assert p.alleles("c1", 1000, 1005) is None
    q = _panel(tmp_path, [("c1", 1050, "AA", "A", "START=1;END=2"), ("c1", 1051, "CACAC", "C", "START=1001;END=1005")], "q.vcf.gz")
    assert q.alleles("c1", 1000, 1005) == (1050, ["CACAC", "C"])      # POS 1050 is not past it: the scan goes on


def test_locus_near_contig_start(tmp_path):
    p = _panel(tmp_path, [("c1", 3, "ATATAT", "AT,ATATATAT", "START=4;END=8"), ("c1", 30, "GG", "G", "START=31;END=31")])
    assert p.alleles("c1", 3, 8) == (2, ["ATATAT", "AT", "ATATATAT"])
    assert p.alleles("c1", 30, 31) == (29, ["GG", "G"])


def test_unknown_contig_is_not_found(tmp_path):
    p = _panel(tmp_path, [("c1", 1000, "ACACAC", "AC", "START=1001;END=1005")])
    assert p.alleles("c2", 1000, 1005) is None
    assert p.alleles("c1", 1000, 1005) is not None


def test_ref_first_and_alt_order_kept(tmp_path):
    p = _panel(tmp_path, [("c1", 1000, "ACACAC", "ACACACACAC,AC,ACACAC" + "AC" * 20 + ",ACAC", "START=1001;END=1005"),
                          ("c1", 2000, "TTT", ".", "START=2001;END=2003")])
    assert p.alleles("c1", 1000, 1005) == (999, ["ACACAC", "ACACACACAC", "AC", "ACACAC" + "AC" * 20, "ACAC"])
    assert p.alleles("c1", 2000, 2003) == (1999, ["TTT"])             # ALT "." = no alternates


# ---- 4. the panel haplotype ------------------------------------------------------------------------------------
def _read_set(chrom_seq, lo, reads, region):
    raw = [dict(pos=a, end_pos=b, bases=chrom_seq[a - lo:b - lo], cigar=[("=", b - a)], sample=0) for a, b in reads]
    return _lib.ReadSet(raw, 1, region[0], region[1], chrom_seq, lo)


def _chrom(n, seed=3):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


def test_vcf_haplotype_blocks_by_hand():
    lo, chrom_len = 1000, 100_000
    seq = _chrom(1200)
    ref = seq[1400 - lo:1430 - lo]
    alts = [b"ac" * 20, ref[:10], ref + b"GGGG"]
    # reads far beyond the repeat: the flanks are the reference's 35 bp
    rs = _read_set(seq, lo, [(1050, 1800), (1060, 1790)], (1400, 1430))
    hb = rs.build_vcf_haplotype(1400, [ref.decode()] + [a.decode() for a in alts], 2, lo, chrom_len)
    assert hb["failure"] == "" and hb["unplaced_reads"] == 0
    b = hb["blocks"]
    assert [(x["start"], x["end"], x["is_repeat"], x["period"]) for x in b] == [(1365, 1400, False, 0), (1400, 1430, True, 2), (1430, 1465, False, 0)]
    assert b[0]["alleles"] == [seq[365:400]] and b[2]["alleles"] == [seq[430:465]]
    assert b[1]["alleles"] == [ref, b"AC" * 20, ref[:10], ref + b"GGGG"]        # uppercased, panel order, nothing added or dropped
    # reads that end near the repeat: the flanks stop at the reads' bounds (an alignment's stop is its last base), but keep 10 bp
    rs2 = _read_set(seq, lo, [(1380, 1460), (1385, 1455)], (1400, 1430))
    b2 = rs2.build_vcf_haplotype(1400, [ref.decode(), "AC"], 2, lo, chrom_len)["blocks"]
    assert [(x["start"], x["end"]) for x in b2] == [(1380, 1400), (1400, 1430), (1430, 1459)]
    rs3 = _read_set(seq, lo, [(1395, 1433)], (1400, 1430))
    b3 = rs3.build_vcf_haplotype(1400, [ref.decode(), "AC"], 2, lo, chrom_len)["blocks"]
    assert [(x["start"], x["end"]) for x in b3] == [(1390, 1400), (1400, 1430), (1430, 1440)]
    assert b3[0]["alleles"] == [seq[390:400]] and b3[2]["alleles"] == [seq[430:440]]


def test_vcf_haplotype_failures():
    lo = 0
    seq = _chrom(3000)
    rs = _read_set(seq, lo, [(1000, 2000)], (1400, 1430))
    ref = seq[1400:1430].decode()
    bad_ref = ("C" if ref[3] != "C" else "G").join((ref[:3], ref[4:]))
    assert rs.build_vcf_haplotype(1400, [bad_ref, "AC"], 2, lo, 3000)["failure"] == "The reference VCF's REF allele does not match the reference sequence"
    assert rs.build_vcf_haplotype(1400, [ref.lower(), "AC"], 2, lo, 3000)["blocks"] is not None      # (case does not matter)
    for sym in ("<INS>", "*", "<CN0>", "A[c1:100["):
        hb = rs.build_vcf_haplotype(1400, [ref, "AC", sym], 2, lo, 3000)
        assert hb["blocks"] is None and hb["failure"].startswith(f"Symbolic allele {sym}")
    assert rs.build_vcf_haplotype(1400, ["<DEL>", "AC"], 2, lo, 3000)["failure"].startswith("Symbolic allele <DEL>")
    # an ALT "<DEL>" is the block allele with no bases, as the VCF record writes it (get_alleles)
    assert rs.build_vcf_haplotype(1400, [ref, "<DEL>", "AC"], 2, lo, 3000)["blocks"][1]["alleles"] == [ref.encode(), b"", b"AC"]
    near = "Haplotype blocks are too near to the chromosome ends"
    rs0 = _read_set(seq, lo, [(0, 200)], (34, 60))
    assert rs0.build_vcf_haplotype(34, [seq[34:60].decode(), "A"], 1, lo, 3000)["failure"] == near
    assert rs0.build_vcf_haplotype(35, [seq[35:60].decode(), "A"], 1, lo, 3000)["failure"] == ""
    assert rs.build_vcf_haplotype(1400, [ref, "AC"], 2, lo, 1430 + 35)["failure"] == near              # region_end + 35 >= length
    assert rs.build_vcf_haplotype(1400, [ref, "AC"], 2, lo, 1430 + 36)["failure"] == ""
