"""A second restatement of the reference's SNP phasing priors for reads without mates, written from create_snp_trees
(src/snp_tree.cpp:9-15, :25-113, without a tracker), VCF::Variant (src/vcf_reader.h:67-71, vcf_reader.cpp:31-73, :108-111) and
calc_het_snp_factors (src/snp_phasing_quality.cpp:4-120); it does not call the library, except that the two base-quality tables
are handed in (the library's hook gives them, and they are pinned to the compiled reference on their own).  Where it follows
include/ltr_snp.h rather than the reference is named there: '*' and symbolic ALTs are no SNPs, calls of other than two alleles are
skipped, ties in position keep file order, and what ends the reference's run is an error code.

Also the hand-made cases: one read per branch of the CIGAR walk, one record per rule of the record filter."""
import re

import numpy as np

OK, INVALID, CIGAR = 0, -1, -5
MIN_Q, MAX_Q = ord("!"), ord("J")
HEADER = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


class SnpDie(Exception):
    """Where the reference ends the run (printErrorAndDie, .at(), assert) or reads past its arrays."""

    def __init__(self, code, text=""):
        super().__init__(text)
        self.code = code


# ---- the record side ------------------------------------------------------------------------------------------------------------
def build_set(header_line, lines, skip_regions=(), padding=15):
    """dict(samples=[column names], index={name: column}, snps=[[(pos0, base_one, base_two)...] per column], n_valid)."""
    head = header_line.rstrip("\r\n").split("\t")
    if len(head) < 8 or head[0] != "#CHROM" or (len(head) > 8 and head[8] != "FORMAT"):
        raise SnpDie(INVALID, "header")
    samples = head[9:]
    index = {}
    for column, name in enumerate(samples):                      # sample_indices_[name] = i: a later column replaces an earlier one
        index[name] = column
    per_column = [[] for _ in samples]
    n_valid = 0
    for line in lines:
        line = line.rstrip("\r\n")
        if not line:
            continue
        f = line.split("\t")
        if len(f) < 8 or not re.fullmatch(r"[0-9]+", f[1]) or not 1 <= int(f[1]) < 2 ** 31:
            raise SnpDie(INVALID, "columns / POS")
        pos = int(f[1])
        alleles = [f[3]] + ([] if f[4] == "." else f[4].split(","))
        calls = []                                               # per column (gt_a, gt_b) of a usable call, else None
        if samples:
            keys = f[8].split(":") if len(f) > 8 else []
            if "GT" not in keys or len(f) < 9 + len(samples):
                raise SnpDie(INVALID, f"POS {pos}")
            at = keys.index("GT")
            for field in f[9:9 + len(samples)]:
                sub = field.split(":")
                if at >= len(sub):
                    calls.append(None)
                    continue
                parts = re.split(r"([/|])", sub[at])             # allele, separator, allele, ...
                gt = []
                for a in parts[0::2]:
                    if a == ".":
                        gt.append(None)
                    elif re.fullmatch(r"[0-9]{1,6}", a):
                        if int(a) >= len(alleles):
                            raise SnpDie(INVALID, f"POS {pos}")
                        gt.append(int(a))
                    else:
                        raise SnpDie(INVALID, f"POS {pos}")
                usable = len(gt) == 2 and None not in gt and parts[1] == "|"       # bcf_gt_is_phased of the SECOND allele
                calls.append((gt[0], gt[1]) if usable else None)
        if len(alleles) != 2 or any(len(a) != 1 or a in "*." for a in alleles):    # is_biallelic_snp
            continue
        if any(pos >= start - padding and pos <= stop + padding for start, stop in skip_regions):   # in_any_region
            continue
        n_valid += 1
        for column, c in enumerate(calls):
            if c is not None and c[0] != c[1]:
                per_column[column].append((pos - 1, alleles[c[0]][0], alleles[c[1]][0]))
    return dict(samples=samples, index=index, snps=[sorted(v, key=lambda s: s[0]) for v in per_column], n_valid=n_valid)   # (sorted is stable)


# ---- the read side --------------------------------------------------------------------------------------------------------------
def quality_index(byte):
    q = byte - 256 if byte > 127 else byte                       # `char` is signed where the reference is built
    return 0 if q < MIN_Q else MAX_Q - MIN_Q if q > MAX_Q else q - MIN_Q


def extract(read, snps):
    """extract_bases_and_qualities: [(base byte, quality byte) or None for '-'] per SNP."""
    out, pos, base_index, k, c = [], read["pos"], 0, 0, 0
    bases, quals, cigar = read["bases"], read["quals"], read["cigar"]
    while k < len(snps) and c < len(cigar):
        op, n = cigar[c]
        if op in "M=X":
            if snps[k][0] < pos + n:
                at = snps[k][0] - pos + base_index
                if not 0 <= at < len(bases):
                    raise SnpDie(INVALID, ".at()")
                out.append((bases[at], quals[at]))
                k += 1
            else:
                pos, base_index, c = pos + n, base_index + n, c + 1
        elif op == "D":
            if snps[k][0] < pos + n:
                out.append(None)
                k += 1
            else:
                pos, c = pos + n, c + 1
        elif op == "I":
            base_index, c = base_index + n, c + 1
        elif op == "S":
            if snps[k][0] < pos:                                 # (never true for SNPs at or right of the read's start: kept as the reference has it)
                out.append(None)
                k += 1
            else:
                base_index, c = base_index + n, c + 1
        elif op == "H":
            c += 1
        else:
            raise SnpDie(CIGAR, "Invalid CIGAR option encountered")
    if k != len(snps):
        raise SnpDie(INVALID, "assert")
    return out


def read_priors(snps, read, log_correct, log_error):
    """add_log_phasing_probs from 0.0: (log_p1, log_p2, [p1 matches, p2 matches, mismatches])."""
    mine = [s for s in snps if read["pos"] <= s[0] <= read["end_pos"] - 1]
    p1, p2, n = 0.0, 0.0, [0, 0, 0]
    if mine:
        for s, got in zip(mine, extract(read, mine)):
            if got is None:
                continue
            q = quality_index(got[1])
            if got[0] == ord(s[1]):
                p1, p2 = p1 + float(log_correct[q]), p2 + float(log_error[q])
                n[0] += 1
            elif got[0] == ord(s[2]):
                p1, p2 = p1 + float(log_error[q]), p2 + float(log_correct[q])
                n[1] += 1
            else:
                p1, p2 = p1 + float(log_error[q]), p2 + float(log_error[q])
                n[2] += 1
    return p1, p2, n


def priors(snp_set, column, reads, tables):
    """(log_p1[], log_p2[], counts[3]) of one sample's reads; column < 0: zeros."""
    p1, p2, counts = np.zeros(len(reads)), np.zeros(len(reads)), [0, 0, 0]
    if column >= 0:
        for i, r in enumerate(reads):
            p1[i], p2[i], n = read_priors(snp_set["snps"][column], r, *tables)
            counts = [a + b for a, b in zip(counts, n)]
    return p1, p2, counts


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------
def parse_cigar(text):
    return [(op, int(n)) for n, op in re.findall(r"([0-9]+)([A-Za-z=])", text)]


def make_read(pos, cigar, bases=None, quals=None, end_pos=None):
    cig = parse_cigar(cigar)
    n_query = sum(n for op, n in cig if op in "M=XIS")
    if bases is None:
        bases = bytes(b"ACGT"[i % 4] for i in range(n_query))
    if quals is None:
        quals = bytes(MIN_Q + (7 * i + 3) % 42 for i in range(len(bases)))
    if end_pos is None:
        end_pos = pos + sum(n for op, n in cig if op in "M=XDN")
    return dict(pos=pos, end_pos=end_pos, bases=bytes(bases), quals=bytes(quals), cigar=cig)


def snp_lines(snps, chrom="chr1"):
    """One-sample record lines, `0|1`, for SNPs (pos0, base_one, base_two)."""
    return [f"{chrom}\t{p + 1}\t.\t{a}\t{b}\t.\t.\t.\tGT\t0|1" for p, a, b in snps]


def read_cases():
    """[(name, snps of the one sample, [reads], want)]: want = (status, [p1 matches, p2 matches, mismatches] or None).
    Reads start at 100 and hold ACGTACGT... unless said otherwise."""
    R = make_read
    return [
        # SNPs in the first and last base of an M run = at pos and at end_pos - 1; those at pos - 1 and end_pos are not taken
        ("m_first_last", [(99, "A", "C"), (100, "A", "G"), (109, "T", "C"), (110, "A", "C")], [R(100, "10M")], (OK, [1, 1, 0])),
        # M 100-104, D 105-107, M 108-112: the SNPs in the D give '-', the ones either side are read
        ("snp_in_d", [(104, "A", "C"), (105, "A", "C"), (107, "G", "T"), (108, "G", "C")], [R(100, "5M3D5M")], (OK, [1, 1, 0])),
        # M 100-103, I of 2, M 104-109: 106 is base 4 + 2 + 2 = 8 ('A')
        ("i_before", [(103, "T", "A"), (106, "A", "T")], [R(100, "4M2I6M")], (OK, [2, 0, 0])),
        # 3 clipped bases come first: 100 is base 3 ('T'), 107 is base 10 ('G'); the trailing clip is never reached
        ("soft_clips", [(100, "T", "A"), (107, "C", "G")], [R(100, "3S8M2S")], (OK, [1, 1, 0])),
        ("hard_clips", [(104, "C", "A")], [R(100, "2H10M3H")], (OK, [0, 1, 0])),
        # 104 is the X ('A', neither G nor T)
        ("eq_and_x", [(101, "C", "A"), (104, "G", "T"), (109, "C", "T")], [R(100, "4=1X5=")], (OK, [2, 0, 1])),
        # qualities below '!' (a blank, and a byte above 127, negative as a char), above 'J', and the ends of the table
        ("quality_range", [(100 + i, "ACGT"[i % 4], "ACGT"[(i + 1) % 4]) for i in range(8)],
         [R(100, "8M", quals=bytes([0x20, 0x90, ord("K"), ord("~"), ord("!"), ord("J"), ord('"'), ord("I")]))], (OK, [8, 0, 0])),
        # two SNPs at one position, after another one, keep file order: the sums of the two orders differ in the last bit
        ("two_at_one_position", [(100, "A", "C"), (102, "G", "A"), (102, "T", "G")], [R(100, "6M", quals=b"7I#8+D")], (OK, [2, 1, 0])),
        ("no_snp_at_all", [(50, "A", "C"), (200, "A", "C")], [R(100, "6M")], (OK, [0, 0, 0])),
        ("no_snps_in_set", [], [R(100, "6M"), R(300, "2S6M")], (OK, [0, 0, 0])),
        ("n_before_last_snp", [(101, "C", "A"), (116, "A", "C")], [R(100, "4M10N4M")], (CIGAR, None)),
        ("n_after_last_snp", [(101, "C", "A")], [R(100, "4M10N4M")], (OK, [1, 0, 0])),
        ("p_before_last_snp", [(106, "A", "C")], [R(100, "4M2P4M")], (CIGAR, None)),
        ("bases_shorter_than_cigar", [(108, "A", "C")], [R(100, "10M", bases=b"ACGTA", quals=b"IIIII")], (INVALID, None)),
        ("cigar_shorter_than_end_pos", [(107, "A", "C")], [R(100, "5M", end_pos=110)], (INVALID, None)),
        # several reads of a sample in one call: the counters add up, a read without SNPs stays at zero
        ("three_reads", [(104, "A", "C"), (120, "A", "C"), (131, "T", "G")],
         [R(100, "10M"), R(110, "4S12M"), R(118, "6M2D6M3I4M"), R(400, "9M")], (OK, [2, 0, 2])),
    ]


SKIP = [(1000, 1040)]                                            # with padding 15: POS 985 .. 1055 hold no SNP


def record_cases():
    """[(name, header line, record lines, skip regions, want)]: want = (status, n_valid, [SNPs per column]) or (status, POS)."""
    two, dup = HEADER + "\tS1\tS2", HEADER + "\tS1\tS1"
    rec = lambda pos, ref, alt, fmt, *calls: "\t".join(["chr1", str(pos), ".", ref, alt, ".", "PASS", ".", fmt] + list(calls))
    return [
        ("calls", two, [rec(100, "A", "C", "GT", "0|1", "1|0"), rec(101, "A", "C", "GT", "0/1", "1|1"), rec(102, "G", "T", "GT", ".|1", "."),
                        rec(103, "G", "T", "GT", "1", "0|1"), rec(104, "G", "T", "GT", "0|1|1", "./."), rec(105, "C", "T", "GT", "0|0", "1/0")],
         SKIP, (OK, 6, [[(99, "A", "C")], [(99, "C", "A"), (102, "G", "T")]])),
        ("gt_not_first", two, [rec(100, "A", "C", "DP:GT:GQ", "12:0|1:40", "7:1|0"), rec(101, "A", "G", "DP:GT", "5", "3:.|.")],
         SKIP, (OK, 2, [[(99, "A", "C")], [(99, "C", "A")]])),
        ("not_snps", two, [rec(100, "A", "C,G", "GT", "1|2", "0|2"), rec(101, "AT", "A", "GT", "0|1", "0|1"), rec(102, "A", "AT", "GT", "0|1", "0|1"),
                           rec(103, "A", "*", "GT", "0|1", "0|1"), rec(104, "A", "<X>", "GT", "0|1", "0|1"), rec(105, "A", "<*>", "GT", "0|1", "0|1"),
                           rec(106, "A", ".", "GT", "0|0", "0|0"), rec(107, "G", "C", "GT", "0|1", "0|0")],
         SKIP, (OK, 1, [[(106, "G", "C")], []])),
        ("skip_region_edges", two, [rec(984, "A", "C", "GT", "0|1", "0|1"), rec(985, "A", "G", "GT", "0|1", "0|1"), rec(1020, "A", "G", "GT", "0|1", "0|1"),
                                    rec(1055, "A", "T", "GT", "0|1", "0|1"), rec(1056, "C", "T", "GT", "0|1", "1|0")],
         SKIP, (OK, 2, [[(983, "A", "C"), (1055, "C", "T")], [(983, "A", "C"), (1055, "T", "C")]])),
        ("no_skip_regions", two, [rec(985, "A", "G", "GT", "0|1", "0|0")], [], (OK, 1, [[(984, "A", "G")], []])),
        ("duplicate_sample_name", dup, [rec(100, "A", "C", "GT", "0|1", "0|0"), rec(101, "A", "G", "GT", "0|0", "1|0")],
         SKIP, (OK, 2, [[(99, "A", "C")], [(100, "G", "A")]])),
        ("ties_keep_file_order", two, [rec(100, "A", "C", "GT", "0|1", "0|0"), rec(100, "A", "G", "GT", "1|0", "0|0"), rec(100, "A", "T", "GT", "0|1", "0|0")],
         SKIP, (OK, 3, [[(99, "A", "C"), (99, "G", "A"), (99, "A", "T")], []])),
        ("no_samples", HEADER[:HEADER.rindex("\t")], ["chr1\t100\t.\tA\tC\t.\t.\t."], SKIP, (OK, 1, [])),
        ("empty_window", two, [], SKIP, (OK, 0, [[], []])),
        ("too_few_columns", two, [rec(100, "A", "C", "GT", "0|1", "0|1"), rec(2345, "A", "C", "GT", "0|1")], SKIP, (INVALID, 2345)),
        ("allele_index_2", two, [rec(3456, "A", "C", "GT", "0|2", "0|1")], SKIP, (INVALID, 3456)),
        ("no_gt_key", two, [rec(4567, "A", "C", "DP", "3", "4")], SKIP, (INVALID, 4567)),
        ("no_gt_key_in_an_indel", two, [rec(5678, "AT", "A", "DP", "3", "4")], SKIP, (INVALID, 5678)),   # a Variant is built before it is judged
        ("unreadable_gt", two, [rec(6789, "A", "C", "GT", "0|x", "0|1")], SKIP, (INVALID, 6789)),
    ]
