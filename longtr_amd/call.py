"""Region file in, VCF out: the reference's locus loop over this library's entry points.

    python -m longtr_amd.call --bams a.bam,b.bam --fasta ref.fa --regions regions.bed --tr-vcf out.vcf.gz

genotype_regions() is BamProcessor::process_regions (src/bam_processor.cpp:536-628) + process_reads / process_phased_reads +
the gates of GenotyperBamProcessor::analyze_reads_and_phasing (src/genotyper_bam_processor.cpp:227-312) for the path the library
covers: unpaired (long) reads, the reference's fixed stutter model.  The phasing priors of a read come from its HP tag
(--phased-bam), from the heterozygous SNPs of a phased SNP VCF it overlaps (--phased-snps, the reference's --snp-vcf:
include/ltr_snp.h) or are zero.  The read filter is ltr_filter_reads (include/ltr_filter.h).  The filter, the gates and the SNP
priors are restatements: they cannot be pinned to the compiled reference, because these units include htslib.  Options carry the reference's names (hipstr_main.cpp:140-190) and defaults.
"""
import argparse
import queue
import sys
import threading
import time

import numpy as np

from . import _abi
from ._filter import filter_options, filter_reads
from ._formats import Bam, Fasta, VcfPanel, VcfWriter, read_regions, vcf_header
from ._haplotypes import ReadSet
from ._host import phasing_priors
from ._loader import LtrError
from ._snp import PhasedSnps

MAX_MATE_DIST = 1000      # bam_processor.h: the records of a region are fetched this far either side (:586-587)
CONTIG_END = 50           # bam_processor.cpp:580-583
REF_PAD = 400             # reference window either side of a region: left_align_reads cuts reads to region -+ 200, the record and the
                          # haplotype flanks read up to 200 beyond that
STAGES = ("bam", "filter", "left_align", "haplotypes", "alignment", "genotype", "records")

# the options of the reference this driver does not serve, each with its sentence
REFUSED = {
    "snp_vcf": "--snp-vcf is not taken under that name: give the same file to --phased-snps.",
    "fam": "--fam is not supported: pedigree-based filtering of SNP phasing is out of scope.",
    "pass_bam": "--pass-bam is not supported: this driver writes no BAM files.",
    "filt_bam": "--filt-bam is not supported: this driver writes no BAM files.",
    "viz_out": "--viz-out is not supported: the alignment visualisation output is out of scope.",
}
CRAM_REFUSAL = "CRAM input is not supported: convert to BAM with a .bai index."

DEFAULTS = dict(chrom=None, phased_bam=False, haploid_chrs=(), bam_samps=None, bam_libs=None, ref_vcf=None, min_mapq=20, min_mean_qual=30.0,
                max_tr_len=1000, min_reads=10, max_reads=1000000, max_haps=1000, indel_flank_len=5, alignment_params=None, stutter_align_len=0,
                output_gls=False, output_pls=False, output_phased_gls=False, output_filters=False, alleles="exact", chunk_loci=1024,
                chunk_read_bytes=256 << 20, overlap=True, full_command="longtr_amd.call", require_spanning=1, min_flank=5, sample_ploidy=None, phased_snps=None)


# ---- the reference sequence ---------------------------------------------------------------------------------------------------
class FastaReference:
    """A FASTA path through ltr_fasta_*: fetch(chrom, start, end) 0-based with end INCLUSIVE (FastaReader::get_sequence), clamped to
    the sequence; length(chrom) (-1 = unknown); contig_lines().  Any object with these three methods serves as `reference`."""

    def __init__(self, path):
        self.path, self._fa = path, Fasta(path)

    def fetch(self, chrom, start, end):
        return self._fa.fetch(chrom, start, end)

    def length(self, chrom):
        return self._fa.seq_len(chrom)

    def contig_lines(self):
        return self._fa.contig_lines()

    def close(self):
        self._fa.close()


class DictReference:
    """The same three methods over sequences held in memory: {chrom: sequence}."""

    path = "(sequences in memory)"

    def __init__(self, seqs):
        self.seqs = dict(seqs)

    def fetch(self, chrom, start, end):
        return self.seqs[chrom][max(int(start), 0):max(int(end) + 1, 0)]

    def length(self, chrom):
        return len(self.seqs[chrom]) if chrom in self.seqs else -1

    def contig_lines(self):
        return "".join(f"##contig=<ID={c},length={len(s)}>\n" for c, s in self.seqs.items())


def reference_window(reference, chrom, start, stop, chrom_len):
    """(lo, bases of [lo, hi)) with lo = start - REF_PAD, hi = stop + REF_PAD clamped to the contig: what ltr_left_align_reads,
    the haplotype builders and ltr_vcf_locus read for a region -- not the whole chromosome."""
    lo, hi = max(start - REF_PAD, 0), min(stop + REF_PAD, chrom_len)
    seq = reference.fetch(chrom, lo, hi - 1)
    return lo, seq.encode() if isinstance(seq, str) else bytes(seq)


# ---- samples ------------------------------------------------------------------------------------------------------------------
def sample_columns(read_groups, bam_samps=None, n_files=None):
    """The VCF's columns: the sorted unique sample names of all inputs (hipstr_main.cpp:463-515, a std::set;
    genotyper_bam_processor.h:195-199) -- the SM of every @RG line, or the names of --bam-samps."""
    if bam_samps is not None:
        if n_files is not None and len(bam_samps) != n_files:
            raise LtrError(_abi.LTR_ERR_INVALID, "Number of BAM/CRAM files in --bams and samples in --bam-samps must match")
        return sorted(set(bam_samps), key=lambda s: s.encode())
    if n_files is not None:
        for f in range(n_files):
            if not any(g["file"] == f for g in read_groups):
                raise LtrError(_abi.LTR_ERR_INVALID, "Provided BAM/CRAM files don't contain read groups in the header and the --bam-samps flag was not specified")
    return sorted({g["sample"] for g in read_groups}, key=lambda s: s.encode())


# ---- ploidy -------------------------------------------------------------------------------------------------------------------
def read_sample_ploidy(source, samples=None):
    """{(sample, chrom): 1 | 2} of --sample-ploidy: a path to tab-separated lines `sample  chrom  ploidy` (# starts a comment, blank
    lines are skipped) or such a dict.  A ploidy other than 1 or 2, a malformed line, or -- with `samples`, the VCF's columns -- a
    sample none of the inputs holds raise LtrError(LTR_ERR_INVALID).  A pair named twice keeps its last value."""
    bad = lambda text: LtrError(_abi.LTR_ERR_INVALID, "--sample-ploidy: " + text)
    table = {}
    if source is None:
        return table
    if isinstance(source, dict):
        rows = [(f"entry {k!r}", k, v) for k, v in source.items()]
        for where, k, _ in rows:
            if not (isinstance(k, tuple) and len(k) == 2 and all(isinstance(x, str) and x for x in k)):
                raise bad(f"{where}: a key is (sample, chrom)")
    else:
        rows = []
        with open(source) as fh:
            for n, line in enumerate(fh, 1):
                text = line.split("#", 1)[0].strip()
                if not text:
                    continue
                cols = text.split("\t")
                if len(cols) != 3 or not all(c.strip() for c in cols):
                    raise bad(f"{source}:{n}: expected `sample<TAB>chrom<TAB>ploidy`, got {line.rstrip()!r}")
                rows.append((f"{source}:{n}", (cols[0].strip(), cols[1].strip()), cols[2].strip()))
    for where, key, val in rows:
        if str(val) not in ("1", "2") or isinstance(val, bool):
            raise bad(f"{where}: ploidy is 1 or 2, got {val!r} (leave a sample without a copy out of the BAM list)")
        if samples is not None and key[0] not in samples:
            raise bad(f"{where}: sample {key[0]!r} is in none of the BAMs (samples: {', '.join(samples)})")
        table[key] = int(val)
    return table


def sample_ploidy(table, haploid_chrs, sample, chrom):
    """1 or 2: the table's value for (sample, chrom); a pair it does not name is 1 on a chromosome of --haploid-chrs, else 2."""
    return table.get((sample, chrom), 1 if chrom in haploid_chrs else 2)


# ---- gates --------------------------------------------------------------------------------------------------------------------
# In the reference's order; each (counter, test(facts, options) -> status text or None).  A fact a gate needs and the locus does not
# have yet ends the walk: the gates before it have passed and the locus goes on to the stage that supplies it.
def _g_too_long(f, o):
    n = f["stop"] - f["start"]
    return f"reference allele length exceeds the threshold ({n} vs {o['max_tr_len']}): see --max-tr-len" if n > o["max_tr_len"] else None


def _g_contig_end(f, o):
    return "region within 50bp of the end of the contig" if f["start"] < CONTIG_END or f["stop"] + CONTIG_END >= f["chrom_len"] else None


def _g_too_few(f, o):
    return f"too few reads: TOTAL={f['n_reads']}, MIN={o['min_reads']}" if f["n_reads"] < o["min_reads"] else None


def _g_too_many(f, o):
    return f"too many reads: TOTAL={f['n_reads']}, MAX={o['max_reads']}" if f["too_many_reads"] else None


def _g_hap_failed(f, o):
    return (f["hap_failure"] or "haplotype construction failed") if not f["hap_built"] else None


def _g_too_many_haps(f, o):
    return f"too many candidate haplotypes (# Found = {f['n_haps']}, MAX = {o['max_haps']}): see --max-haps" if f["n_haps"] > o["max_haps"] else None


def _g_no_pair(f, o):
    return "a sample has no optimal haplotype pair" if f["missing_pair"] else None


GATES = (("too_long", ("start", "stop"), _g_too_long), ("contig_end", ("start", "stop", "chrom_len"), _g_contig_end),
         ("too_few_reads", ("n_reads",), _g_too_few), ("too_many_reads", ("n_reads", "too_many_reads"), _g_too_many),
         ("hap_failed", ("hap_built", "hap_failure"), _g_hap_failed), ("too_many_haps", ("n_haps",), _g_too_many_haps),
         ("no_optimal_pair", ("missing_pair",), _g_no_pair))
COUNTERS = tuple(g[0] for g in GATES) + ("genotype_success", "genotype_fail")


def apply_gates(facts, options):
    """(counter, status text) of the first gate that removes the locus, or None: bam_processor.cpp:566-571, :580-583,
    genotyper_bam_processor.cpp:231-238, :241-245, a failed haplotype construction, seq_stutter_genotyper.cpp:606-610, a sample
    without an optimal pair."""
    o = dict(DEFAULTS, **options)
    for counter, needs, test in GATES:
        if any(k not in facts for k in needs):
            return None
        text = test(facts, o)
        if text is not None:
            return counter, text
    return None


# ---- chunks -------------------------------------------------------------------------------------------------------------------
def iter_chunks(items, size_of, chunk_loci, chunk_read_bytes):
    """Lists of consecutive items: a chunk closes once it holds chunk_loci items or chunk_read_bytes bytes (size_of(item)),
    whichever comes first; None / 0 = no such limit.  An item is never split, so one larger than chunk_read_bytes is a chunk."""
    cur, nbytes = [], 0
    for it in items:
        cur.append(it)
        nbytes += size_of(it)
        if (chunk_loci and len(cur) >= chunk_loci) or (chunk_read_bytes and nbytes >= chunk_read_bytes):
            yield cur
            cur, nbytes = [], 0
    if cur:
        yield cur


def plan_chunks(sizes, chunk_loci, chunk_read_bytes):
    """[(first, end)...] of the chunks iter_chunks makes of loci with these read bytes."""
    out, k = [], 0
    for c in iter_chunks(list(sizes), lambda s: s, chunk_loci, chunk_read_bytes):
        out.append((k, k + len(c)))
        k += len(c)
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def verify_vcf_chromosomes(snps, chroms):
    """SNPBamProcessor::verify_vcf_chromosomes (snp_bam_processor.cpp:8-33): every chromosome of the region list is in the SNP
    VCF's index, or LtrError(LTR_ERR_INVALID) with the reference's message and its chr / no-chr hint."""
    for chrom in chroms:
        if snps.has_chromosome(chrom):
            continue
        text = (f"No entries for chromosome {chrom} found in the SNP VCF file\n\tPlease ensure that the chromosome names in your BED file "
                "match those in your SNP VCF file")
        for alt in ["chr" + chrom] + ([chrom[3:]] if len(chrom) > 3 and chrom.startswith("chr") else []):
            if snps.has_chromosome(alt):
                text += f"\n\tNOTE: Found chromosome {alt} in the VCF, but not chromosome {chrom}"
        raise LtrError(_abi.LTR_ERR_INVALID, text)


def _check_options(options):
    for k, text in REFUSED.items():
        if options.get(k):
            raise LtrError(_abi.LTR_ERR_UNSUPPORTED, text)
    unknown = [k for k in options if k not in DEFAULTS and k not in REFUSED]
    if unknown:
        raise TypeError(f"genotype_regions: unknown option(s) {', '.join(sorted(unknown))}")
    o = dict(DEFAULTS, **options)
    o["sample_ploidy"] = read_sample_ploidy(o["sample_ploidy"])   # (format errors here, before anything is opened; the samples are checked once the BAM headers are read)
    if o["alleles"] not in ("exact", "clustered", "consensus"):
        raise LtrError(_abi.LTR_ERR_INVALID, 'alleles is "exact", "clustered" or "consensus"')
    if o["ref_vcf"] and o["alleles"] != "exact":
        raise LtrError(_abi.LTR_ERR_INVALID, "--ref-vcf gives the candidate alleles: alleles must stay \"exact\"")
    return o


class _Prepared:
    """What the producer hands over for one locus: the report entry, and for a locus still alive its prepared reads."""

    def __init__(self, entry):
        self.entry, self.rs, self.reads, self.read_bytes = entry, None, None, 0


def _snp_priors(snps, reg, raw, sample_names, entry):
    """log_p1 / log_p2 of the passing raw reads from the phased SNPs within 1000 bp of the region (process_reads,
    snp_bam_processor.cpp:52-117), sample by sample, and the numbers of its two log lines as entry["snp_info"]."""
    p1, p2 = np.zeros(len(raw)), np.zeros(len(raw))
    found = 0
    with snps.handle.window(reg["chrom"], reg["start"], reg["stop"]) as snp_set:
        for k, name in enumerate(sample_names):
            mine = [j for j, r in enumerate(raw) if r["sample"] == k]
            column = snp_set.sample_index(name)
            found += column >= 0
            p1[mine], p2[mine] = snp_set.priors(column, [raw[j] for j in mine], snps.counts)
        n_valid = snp_set.n_valid_snps
    differ = p1 != p2
    entry["snp_info"] = dict(n_valid_snps=n_valid, samples_in_vcf=int(found), phased_reads=int(differ.sum()),
                             phased_samples=len({raw[j]["sample"] for j in np.flatnonzero(differ)}))
    return p1, p2


class _SnpSource:
    """The producer's side of --phased-snps: the open VCF, the match counters its calls add to, and the seconds they took."""

    def __init__(self, path):
        self.handle, self.counts, self.seconds = PhasedSnps(path), np.zeros(3, dtype=np.int32), 0.0


def _prepare(bam, reference, reg, chrom_len, o, samples_arg, fopt, stage, snps=None):
    """BAM seek + read, filter, reference fetch, left alignment and priors of one locus (the producer's side)."""
    entry = dict(chrom=reg["chrom"], start=reg["start"], stop=reg["stop"], name=reg["name"], status="ok", gate=None, n_records=0,
                 n_reads=0, samples=[], filter_counters=None)
    p = _Prepared(entry)
    facts = dict(start=reg["start"], stop=reg["stop"])
    p.facts = facts
    if reg["period"] < 1:
        entry["status"] = "motifs differ in length"            # (our rule: Region::computePeriod gave -1, nothing downstream takes it)
        return p
    facts["chrom_len"] = chrom_len
    gate = apply_gates(facts, o)
    if gate is None:
        t = time.perf_counter()
        recs = bam.fetch(reg["chrom"], max(0, reg["start"] - MAX_MATE_DIST), reg["stop"] + MAX_MATE_DIST, tags=("RG", "XA", "HP"))
        stage["bam"] += time.perf_counter() - t
        t = time.perf_counter()
        fr = filter_reads(recs, reg["start"], reg["stop"], fopt, **samples_arg)
        stage["filter"] += time.perf_counter() - t
        entry.update(n_records=len(recs), n_reads=len(fr["passing"]), samples=fr["samples"], filter_counters=fr["counters"])
        facts.update(n_reads=len(fr["passing"]), too_many_reads=fr["too_many_reads"])
        gate = apply_gates(facts, o)
    if gate is not None:
        entry["gate"], entry["status"] = gate
        return p
    lo, ref = reference_window(reference, reg["chrom"], reg["start"], reg["stop"], chrom_len)
    raw = []
    for i, s, pf in fr["passing"]:
        r = recs[i]
        raw.append(dict(pos=r["pos"], end_pos=r["end_pos"], bases=r["seq"].encode(), cigar=r["cigar"], sample=s, hp=r["HP"] if isinstance(r.get("HP"), int) else 0,
                        quals=r["qual"].encode("latin-1"), reverse=int(bool(r["flag"] & 16)), use_for_hap_generation=int(pf)))
    t = time.perf_counter()
    rs = ReadSet(raw, len(fr["samples"]), reg["start"], reg["stop"], ref, lo)
    stage["left_align"] += time.perf_counter() - t
    reads = rs.reads                                             # deleted reads stay, as in the reference (the 10-bp substitute is aligned)
    sample = [r["sample"] for r in reads]
    if o["phased_bam"]:                                          # process_phased_reads; otherwise both priors 0 (snp_bam_processor.cpp:93-103)
        hp = [raw[r["source"]]["hp"] for r in reads]
        p1, p2, _ = phasing_priors(sample, [h if h in (1, 2) else -1 for h in hp], len(fr["samples"]))
    elif snps is not None:                                       # process_reads: the priors of the raw reads, carried to what left alignment kept
        t = time.perf_counter()
        raw_p1, raw_p2 = _snp_priors(snps, reg, raw, fr["samples"], entry)
        source = [r["source"] for r in reads]
        p1, p2 = raw_p1[source], raw_p2[source]
        snps.seconds += time.perf_counter() - t
    else:
        p1, p2 = np.zeros(len(reads)), np.zeros(len(reads))
    p.rs, p.reads, p.read_bytes = rs, reads, sum(len(r["seq"]) for r in reads)
    p.region, p.ref, p.lo, p.chrom_len, p.sample, p.p1, p.p2, p.raw = reg, ref, lo, chrom_len, sample, p1, p2, raw
    entry["n_aligned_reads"] = len(reads)
    return p


def _build_haplotypes(ctx, live, o, panel):
    """Per live locus the dict of ReadSet.build_haplotype (+ inexact for the batched forms)."""
    ifl = o["indel_flank_len"]
    if panel is not None:
        out = []
        for p in live:
            rec = panel.alleles(p.region["chrom"], p.region["start"], p.region["stop"])
            out.append(dict(blocks=None, failure="no panel record") if rec is None else
                       p.rs.build_vcf_haplotype(rec[0], rec[1], p.region["period"], p.lo, p.chrom_len, ctx=ctx))
        return out
    if o["alleles"] == "exact":
        return [p.rs.build_haplotype(p.region["start"], p.region["stop"], p.region["period"], p.lo, p.chrom_len, ifl, ctx=ctx) for p in live]
    loci = [dict(rs=p.rs, region_start=p.region["start"], region_stop=p.region["stop"], period=p.region["period"], chrom_seq_start=p.lo,
                 chrom_len=p.chrom_len) for p in live]
    return ctx.build_haplotypes_consensus(loci, ifl) if o["alleles"] == "consensus" else ctx.build_haplotypes_clustered(loci, ifl)


def _gate(p, o, **facts):
    p.facts.update(facts)
    gate = apply_gates(p.facts, o)
    if gate is not None:
        p.entry["gate"], p.entry["status"] = gate
    return gate is not None


def _run_chunk(ctx, chunk, o, panel, columns, vopt, writer, stage, haploid_chrs):
    """Haplotypes, alignment, genotypes and records of one chunk (the calling thread: every GPU call is here)."""
    one_copy = lambda p: [sample_ploidy(o["sample_ploidy"], haploid_chrs, s, p.region["chrom"]) == 1 for s in p.entry["samples"]]
    live = [p for p in chunk if p.rs is not None]
    try:
        t = time.perf_counter()
        built = _build_haplotypes(ctx, live, o, panel) if live else []
        stage["haplotypes"] += time.perf_counter() - t
        todo = []
        for p, hb in zip(live, built):
            n_haps = int(np.prod([len(b["alleles"]) for b in hb["blocks"]], dtype=np.int64)) if hb["blocks"] is not None else 0
            if _gate(p, o, hap_built=hb["blocks"] is not None, hap_failure=hb["failure"], n_haps=n_haps):
                continue
            p.blocks, p.inexact = hb["blocks"], hb.get("inexact")
            p.alns = [dict(start=r["start"], stop=r["stop"], seq=r["seq"], cigar=r["cigar"]) for r in p.reads]
            todo.append(p)
        if not todo:
            return
        t = time.perf_counter()
        res = ctx.calc_hap_aln_probs([(p.blocks, p.alns, None) for p in todo])
        stage["alignment"] += time.perf_counter() - t
        fields = dict(want_gls=o["output_gls"], want_pls=o["output_pls"], want_phased_gls=o["output_phased_gls"])
        t = time.perf_counter()
        while todo:
            lro = np.zeros(len(todo) + 1, dtype=np.int64)
            lro[1:] = np.cumsum([len(p.alns) for p in todo])
            # The ploidy per locus as long as the samples of every locus are alike (the bytes of --haploid-chrs); a call with a
            # mixed locus carries the flags of every sample instead (its uniform loci take the per-locus path inside all the same).
            flags = [one_copy(p) for p in todo]
            mixed = any(len(set(f)) > 1 for f in flags)
            by_chrom = lambda p: p.region["chrom"] in haploid_chrs                # (a locus without a sample: what --haploid-chrs says, as before)
            ploidy = dict(sample_haploid=flags) if mixed else dict(locus_haploid=[f[0] if f else by_chrom(p) for f, p in zip(flags, todo)])
            result = ctx.genotype_ll([m for m, _ in res], [s for _, s in res], [p.blocks for p in todo], lro, np.concatenate([p.p1 for p in todo]),
                                     np.concatenate([p.p2 for p in todo]), np.concatenate([np.asarray(p.sample, dtype=np.int32) for p in todo]),
                                     [len(p.entry["samples"]) for p in todo], prune=panel is None, fields=fields, **ploidy)
            # a sample without an optimal pair (best_gts = -1) would make ltr_genotype_result_vcf_records refuse the whole call
            bad = [k for k, p in enumerate(todo) if _gate(p, o, missing_pair=bool((result.fields(k)["best_gts"] < 0).any()))]
            if not bad:
                break
            result.close()                                       # the loci are independent: genotype the others again without them
            todo, res = [p for k, p in enumerate(todo) if k not in bad], [r for k, r in enumerate(res) if k not in bad]
        else:
            return
        stage["genotype"] += time.perf_counter() - t
        t = time.perf_counter()
        with result:
            pvs, none = [], np.zeros(0)
            for k, p in enumerate(todo):
                g = result.locus(k)
                alleles = g["blocks"][1]["alleles"]
                inexact = np.zeros(len(alleles), dtype=np.uint8)
                if p.inexact is not None:                        # the candidates' flags, without the alleles that were pruned
                    inexact = np.asarray([x for a, x in enumerate(p.inexact) if a not in set(g["removed"][1])], dtype=np.uint8)
                reg = p.region
                pvs.append(_abi.PackedVcfLocus(dict(
                    chrom=reg["chrom"], region_start=reg["start"], region_stop=reg["stop"], name=reg["name"], motif=reg["motif"],
                    period_str=reg["period_str"], chrom_seq=p.ref, chrom_seq_start=p.lo, blocks=g["blocks"], block=1, inexact_allele=inexact,
                    log_aln_probs=none, log_p1=p.p1, log_p2=p.p2, sample_label=np.asarray(p.sample, dtype=np.int32), alns=p.alns,
                    aln_deleted=[r["deleted"] for r in p.reads], log_sample_posteriors=none, sample_total_ll=none,
                    best_haplotypes=np.zeros(0, dtype=np.int32), n_p1s=p.rs.n_p1s, n_p2s=p.rs.n_p2s, sample_names=p.entry["samples"],
                    haploid=all(one_copy(p)) if p.entry["samples"] else reg["chrom"] in haploid_chrs, out_sample_names=columns)))
                p.entry.update(n_haplotypes=int(g["n_haps"]), n_alleles=len(alleles))
            lines, pos = result.vcf_records(pvs, vopt)
        for p, line, ps in zip(todo, lines, pos):
            writer.add_record(p.region["chrom"], int(ps), line)
            p.entry["pos"] = int(ps)
        stage["records"] += time.perf_counter() - t
    finally:
        for p in live:
            p.rs.close()
            p.rs = None


def genotype_regions(ctx, bams, reference, regions, out_vcf, **options):
    """Genotype every region of a region file from indexed BAMs and write the VCF.

    ctx: a Context (the GPU).  bams: BAM paths, each with its .bai.  reference: a FASTA path (with its .fai), or any object with
    fetch(chrom, start, end) (0-based, end inclusive), length(chrom) and contig_lines().  regions: a region file (CHROM START STOP
    MOTIF [NAME], ltr_read_regions) or a list of the dicts read_regions gives.  out_vcf: the VCF (BGZF for *.gz).

    options, with the reference's names and defaults: chrom, phased_bam, haploid_chrs, sample_ploidy (ours: a path or {(sample, chrom):
    1 | 2}, the ploidy of a sample on a chromosome where it differs from what haploid_chrs says -- chrX of a cohort of men and women),
    phased_snps (the reference's snp_vcf under a name of ours: a bgzipped, tabix-indexed VCF of phased SNP genotypes of the samples; the
    priors of a read are those of the heterozygous SNPs it overlaps within 1000 bp of the region; with phased_bam the HP tags win and
    the file is not opened; every chromosome of the region list must be in its index), bam_samps, bam_libs (accepted; libraries are
    unused, duplicate removal is off in the reference, hipstr_main.cpp:383), ref_vcf, min_mapq 20, min_mean_qual 30, max_tr_len 1000,
    min_reads 10, max_reads 1000000, max_haps 1000, indel_flank_len 5, alignment_params (7 numbers), stutter_align_len 0, output_gls,
    output_pls, output_phased_gls, output_filters.  Ours: alleles = "exact" (ltr_build_haplotype) | "clustered" | "consensus" (the two
    batched forms); chunk_loci, chunk_read_bytes; overlap; full_command (the ##command line).

    Regions are taken in ltr_region_set_order order and worked in chunks.  A chunk closes at chunk_loci loci or chunk_read_bytes bytes
    of left-aligned reads, whichever comes first; the defaults, 1024 loci and 256 MB, are starting values nobody has measured.  With
    overlap=True ONE producer thread prepares chunk k + 1 (BAM reading, filter, left alignment, priors, reference fetch; the BAM
    handle is its alone) while the calling thread runs chunk k on the GPU (haplotypes, ltr_calc_hap_aln_probs,
    ltr_ll_genotype_ploidy with the fields request and prune = (ref_vcf is None), ltr_genotype_result_vcf_records, the writer).
    Only one chunk's loci are held at a time (two with overlap).  A chunk that fails leaves its error in the report and ends the
    run: no retries.

    Returns the report: loci (per locus chrom, start, stop, name, status, gate, n_records, n_reads, samples, filter_counters, ...),
    counters (the reference's summary: too_long, too_few_reads, too_many_reads, genotype_success, genotype_fail, and one per gate),
    columns, error (None or text), timing (stage_seconds over STAGES, timers = ltr_ctx_timers, wall_seconds, chunks).  With phased_snps:
    per locus snp_info (n_valid_snps in the window, samples_in_vcf, phased_reads, phased_samples), the counters snp_match and
    snp_mismatch, and timing["snp_seconds"] (part of the producer's time, beside STAGES); with phased_bam as well, only the key
    phased_snps, the sentence that the file was ignored."""
    o = _check_options(options)
    if isinstance(bams, str):
        bams = bams.split(",")
    if any(b.lower().endswith(".cram") for b in bams):
        raise LtrError(_abi.LTR_ERR_UNSUPPORTED, CRAM_REFUSAL)
    t_wall = time.perf_counter()
    own_ref = isinstance(reference, (str, bytes))
    ref = FastaReference(reference) if own_ref else reference
    regs = read_regions(regions, chrom_limit=o["chrom"], order=True)[0] if isinstance(regions, (str, bytes)) else \
        sorted((r for r in regions if not o["chrom"] or r["chrom"] == o["chrom"]), key=lambda r: (r["chrom"].encode(), r["start"], r["stop"]))
    bam = Bam(list(bams), merge_by_position=False)              # ORDER_ALNS_BY_FILE (bam_processor.cpp:193)
    panel = writer = snps = None
    stage, n_chunks = dict.fromkeys(STAGES, 0.0), 0
    report = dict(loci=[], counters=dict.fromkeys(COUNTERS, 0), columns=None, error=None, timing=None)
    if o["phased_snps"] and o["phased_bam"]:                     # the HP tags win and the file is never opened (hipstr_main.cpp:364-366)
        report["phased_snps"] = "Using phased BAM tags to genotype and phase TRs (WARNING: Any arguments provided to --phased-snps will be ignored)"
    elif o["phased_snps"]:                                       # an unusable file or a missing chromosome raises: nothing has been written yet
        try:
            snps = _SnpSource(o["phased_snps"])
            verify_vcf_chromosomes(snps.handle, dict.fromkeys(r["chrom"] for r in regs))
        except BaseException:
            for h in (snps and snps.handle, bam) + ((ref,) if own_ref else ()):
                if h is not None:
                    h.close()
            raise
    old_params = ctx.params
    try:
        read_groups = bam.read_groups()
        columns = sample_columns(read_groups, o["bam_samps"], len(bams))
        report["columns"] = columns
        read_sample_ploidy(o["sample_ploidy"], samples=columns)   # a sample none of the BAMs holds: an error before any work
        samples_arg = dict(file_samples=list(o["bam_samps"])) if o["bam_samps"] is not None else dict(read_groups=read_groups)
        bam_refs = dict(bam.refs())
        for chrom in dict.fromkeys(r["chrom"] for r in regs):    # verify_chromosomes (bam_processor.cpp:490-533)
            if ref.length(chrom) == -1:
                raise LtrError(_abi.LTR_ERR_INVALID, f"No sequence for chromosome {chrom} found in the FASTA file")
            if chrom not in bam_refs:
                raise LtrError(_abi.LTR_ERR_INVALID, f"No entries for chromosome {chrom} found in the BAM/CRAM(s)")
        fopt = filter_options(min_mapq=o["min_mapq"], min_mean_qual=o["min_mean_qual"], max_total_reads=o["max_reads"],
                              require_spanning=o["require_spanning"], min_flank=o["min_flank"])
        vopt = _abi.vcf_options(output_gls=int(o["output_gls"]), output_pls=int(o["output_pls"]), output_phased_gls=int(o["output_phased_gls"]),
                                output_filters=int(o["output_filters"]))
        prm = _abi.make_params([getattr(old_params, f) for f, _ in _abi.AlignParams._fields_[:7]] if o["alignment_params"] is None
                               else o["alignment_params"], o["indel_flank_len"], int(o["stutter_align_len"]))
        ctx.set_params(prm)
        panel = VcfPanel(o["ref_vcf"]) if o["ref_vcf"] else None
        writer = VcfWriter(out_vcf)
        writer.header(vcf_header(getattr(ref, "path", "") or "", o["full_command"], ref.contig_lines() or None, columns, vopt))
        haploid_chrs = set(o["haploid_chrs"].split(",") if isinstance(o["haploid_chrs"], str) else o["haploid_chrs"])

        def prepared():
            for reg in regs:
                p = _prepare(bam, ref, reg, ref.length(reg["chrom"]), o, samples_arg, fopt, stage, snps)
                p.entry["sample_ploidy"] = [sample_ploidy(o["sample_ploidy"], haploid_chrs, s, reg["chrom"]) for s in columns]
                yield p

        chunks = iter_chunks(prepared(), lambda p: p.read_bytes, o["chunk_loci"], o["chunk_read_bytes"])
        source = _ahead(chunks) if o["overlap"] else chunks
        try:
            for chunk in source:
                n_chunks += 1
                try:
                    _run_chunk(ctx, chunk, o, panel, columns, vopt, writer, stage, haploid_chrs)
                finally:
                    report["loci"] += [p.entry for p in chunk]
        finally:
            source.close()                                       # the producer has stopped before the BAM handle is closed below
    except Exception as e:                                       # the error stays in the report; the run ends here
        report["error"] = f"{type(e).__name__}: {e}"
    finally:
        ctx.set_params(old_params)
        for h in (writer, panel, snps and snps.handle, bam) + ((ref,) if own_ref else ()):
            if h is not None:
                h.close()
    for e in report["loci"]:
        g = e.get("gate")
        if g:
            report["counters"][g] += 1
        c = report["counters"]
        if e["status"] == "ok" and "pos" in e:
            c["genotype_success"] += 1
        elif g in ("hap_failed", "too_many_haps", "no_optimal_pair"):
            c["genotype_fail"] += 1
    report["timing"] = dict(stage_seconds=stage, timers=ctx.timers(), wall_seconds=time.perf_counter() - t_wall,
                            chunks=n_chunks if report["error"] is None else None)
    if snps is not None:                                         # match_count_ / mismatch_count_ of the reference, and the time of the SNP step
        report["counters"].update(snp_match=int(snps.counts[0] + snps.counts[1]), snp_mismatch=int(snps.counts[2]))
        report["timing"]["snp_seconds"] = snps.seconds
    return report


def _ahead(chunks):
    """The chunks of an iterator, each prepared by ONE producer thread while the consumer works on the one before."""
    q = queue.Queue(maxsize=1)
    stop = threading.Event()

    def produce():
        try:
            for c in chunks:
                while not stop.is_set():
                    try:
                        q.put(("chunk", c), timeout=0.1)
                        break
                    except queue.Full:
                        pass
                if stop.is_set():
                    for p in c:
                        if p.rs is not None:
                            p.rs.close()
                    return
            q.put(("end", None))
        except BaseException as e:                               # handed to the calling thread
            q.put(("error", e))

    t = threading.Thread(target=produce, name="ltr-call-producer", daemon=True)
    t.start()
    try:
        while True:
            kind, val = q.get()
            if kind == "end":
                return
            if kind == "error":
                raise val
            yield val
    finally:
        stop.set()
        while t.is_alive():                                      # let a producer blocked on the queue see the flag
            try:
                kind, val = q.get(timeout=0.05)
                if kind == "chunk":
                    for p in val:
                        if p.rs is not None:
                            p.rs.close()
            except queue.Empty:
                pass
        t.join()


# ---- the command line ---------------------------------------------------------------------------------------------------------
def make_parser():
    ap = argparse.ArgumentParser(prog="python -m longtr_amd.call", description="Genotype the tandem repeats of a region file from BAMs on the GPU "
                                 "(options as in LongTR).")
    ap.add_argument("--bams", required=True, metavar="<list_of_bams>", help="comma separated list of BAM files, each with its .bai")
    ap.add_argument("--fasta", required=True, metavar="<genome.fa>", help="FASTA file of the reference genome, with its .fai")
    ap.add_argument("--regions", required=True, metavar="<region_file.bed>", help="CHROM START STOP MOTIF [NAME] per line")
    ap.add_argument("--tr-vcf", required=True, metavar="<tr_gts.vcf.gz>", help="VCF to write (BGZF for *.gz)")
    ap.add_argument("--chrom", default=None, metavar="<chrom>", help="only consider regions on this chromosome")
    ap.add_argument("--phased-bam", action="store_true", help="use the reads' HP tags as phasing priors")
    ap.add_argument("--phased-snps", default=None, metavar="<phased_snps.vcf.gz>", help="Bgzipped input VCF file containing phased SNP genotypes for the samples "
                    "(LongTR's --snp-vcf), with its .tbi")
    ap.add_argument("--haploid-chrs", default="", metavar="<list_of_chroms>", help="comma separated list of chromosomes to treat as haploid")
    ap.add_argument("--sample-ploidy", default=None, metavar="<ploidy.tsv>", help="tab separated lines `sample chrom ploidy` (1 or 2, # comments): the copies of a "
                    "chromosome a sample has, e.g. chrX of a man; a pair not named is 1 on a chromosome of --haploid-chrs, else 2")
    ap.add_argument("--bam-samps", default=None, metavar="<list_of_samples>", help="comma separated list of samples in the same order as the BAM files")
    ap.add_argument("--bam-libs", default=None, metavar="<list_of_libraries>", help="accepted; libraries are unused (no duplicate removal)")
    ap.add_argument("--ref-vcf", default=None, metavar="<tr_ref_panel.vcf.gz>", help="bgzipped, tabix-indexed VCF of candidate alleles")
    ap.add_argument("--min-mapq", type=int, default=DEFAULTS["min_mapq"], metavar="<min_mapq>", help="minimum MAPQ of a read (default 20)")
    ap.add_argument("--min-mean-qual", type=float, default=DEFAULTS["min_mean_qual"], metavar="<min_qual>", help="minimum mean base quality of a read (default 30)")
    ap.add_argument("--max-tr-len", type=int, default=DEFAULTS["max_tr_len"], metavar="<max_bp>", help="only genotype repeats of at most this reference length (default 1000)")
    ap.add_argument("--min-reads", type=int, default=DEFAULTS["min_reads"], metavar="<num_reads>", help="minimum total reads to genotype a locus (default 10)")
    ap.add_argument("--max-reads", type=int, default=DEFAULTS["max_reads"], metavar="<num_reads>", help="skip a locus with more reads (default 1000000)")
    ap.add_argument("--max-haps", type=int, default=DEFAULTS["max_haps"], metavar="<max_haplotypes>", help="maximum candidate haplotypes of a locus (default 1000)")
    ap.add_argument("--indel-flank-len", type=int, default=DEFAULTS["indel_flank_len"], metavar="<max_bp>", help="flank indels this close to the repeat are part of it (default 5)")
    ap.add_argument("--alignment-params", default=None, metavar="<7 numbers>", help="comma separated transition log-probabilities of the alignment model")
    ap.add_argument("--stutter-align-len", type=int, default=DEFAULTS["stutter_align_len"], metavar="<threshold>", help="use the stutter alignment for homopolymers (default 0: off)")
    ap.add_argument("--output-gls", action="store_true", help="write the GL FORMAT field")
    ap.add_argument("--output-pls", action="store_true", help="write the PL FORMAT field")
    ap.add_argument("--output-phased-gls", action="store_true", help="write the PHASEDGL FORMAT field")
    ap.add_argument("--output-filters", action="store_true", help="write the FILTER FORMAT field")
    ap.add_argument("--alleles", choices=("exact", "clustered", "consensus"), default="exact", help="how candidate alleles are found (default exact)")
    ap.add_argument("--chunk-loci", type=int, default=DEFAULTS["chunk_loci"], help="loci per chunk (default 1024, unmeasured)")
    ap.add_argument("--chunk-read-bytes", type=int, default=DEFAULTS["chunk_read_bytes"], help="read bytes per chunk (default 256 MB, unmeasured)")
    ap.add_argument("--no-overlap", action="store_true", help="prepare and run chunks one after the other")
    ap.add_argument("--device", type=int, default=0, help="GPU to use (default 0)")
    for name in ("--snp-vcf", "--fam", "--pass-bam", "--filt-bam", "--viz-out"):
        ap.add_argument(name, default=None, help=argparse.SUPPRESS)
    return ap


def options_from_args(args):
    """The keyword options of genotype_regions for parsed arguments; a refused option ends the parse with its sentence."""
    for k, text in REFUSED.items():
        if getattr(args, k, None):
            raise LtrError(_abi.LTR_ERR_UNSUPPORTED, text)
    if any(b.lower().endswith(".cram") for b in args.bams.split(",")):
        raise LtrError(_abi.LTR_ERR_UNSUPPORTED, CRAM_REFUSAL)
    split = lambda s: None if s is None else s.split(",")
    return dict(chrom=args.chrom, phased_bam=args.phased_bam, phased_snps=args.phased_snps, haploid_chrs=tuple(c for c in args.haploid_chrs.split(",") if c),
                bam_samps=split(args.bam_samps), bam_libs=split(args.bam_libs), ref_vcf=args.ref_vcf, min_mapq=args.min_mapq,
                min_mean_qual=args.min_mean_qual, max_tr_len=args.max_tr_len, min_reads=args.min_reads, max_reads=args.max_reads,
                max_haps=args.max_haps, indel_flank_len=args.indel_flank_len,
                alignment_params=None if args.alignment_params is None else [float(x) for x in args.alignment_params.split(",")],
                stutter_align_len=args.stutter_align_len, output_gls=args.output_gls, output_pls=args.output_pls,
                output_phased_gls=args.output_phased_gls, output_filters=args.output_filters, alleles=args.alleles, chunk_loci=args.chunk_loci,
                chunk_read_bytes=args.chunk_read_bytes, overlap=not args.no_overlap, sample_ploidy=read_sample_ploidy(args.sample_ploidy) or None)


def main(argv=None):
    ap = make_parser()
    args = ap.parse_args(argv)
    try:
        options = options_from_args(args)
    except LtrError as e:
        ap.error(str(e))
    if options["sample_ploidy"]:                                 # its samples against the BAM headers, before a GPU is opened
        try:
            bam = Bam(args.bams.split(","), merge_by_position=False)
            try:
                read_sample_ploidy(options["sample_ploidy"], samples=sample_columns(bam.read_groups(), options["bam_samps"], len(args.bams.split(","))))
            finally:
                bam.close()
        except LtrError as e:
            ap.error(str(e))
    from ._context import Context
    ctx = Context(args.device)
    try:
        report = genotype_regions(ctx, args.bams.split(","), args.fasta, args.regions, args.tr_vcf,
                                  full_command="longtr_amd.call " + " ".join(sys.argv[1:] if argv is None else argv), **options)
    finally:
        ctx.close()
    c = report["counters"]
    for e in report["loci"]:
        if e["status"] != "ok":
            print(f"{e['chrom']}:{e['start']}-{e['stop']} {e['name']}: skipped: {e['status']}", file=sys.stderr)
    print(f"Genotyping succeeded for {c['genotype_success']}/{c['genotype_success'] + c['genotype_fail']} loci; skipped: {c['too_long']} too long, "
          f"{c['too_few_reads']} with too few reads, {c['too_many_reads']} with too many reads", file=sys.stderr)
    if report["error"]:
        print("ERROR: " + report["error"], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
