"""The whole chain on REAL reads: the reference's bundled HiFi BAMs of the HG002 / HG003 / HG004 trio
(test_data/*.bam) at the loci of its bundled BED, through this library only:

  BED text           -> ltr_read_regions            (the bundled file puts the motif in column 7: converted first)
  BAM + BAI          -> ltr_bam_*                   (no htslib)
  reference sequence -> rebuilt from the reads      (hg38 is not bundled: HiFi CIGARs are =/X/I/D, so every
                                                     base some read matches ('=') is known; see rebuild_reference)
  left_align_reads   -> ltr_left_align_reads
  candidate alleles  -> ltr_build_haplotype         (exact alleles, no POA)
                        or, with --ref-vcf, ltr_vcf_read_alleles + ltr_build_vcf_haplotype (a bgzipped, tabix-indexed
                        panel's alleles in the panel's order; ltr_vcf_index writes the index)
  read x haplotype   -> ltr_calc_hap_aln_probs      (GPU; every locus in one call)
  phasing priors     -> ltr_phasing_priors          (the HP tags, process_phased_reads' rule: --phased-bam)
  posteriors, GT     -> ltr_posteriors
                        or, with --prune-alleles, ltr_plan_create / _execute + ltr_plan_genotype: every locus in one resident
                        plan, posteriors -> uncalled alleles removed -> posteriors over the surviving haplotypes
                        (SeqStutterGenotyper::genotype, seq_stutter_genotyper.cpp:632-645)
  VCF                -> ltr_vcf_header, ltr_vcf_record, ltr_vcf_writer_*

    python examples/real_reads_trio.py [out.vcf.gz] [--ref-vcf panel.vcf.gz] [--prune-alleles]

run(...) returns the per-locus results (used by tests/test_gpu_real_reads.py, which also bit-compares the
LL matrices with the CPU oracle and checks the trio for Mendelian consistency)."""
import math, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from longtr_amd import _abi, _lib  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "bam")
SAMPLES = ["HG002", "HG003", "HG004"]
PAD = 400                     # reference window either side of a region (left_align_reads cuts reads to region -+ 200)


def convert_bed(src, dst):
    """CHROM START STOP PERIOD COPIES NAME MOTIF (the bundled file) -> CHROM START STOP MOTIF NAME (readRegions)."""
    with open(dst, "w") as out:
        for line in open(src):
            c = line.split()
            if len(c) >= 7:
                out.write("\t".join([c[0], c[1], c[2], c[6].replace("/", ","), c[5]]) + "\n")      # (alternative motifs: "/" -> the reader's ",")


def rebuild_reference(reads, lo, hi):
    """Reference bases of [lo, hi): known wherever some read matches ('=' runs).  A position every read
    mismatches ('X': the trio is homozygous for a substitution against hg38) takes the reads' majority base --
    NOT the hg38 base, which nothing here can know; it only ever sits in a flank.  'N' where the reads say nothing
    (a base all of them delete)."""
    ref = bytearray(b"N" * (hi - lo))
    votes = {}
    for r in reads:
        rp, qp = r["pos"], 0
        for t, n in r["cigar"]:
            if t in "=X":
                a, b = max(rp, lo), min(rp + n, hi)
                if a < b and t == "=":
                    ref[a - lo:b - lo] = r["seq"][qp + (a - rp):qp + (b - rp)].encode()
                elif a < b:
                    for k in range(a, b):
                        votes.setdefault(k, []).append(r["seq"][qp + (k - rp)])
            if t in "M=X":
                rp += n; qp += n
            elif t in "DN":
                rp += n
            elif t in "IS":
                qp += n
    for k, v in votes.items():
        if ref[k - lo] == ord("N"):
            ref[k - lo] = ord(max(sorted(set(v)), key=v.count))
    return bytes(ref)


def phasing_priors(sample, hp):
    """--phased-bam: SNPBamProcessor::process_phased_reads (snp_bam_processor.cpp:141-226) = ltr_phasing_priors: a read with an
    HP tag gets FROM_HAP_LL / OTHER_HAP_LL unless too few reads are phased (running totals over the samples, sticky verdict)."""
    p1, p2, _ = _lib.phasing_priors(sample, [h if h in (1, 2) else -1 for h in hp], len(SAMPLES))
    return p1, p2


def plan_genotype(ctx, todo, device_fields=False):
    """Every locus in ONE resident plan (pools trimmed like HapAligner::process_reads) and one ltr_plan_genotype call: per locus
    the dict of Plan.genotype (final blocks, posteriors, best pairs, per-read scores in the final columns).
    device_fields: ltr_plan_genotype_fields instead -- the GenotypeResult itself (the caller closes it); neither the posterior
    blocks nor the per-read scores leave the device."""
    flat, lro, pool_index, p1s, p2s, labs = [], [0], [], [], [], []
    for l in todo:
        alns, rb = l["alns"], l["blocks"][1]
        n, idx = _lib.pool_reads([a["seq"] for a in alns])
        first = {}
        for i, q in enumerate(idx):
            first.setdefault(int(q), i)
        pools = []
        for q in range(n):                                          # the pool's first read stands for it (ReadPooler)
            a = alns[first[q]]
            rc, lt, rt = _lib.trim_alignment(a, rb["start"], rb["end"], ctx.params.indel_flank_len)
            assert rc == 0
            t = a["seq"][lt:len(a["seq"]) - rt]
            pools.append(t if t else l["blocks"][0]["alleles"][0][-5:] + l["blocks"][2]["alleles"][0][:5])     # HapAligner.cpp:820-823
        flat.append((pools, _lib.haplotype_seqs(l["blocks"])))
        p1, p2 = phasing_priors(l["sample"], l["hp"])
        pool_index += list(idx); p1s += list(p1); p2s += list(p2); labs += list(l["sample"])
        lro.append(lro[-1] + len(alns))
    plan = ctx.plan(_abi.PackedBatch(flat))
    plan.execute()
    if device_fields:
        out = plan.genotype_fields([l["blocks"] for l in todo], lro, pool_index, p1s, p2s, labs, [len(SAMPLES)] * len(todo), prune=True)
        plan.close()
        return out
    out = plan.genotype([l["blocks"] for l in todo], lro, pool_index, p1s, p2s, labs, [len(SAMPLES)] * len(todo), prune=True)
    plan.close()
    return out


def ll_genotype(ctx, todo):
    """No plan: the per-read matrices and seed positions ltr_calc_hap_aln_probs returns go straight into ltr_ll_genotype (pruning
    and the fields of every record on the device) -- the GenotypeResult itself (the caller closes it)."""
    res = ctx.calc_hap_aln_probs([(l["blocks"], l["alns"], None) for l in todo])
    lro, p1s, p2s, labs = [0], [], [], []
    for l in todo:
        p1, p2 = phasing_priors(l["sample"], l["hp"])
        p1s += list(p1); p2s += list(p2); labs += list(l["sample"])
        lro.append(lro[-1] + len(l["alns"]))
    return ctx.genotype_ll([m for m, _ in res], [s for _, s in res], [l["blocks"] for l in todo], lro, p1s, p2s, labs,
                           [len(SAMPLES)] * len(todo), prune=True, fields={})


def run(ctx, vcf_path=None, max_loci=None, tmp_dir="/tmp", ref_vcf=None, prune=False, device_fields=False, from_ll=False, consensus=False):
    """consensus (not with ref_vcf): candidate alleles by ltr_build_haplotypes_consensus -- reads of a sample without an exact allele are clustered
    and the clusters' partial-order-alignment consensus joins the candidates.  It runs only where more than a quarter of a sample's reads
    carry no exact allele.  On the bundled HiFi trio that is not nowhere: 13 consensus alleles join the candidates and 5 of the 39 genotyped loci
    print differently (homopolymers and one 5 kb repeat, where a sample's reads disagree with every exact allele), the other 34 are unchanged
    (main prints how many consensus alleles came out).
    ref_vcf: a bgzipped, tabix-indexed VCF whose records give the candidate alleles (--ref-vcf: read_vcf_alleles,
    add_vcf_haplotype_block); a locus without a record gets the status "no panel record".
    prune: discovery mode as the reference runs it (seq_stutter_genotyper.cpp:636-645) -- alleles no sample carries in its best
    haplotype pair are removed once and the posteriors recomputed over the surviving haplotypes (ltr_plan_genotype), so the
    record lists only called ALT alleles and Q is normalised over the diplotypes LongTR keeps.  With ref_vcf nothing is
    pruned, as in the reference (:636).  Default off: every candidate allele stays in the record.
    device_fields (with prune): the numbers of every record (GT, Q, PQ, GLDIFF, DP, DSNP, PSNP, MALLREADS) are computed on the
    device by ltr_plan_genotype_fields and all records formatted by one ltr_genotype_result_vcf_records call.
    from_ll (with prune and device_fields): no resident plan -- ltr_calc_hap_aln_probs scores the reads as in the default run and its
    matrices and seed positions are handed to ltr_ll_genotype, which does the rest of device_fields on them."""
    bed = os.path.join(tmp_dir, f"ltr_regions_{os.getpid()}.bed")
    convert_bed(os.path.join(DATA, "test_regions_hg38.bed"), bed)
    regions, _ = _lib.read_regions(bed, order=True)
    os.remove(bed)
    if max_loci:
        regions = regions[:max_loci]
    bam = _lib.Bam([os.path.join(DATA, f"{s}_sample_reads.bam") for s in SAMPLES])
    sample_of_file = {rg["file"]: SAMPLES.index(rg["sample"]) for rg in bam.read_groups()}
    chrom_len = dict(bam.refs())
    panel = _lib.VcfPanel(ref_vcf) if ref_vcf else None
    loci = []
    for reg in regions:
        if reg["period"] < 1:
            continue
        recs = bam.fetch(reg["chrom"], reg["start"], reg["stop"], tags=("HP",))
        recs = [r for r in recs if r["mapq"] >= 20 and not (r["flag"] & 0x704)]            # mapped, primary, not QC-fail / duplicate
        lo, hi = max(reg["start"] - PAD, 0), min(reg["stop"] + PAD, chrom_len[reg["chrom"]])
        ref = rebuild_reference(recs, lo, hi)
        raw = [dict(pos=r["pos"], end_pos=r["end_pos"], bases=r["seq"].encode(), cigar=r["cigar"], sample=sample_of_file[r["file"]],
                    hp=int(r.get("HP", 0)), quals=r["qual"].encode("latin-1"), reverse=int(bool(r["flag"] & 16))) for r in recs]
        loc = dict(region=reg, n_raw=len(raw), ref_unknown=ref.count(b"N"), status="ok")
        loci.append(loc)
        if b"N" in ref[PAD - 250:len(ref) - PAD + 250]:
            loc["status"] = "reference not covered by matching reads"; continue
        rs = _lib.ReadSet(raw, len(SAMPLES), reg["start"], reg["stop"], ref, lo)
        if panel is None and consensus:
            hb = ctx.build_haplotypes_consensus([dict(rs=rs, region_start=reg["start"], region_stop=reg["stop"], period=reg["period"],
                                                      chrom_seq_start=lo, chrom_len=chrom_len[reg["chrom"]])])[0]
            loc["consensus_alleles"] = sum(hb["inexact"] or [])
        elif panel is None:
            hb = rs.build_haplotype(reg["start"], reg["stop"], reg["period"], lo, chrom_len[reg["chrom"]])
        else:
            rec = panel.alleles(reg["chrom"], reg["start"], reg["stop"])
            hb = dict(blocks=None, failure="no panel record") if rec is None else \
                rs.build_vcf_haplotype(rec[0], rec[1], reg["period"], lo, chrom_len[reg["chrom"]])
        reads = [r for r in rs.reads if not r["deleted"]]
        n_p1s, n_p2s = rs.n_p1s, rs.n_p2s
        rs.close()
        if hb["blocks"] is None or len(reads) < 5:
            loc["status"] = hb["failure"] or "too few reads"; continue
        loc.update(blocks=hb["blocks"], alns=[dict(start=r["start"], stop=r["stop"], seq=r["seq"], cigar=r["cigar"]) for r in reads],
                   sample=[r["sample"] for r in reads], hp=[raw[r["source"]]["hp"] for r in reads], ref=ref, ref_start=lo, n_p1s=n_p1s, n_p2s=n_p2s)
    bam.close()
    if panel is not None:
        panel.close()
    todo = [l for l in loci if l["status"] == "ok"]
    # one GPU pass for every locus: ltr_calc_hap_aln_probs, or -- pruning -- a resident plan and ltr_plan_genotype on it
    if device_fields and (not prune or panel is not None):
        raise ValueError("device_fields needs prune=True and no ref_vcf: it is the plan path (ltr_plan_genotype_fields)")
    if from_ll and not device_fields:
        raise ValueError("from_ll is a form of device_fields: ltr_ll_genotype on the output of ltr_calc_hap_aln_probs")
    if device_fields and todo:
        return _run_device_fields(ctx, loci, todo, vcf_path, from_ll)
    final = plan_genotype(ctx, todo) if prune and panel is None and todo else None
    res = ctx.calc_hap_aln_probs([(l["blocks"], l["alns"], None) for l in todo]) if final is None else [(g["read_ll"], None) for g in final]
    writer = _lib.VcfWriter(vcf_path) if vcf_path else None
    if writer:
        # Genotyper::get_vcf_header: field definitions a downstream tool can type the records with (no FASTA here: the
        # reference windows are rebuilt from the reads, so there are no ##contig lines)
        writer.header(_lib.vcf_header("(no hg38 FASTA bundled: windows rebuilt from the reads' = runs)", "examples/real_reads_trio.py", None, SAMPLES))
    for k, (l, (ll, seeds)) in enumerate(zip(todo, res)):
        R, H = ll.shape
        log_p1, log_p2 = phasing_priors(l["sample"], l["hp"])
        lab = np.asarray(l["sample"], dtype=np.int32)
        if final is None:
            post = ctx.posteriors(ll, log_p1, log_p2, lab, len(SAMPLES))
        else:                                                       # the pruned state: blocks, posteriors and scores of the surviving haplotypes
            g = final[k]
            post = dict(post=g["post"], sample_total_ll=g["sample_total_ll"], gts=g["gts"], clamped_ll=g["read_ll"])
            l.update(candidate_blocks=l["blocks"], blocks=g["blocks"], removed=g["removed"])
        alleles = l["blocks"][1]["alleles"]
        l.update(ll=ll, seeds=seeds, gts=post["gts"], allele_lens=[len(a) for a in alleles], log_p1=log_p1,
                 gt_lens=[tuple(sorted(len(alleles[int(g)]) for g in gt)) for gt in post["gts"]])
        if writer:                                                  # SeqStutterGenotyper::write_vcf_record: GT:GB:Q:PQ:DP:...
            reg = l["region"]
            pv = _abi.PackedVcfLocus(dict(chrom=reg["chrom"], region_start=reg["start"], region_stop=reg["stop"], name=reg["name"], motif=reg["motif"],
                                          period_str=reg["period_str"], chrom_seq=l["ref"], chrom_seq_start=l["ref_start"], blocks=l["blocks"], block=1,
                                          inexact_allele=np.zeros(len(alleles), dtype=np.uint8), log_aln_probs=post["clamped_ll"], log_p1=log_p1, log_p2=log_p2,
                                          sample_label=lab, alns=l["alns"], log_sample_posteriors=post["post"], sample_total_ll=post["sample_total_ll"],
                                          best_haplotypes=post["gts"], n_p1s=l["n_p1s"], n_p2s=l["n_p2s"], sample_names=SAMPLES))
            line, pos = _lib.vcf_record(pv)
            l["vcf_line"], l["vcf_locus"] = line, pv
            writer.add_record(reg["chrom"], pos, line)
    if writer:
        writer.close()
    return loci


def _run_device_fields(ctx, loci, todo, vcf_path, from_ll=False):
    """The pruned run with the fields of every record from the device and one formatting call for all records."""
    none = np.zeros(0)
    with (ll_genotype(ctx, todo) if from_ll else plan_genotype(ctx, todo, device_fields=True)) as result:
        pvs = []
        for k, l in enumerate(todo):
            g = result.locus(k)
            l.update(candidate_blocks=l["blocks"], blocks=g["blocks"], removed=g["removed"])
            alleles = l["blocks"][1]["alleles"]
            log_p1, log_p2 = phasing_priors(l["sample"], l["hp"])
            l.update(ll=None, seeds=None, gts=g["gts"], allele_lens=[len(a) for a in alleles], log_p1=log_p1,
                     gt_lens=[tuple(sorted(len(alleles[int(x)]) for x in gt)) for gt in g["gts"]])
            reg = l["region"]
            pvs.append(_abi.PackedVcfLocus(dict(
                chrom=reg["chrom"], region_start=reg["start"], region_stop=reg["stop"], name=reg["name"], motif=reg["motif"],
                period_str=reg["period_str"], chrom_seq=l["ref"], chrom_seq_start=l["ref_start"], blocks=l["blocks"], block=1,
                inexact_allele=np.zeros(len(alleles), dtype=np.uint8), log_aln_probs=none, log_p1=log_p1, log_p2=log_p2,
                sample_label=np.asarray(l["sample"], dtype=np.int32), alns=l["alns"], log_sample_posteriors=none, sample_total_ll=none,
                best_haplotypes=np.zeros(0, dtype=np.int32), n_p1s=l["n_p1s"], n_p2s=l["n_p2s"], sample_names=SAMPLES)))
        lines, pos = result.vcf_records(pvs)
    writer = _lib.VcfWriter(vcf_path) if vcf_path else None
    if writer:
        writer.header(_lib.vcf_header("(no hg38 FASTA bundled: windows rebuilt from the reads' = runs)", "examples/real_reads_trio.py", None, SAMPLES))
    for l, pv, line, p in zip(todo, pvs, lines, pos):
        l["vcf_line"], l["vcf_locus"] = line, pv
        if writer:
            writer.add_record(l["region"]["chrom"], int(p), line)
    if writer:
        writer.close()
    return loci


def main():
    import argparse
    ap = argparse.ArgumentParser(description="The chain on the bundled trio reads.")
    ap.add_argument("out", nargs="?", default=None, help="VCF to write (BGZF for *.gz)")
    ap.add_argument("--ref-vcf", default=None, metavar="PATH", help="bgzipped, tabix-indexed VCF of candidate alleles (LongTR's --ref-vcf)")
    ap.add_argument("--prune-alleles", action="store_true", help="remove the alleles no sample is called with and genotype again (the reference's discovery mode)")
    ap.add_argument("--device-fields", action="store_true", help="needs --prune-alleles, not with --ref-vcf: the records' numbers from the device, all records formatted in one call")
    ap.add_argument("--from-ll", action="store_true", help="with --device-fields: no resident plan, the matrices of ltr_calc_hap_aln_probs go into ltr_ll_genotype")
    ap.add_argument("--consensus", action="store_true", help="not with --ref-vcf: candidate alleles by ltr_build_haplotypes_consensus (reads without an exact allele clustered, POA consensus per cluster)")
    args = ap.parse_args()
    ctx = _lib.Context(0)
    loci = run(ctx, args.out, ref_vcf=args.ref_vcf, prune=args.prune_alleles, device_fields=args.device_fields, from_ll=args.from_ll, consensus=args.consensus)
    if args.consensus:
        print(f"consensus alleles added over all loci: {sum(l.get('consensus_alleles', 0) for l in loci)}")
    for l in loci:
        if l["status"] != "ok":
            print(f"{l['region']['name']:>16} {l['region']['chrom']}:{l['region']['start']}-{l['region']['stop']}  skipped: {l['status']}")
            continue
        child, pa, ma = l["gt_lens"]
        ok = any((child[0] in p1 and child[1] in p2) for p1, p2 in ((pa, ma), (ma, pa)))
        print(f"{l['region']['name']:>16} {l['region']['chrom']}:{l['region']['start']}-{l['region']['stop']} motif {l['region']['motif']:<8} "
              f"reads {len(l['alns']):3d} alleles(bp) {l['allele_lens']}  HG002 {child} HG003 {pa} HG004 {ma}  {'mendelian' if ok else 'MENDELIAN VIOLATION'}")


if __name__ == "__main__":
    main()
