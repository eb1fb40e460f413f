"""-m gpu: a ploidy per (locus, sample) -- ltr_ll_genotype_sample_ploidy, ltr_plan_genotype_sample_ploidy,
ltr_plan_posteriors_sample_ploidy, ltr_genotype_result_sample_haploid, the records of a mixed locus and --sample-ploidy of the
driver (include/ltr_gpu_ploidy.h).

Unit (l, s) depends on the other samples of its locus only through pruning, so the oracle is the library's own per-locus-ploidy
calls, stitched: sample s of a mixed call against sample s of the uniform call of its ploidy.  All comparisons are == on bits,
integers and text; there is no tolerance in this file.  Loci: 24 (70 under the grid cap) with 1 to 3 samples of 0, 1 or 7 reads,
one block of 1 to 4 alleles or two blocks (H = 6), all 2^S ploidy patterns, phasing priors, scores below the -600 clamp."""
import os

import numpy as np
import pytest

import sample_ploidy_util as sp
import vcf_fields_util as vu
from longtr_amd import _abi, _lib, call, synth
from test_gpu_call import BAMS, SAMPLES, ReadsReference, data_lines, rt, strip_timing

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam")
_CACHE = {}


def _case(ctx, n_loci=24, samples=None):
    key = ("case", n_loci, samples)
    if key not in _CACHE:
        case = sp.case_of(sp.make_loci(n_loci, 411 + n_loci, samples))
        case["uniform"] = {p: sp.run(ctx, case, 0, haploid=bool(p)) for p in (0, 1)}      # the two references, computed once
        _CACHE[key] = case
    return _CACHE[key]


def test_the_case_has_the_shapes_and_tells_the_ploidies_apart(gpu_ctx):
    case = _case(gpu_ctx)
    loci = case["loci"]
    assert len(loci) == 24 and {L["S"] for L in loci} == {1, 2, 3}
    assert {len(L["blocks"][1]["alleles"]) for L in loci if len(L["blocks"][0]["alleles"]) == 1} == {1, 2, 3, 4}
    assert {len(L["haps"]) for L in loci if len(L["blocks"][0]["alleles"]) == 2} == {6}
    assert {int((L["lab"] == s).sum()) for L in loci for s in range(L["S"])} == {0, 1, 7}
    assert any((L["p1"] != L["p2"]).any() for L in loci) and any((L["M"] < -600.0).any() for L in loci)
    for l, L in enumerate(loci):
        assert {tuple(sp.pattern(loci, k)[l]) for k in range(8)} == {tuple((m >> s) & 1 for s in range(L["S"])) for m in range(2 ** L["S"])}
    dip, hap = case["uniform"][0], case["uniform"][1]
    differ = [l for l, L in enumerate(loci) if len(L["haps"]) > 1 and len(L["lab"])
              and not sp.same(dip["loci"][l]["sample_total_ll"], hap["loci"][l]["sample_total_ll"])]
    assert len(differ) >= 12                                     # the priors differ: a call that ignored the flags could not match both
    assert any((dip["fields"][l]["best_gts"][:, 0] != dip["fields"][l]["best_gts"][:, 1]).any() for l in range(24))   # heterozygous calls exist
    assert any((dip["fields"][l]["n_snp"] > 0).any() for l in range(24))


@pytest.mark.parametrize("k", range(8))
def test_every_unit_equals_the_uniform_call_of_its_ploidy(gpu_ctx, k):
    """1. prune = 0, GL / PL / PHASEDGL and posteriors: posteriors, totals, best pairs, Q, PQ, GLDIFF, the reads' alleles and the
    counters of every (l, s); a haploid sample's gls / pls row = the haploid run's V values, then 0.0; the accessors echo the flags."""
    case = _case(gpu_ctx)
    flags = sp.pattern(case["loci"], k)
    got = sp.run(gpu_ctx, case, 0, sample_haploid=flags)
    sp.check_stitched(got, case["uniform"], flags, case["loci"], what=k)
    assert any(0 < f.sum() < f.size for f in flags)              # some locus is mixed in every run


@pytest.mark.parametrize("k", range(8))
def test_pruning_takes_the_union_of_the_samples_calls(gpu_ctx, k):
    """2. prune = 1 against the chain of existing calls (sample_ploidy_util.expected_after_pruning): removed sets, block lists,
    second-pass numbers and fields."""
    case = _case(gpu_ctx)
    flags = sp.pattern(case["loci"], k)
    refs, removed = sp.expected_after_pruning(gpu_ctx, case, flags, case["uniform"])
    got = sp.run(gpu_ctx, case, 1, sample_haploid=flags)
    sp.check_stitched(got, refs, flags, case["loci"], what=("prune", k))
    lost = [l for l, r in enumerate(removed) if any(r)]
    assert lost and len(lost) < len(removed)                     # some loci lose alleles, not all
    assert any(0 < flags[l].sum() < flags[l].size for l in lost) # ... a mixed one among them
    for l in lost:
        assert got["loci"][l]["num_aff_alleles"] == sum(len(r) for r in removed[l])
        assert got["loci"][l]["num_aff_blocks"] == sum(1 for r in removed[l] if r)


def test_uniform_flags_and_null_are_the_existing_calls(gpu_ctx):
    """3. all 0 / all 1 through the new entry point = locus_haploid 0 / 1, a NULL array = the call without it: results and text."""
    import ctypes as C
    case = _case(gpu_ctx)
    loci = case["loci"]
    for prune in (0, 1):
        for p in (0, 1):
            want = sp.run(gpu_ctx, case, prune, locus_haploid=np.full(len(loci), p, dtype=np.uint8))
            got = sp.run(gpu_ctx, case, prune, sample_haploid=[np.full(L["S"], p, dtype=np.uint8) for L in loci], haploid=not p)
            old = sp.run(gpu_ctx, case, prune, haploid=bool(p))
            assert got["lines"] == want["lines"] == old["lines"] and np.array_equal(got["pos"], want["pos"])
            assert got["haploid"] == want["haploid"] == [p] * len(loci)
            for l in range(len(loci)):
                assert set(got["fields"][l]) == set(want["fields"][l]) and set(got["loci"][l]) == set(want["loci"][l])
                for image in ("fields", "loci"):
                    for key, a in got[image][l].items():
                        b = want[image][l][key]
                        if key in ("removed", "blocks"):
                            assert [x["alleles"] for x in a] == [x["alleles"] for x in b] if key == "blocks" else a == b, (l, key)
                        else:
                            assert (a is None and b is None) or sp.same(a, b), (prune, p, l, key)
            # NULL through the new symbol
            packed = gpu_ctx.pack_ll_genotype(case["mats"], None, case["blocks"], haploid=bool(p), prune=bool(prune), want_read_ll=True, **case["largs"])
            fr = _abi.FieldsRequest()
            fr.want_gls = fr.want_pls = fr.want_phased_gls = fr.want_posteriors = 1
            h = C.c_void_p()
            assert _lib.lib().ltr_ll_genotype_sample_ploidy(gpu_ctx._h, C.byref(packed["lb"]), C.byref(packed["gb"]), C.byref(fr), None, C.byref(h)) == 0
            with _lib.GenotypeResult(gpu_ctx, h, packed) as res:
                rng = np.random.default_rng(7)                   # the record text of the NULL call: the bytes of the call without the array
                pv = [_abi.PackedVcfLocus(sp._describe(l, L, res.locus(l), False, rng)) for l, L in enumerate(loci)]
                lines, pos = res.vcf_records(pv, _abi.vcf_options(**sp.OPT))
                assert lines == old["lines"] and np.array_equal(pos, old["pos"])
                for l in range(len(loci)):
                    f, g = res.fields(l), res.locus(l)
                    assert all((f[key] is None and v is None) or sp.same(f[key], v) for key, v in old["fields"][l].items()), l
                    assert sp.same(g["post"], old["loci"][l]["post"]) and sp.same(g["gts"], old["loci"][l]["gts"]) and res.haploid(l) == p
                with pytest.raises(_lib.LtrError):
                    res.sample_haploid(len(loci))


@pytest.mark.parametrize("prune", [0, 1])
def test_more_units_than_wavefronts(gpu_ctx, prune):
    """4. 70 loci x 3 samples under ltr_ctx_set_debug("grid_cap", 2): the same bits as uncapped, and as the stitched references.
    (The genotype and fields kernels take one workgroup per unit whatever the cap says; this holds them to that.)"""
    case = _case(gpu_ctx, 70, 3)
    flags = sp.pattern(case["loci"], 3)
    refs = sp.expected_after_pruning(gpu_ctx, case, flags, case["uniform"])[0] if prune else case["uniform"]
    free = sp.run(gpu_ctx, case, prune, sample_haploid=flags)
    try:
        gpu_ctx.set_debug("grid_cap", 2)
        capped = sp.run(gpu_ctx, case, prune, sample_haploid=flags)
    finally:
        gpu_ctx.set_debug("reset", 0)
    sp.check_stitched(capped, refs, flags, case["loci"], what="capped")
    assert capped["lines"] == free["lines"]
    for l in range(70):
        for key, a in capped["fields"][l].items():
            assert (a is None and free["fields"][l][key] is None) or sp.same(a, free["fields"][l][key]), (l, key)
        assert sp.same(capped["loci"][l]["post"], free["loci"][l]["post"]) and sp.same(capped["loci"][l]["gts"], free["loci"][l]["gts"])


def test_plan_path_equals_the_matrices_path(gpu_ctx):
    """5. a 6-locus synthetic plan, executed once: Plan.genotype_fields / genotype / posteriors with sample_haploid against
    Context.genotype_ll on the plan's fetched per-read matrices with the same flags."""
    import genotype_util as gt
    from test_gpu_ll_genotype import WANT
    loci = gt.make_case(77, n_loci=6, reads=(6, 20))
    for L in loci:
        if L["S"] > 3:
            L["S"], L["lab"], L["filt"] = 3, (L["lab"] % 3).astype(np.int32), L["filt"][:3].copy()
    batch, args = gt.pack(loci)
    plan = gpu_ctx.plan(batch)
    try:
        plan.execute()
        ll, seeds = plan.fetch()
        mats = [gt.per_read(batch, ll, l, L) for l, L in enumerate(loci)]
        flags = [np.asarray([(l + s) % 2 for s in range(L["S"])], dtype=np.uint8) for l, L in enumerate(loci)]
        assert any(0 < f.sum() < f.size for f in flags)
        blocks, filt = [L["blocks"] for L in loci], np.concatenate([L["filt"] for L in loci])
        largs = {k: v for k, v in args.items() if k != "pool_index"}
        for prune in (False, True):
            with plan.genotype_fields(blocks, want_read_ll=True, sample_filtered=filt, prune=prune, sample_haploid=flags, **WANT, **args) as a, \
                    gpu_ctx.genotype_ll(mats, None, blocks, prune=prune, want_read_ll=True, fields=WANT, sample_filtered=filt,
                                        sample_haploid=flags, **largs) as b:
                for l in range(len(loci)):
                    fa, fb, ga, gb = a.fields(l), b.fields(l), a.locus(l), b.locus(l)
                    assert np.array_equal(fa["sample_haploid"], flags[l]) and a.haploid(l) == b.haploid(l) == int(flags[l].all())
                    assert all((fa[k] is None and fb[k] is None) or sp.same(fa[k], fb[k]) for k in fa), l
                    assert all(sp.same(ga[k], gb[k]) for k in ("post", "sample_total_ll", "gts", "read_ll", "new_to_old", "sample_haploid")), l
                    assert ga["removed"] == gb["removed"]
            plain = plan.genotype(blocks, sample_filtered=filt, prune=prune, sample_haploid=flags, **args)
            with gpu_ctx.genotype_ll(mats, None, blocks, prune=prune, want_read_ll=True, sample_filtered=filt, sample_haploid=flags, **largs) as b:
                for l in range(len(loci)):
                    assert all(sp.same(plain[l][k], b.locus(l)[k]) for k in ("post", "sample_total_ll", "gts", "read_ll")) and plain[l]["haploid"] == int(flags[l].all())
        post, off, stl, gts = plan.posteriors(sample_haploid=flags, **args)
        first = plan.genotype(blocks, sample_filtered=filt, prune=False, sample_haploid=flags, **args)
        assert sp.same(stl, np.concatenate([g["sample_total_ll"] for g in first])) and sp.same(gts, np.concatenate([g["gts"] for g in first]))
        assert sp.same(post, np.concatenate([g["post"].ravel() for g in first]))
        with pytest.raises(_lib.LtrError):
            plan.posteriors(sample_haploid=flags, locus_haploid=np.zeros(len(loci), dtype=np.uint8), **args)
    finally:
        plan.close()


def _columns(line):
    c = line.split("\t")
    info = dict(kv.split("=", 1) for kv in c[7].split(";") if "=" in kv)
    return c[8].split(":"), [x.split(":") for x in c[9:]], info


def test_records_of_mixed_loci(gpu_ctx):
    """6. a mixed locus writes the ten-field FORMAT; a diploid sample's column is that of the all-diploid record, a haploid
    sample's tokens are those of the all-haploid record with "." where one copy has no value; AN / AC count one allele for it."""
    case = _case(gpu_ctx)
    dip, hap = case["uniform"][0], case["uniform"][1]
    seen = 0
    for k in range(8):
        flags = sp.pattern(case["loci"], k)
        got = sp.run(gpu_ctx, case, 0, sample_haploid=flags)
        for l, L in enumerate(case["loci"]):
            f = flags[l]
            if not 0 < f.sum() < f.size:
                assert got["lines"][l] == (hap if f.all() else dip)["lines"][l]      # the per-locus case: the same bytes
                continue
            fmt, cols, info = _columns(got["lines"][l])
            dfmt, dcols, _ = _columns(dip["lines"][l])
            hfmt, hcols, _ = _columns(hap["lines"][l])
            assert ":".join(fmt).startswith(sp.TEN) and fmt == dfmt and ":".join(hfmt).startswith(sp.SIX)
            an, counts = 0, np.zeros(got["fields"][l]["V"], dtype=int)
            for s in range(L["S"]):
                col = cols[s]
                if col == ["."] or col[-1] != "PASS":            # a sample without a read: the same in every form
                    assert ":".join(col).endswith("NO_READS") and (L["lab"] == s).sum() == 0
                    continue
                assert len(col) == len(fmt)
                if not f[s]:
                    assert col == dcols[s], (l, s)
                    an += 2
                    for a in got["fields"][l]["best_gts"][s]:
                        counts[a] += 1
                    continue
                seen += 1
                mine, ref = dict(zip(fmt, col)), dict(zip(hfmt, hcols[s]))
                for key in ("GT", "GB", "Q", "DP", "DFLANKINDEL", "GLDIFF", "GL", "PL", "HQ", "PHQ", "FILTER"):
                    assert mine[key] == ref[key], (l, s, key)
                assert "|" not in mine["GT"] and "|" not in mine["GB"] and len(mine["GL"].split(",")) == len(mine["PL"].split(",")) == got["fields"][l]["V"]
                assert [mine[key] for key in ("PQ", "DSNP", "PDP", "PSNP", "PHASEDGL")] == ["."] * 5
                an += 1
                counts[got["fields"][l]["best_gts"][s, 0]] += 1
            assert int(info["AN"]) == an and int(info["REFAC"]) == counts[0]
            if len(counts) > 1:                                  # AC in the record's allele order: a permutation of ours; its sum and multiset hold
                ac = [int(x) for x in info["AC"].split(",")]
                assert sorted(ac) == sorted(counts[1:].tolist()) and sum(ac) + counts[0] == an
    assert seen >= 20


def test_a_hand_written_record_of_a_man_and_a_woman():
    """6b. two samples on one locus, the first haploid: the text, written out.  (Host only, but the batched writer is reached
    through a result, so it runs with the GPU tests.)"""
    ctx = _lib.Context(0)
    try:
        flank_l, flank_r = b"GATTACAGATTACAGATTACAGATTACAGATT", b"CCATGGCCATGGCCATGGCCATGGCCATGGCC"
        alleles = [b"ACGACGACGACG", b"ACGACGACGACGACG", b"ACGACGACG"]
        blocks = [dict(start=1000, end=1032, is_repeat=False, period=1, alleles=[flank_l]),
                  dict(start=1032, end=1044, is_repeat=True, period=3, alleles=alleles),
                  dict(start=1044, end=1076, is_repeat=False, period=1, alleles=[flank_r])]
        # reads 0-2: the man (sample 0), all for allele 1; reads 3-6: the woman, two for allele 0 and two for allele 2
        M = np.full((7, 3), -40.0)
        for r, a in enumerate((1, 1, 1, 0, 0, 2, 2)):
            M[r, a] = -1.0
        lab = np.asarray([0, 0, 0, 1, 1, 1, 1], dtype=np.int32)
        lro = np.asarray([0, 7], dtype=np.int64)
        zeros = np.zeros(7)
        with ctx.genotype_ll([M], None, [blocks], lro, zeros, zeros, lab, [2], prune=False, want_read_ll=True,
                             fields=dict(want_gls=True, want_pls=True, want_phased_gls=True, want_posteriors=True),
                             sample_haploid=[[1, 0]]) as res:
            g = res.locus(0)
            chrom = (b"T" * 300 + flank_l + alleles[0] + flank_r + b"T" * 300)
            v = _abi.PackedVcfLocus(dict(chrom="chrX", region_start=1032, region_stop=1044, name="TR1", motif="ACG", period_str="3", chrom_seq=chrom,
                                         chrom_seq_start=700, blocks=g["blocks"], block=1, log_aln_probs=g["read_ll"], log_p1=zeros, log_p2=zeros,
                                         sample_label=lab, alns=None, log_sample_posteriors=g["post"], sample_total_ll=g["sample_total_ll"],
                                         best_haplotypes=g["gts"], n_p1s=np.zeros(2, dtype=np.int32), n_p2s=np.zeros(2, dtype=np.int32),
                                         sample_names=["MAN", "WOMAN"], haploid=True))      # (ignored: the result's ploidy decides)
            lines, pos = res.vcf_records([v], _abi.vcf_options(output_gls=1, output_pls=1, output_phased_gls=1, output_allreads=0, output_mallreads=0))
            assert res.haploid(0) == 0 and res.sample_haploid(0).tolist() == [1, 0]
        # The woman's column is that of the all-diploid record of this locus and the man's tokens those of the all-haploid one
        # (both from the per-locus host writer, ltr_vcf_record, on posteriors worked out by hand); AN = 1 + 2.
        assert lines[0] == (
            "chrX\t1033\tTR1\tACGACGACGACG\tACGACGACG,ACGACGACGACGACG\t.\t.\t"
            "START=1033;END=1044;MOTIF=ACG;PERIOD=3;NSKIP=0;NFILT=0;INEXACT_ALLELE=0,0;BPDIFFS=-3,3;DP=7;DSNP=0;DFLANKINDEL=0;AN=3;REFAC=1;AC=1,1\t"
            "GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF:GL:PL:PHASEDGL\t"
            "2:3:1.00:.:3:.:0:.:.:50.81:-52.12,-52.12,-1.30:508,508,0:.\t"
            "0|1:0|-3:1.00:0.50:4:0:0:0|0:0|0:32.67:-35.61,-2.94,-35.61,-36.21,-36.21,-69.49:326,0,326,332,332,665:"
            "-35.61,-2.94,-36.21,-2.94,-35.61,-36.21,-36.21,-36.21,-69.49")
        assert int(pos[0]) == 1033
    finally:
        ctx.close()


# ---- 7. the driver on the bundled trio ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    d = tmp_path_factory.mktemp("ploidy_call")
    bed = str(d / "regions.bed")
    rt.convert_bed(os.path.join(DATA, "test_regions_hg38.bed"), bed)
    regions, _ = _lib.read_regions(bed, order=True)
    return dict(dir=d, bed=bed, regions=regions, ref=ReadsReference(regions))


def _ploidy_file(trio, name, rows):
    path = str(trio["dir"] / name)
    with open(path, "w") as fh:
        fh.write("# sample\tchrom\tploidy\n" + "".join(f"{s}\t{c}\t{p}\n" for s, c, p in rows))
    return path


def _run(gpu_ctx, trio, name, **options):
    out = str(trio["dir"] / f"{name}.vcf")
    report = call.genotype_regions(gpu_ctx, BAMS, trio["ref"], trio["bed"], out, **options)
    assert report["error"] is None, report["error"]
    return report, out


def test_driver_with_a_ploidy_file(gpu_ctx, trio):
    men = _ploidy_file(trio, "men.tsv", [("HG002", "chr1", 1), ("HG003", "chr1", 1)])
    report, out = _run(gpu_ctx, trio, "men", sample_ploidy=men, chunk_loci=None)
    lines, _ = data_lines(out)
    assert report["columns"] == sorted(SAMPLES) == ["HG002", "HG003", "HG004"] and len(lines) >= 10
    for line in lines.values():
        fmt, cols, _ = _columns(line)
        assert ":".join(fmt) == sp.TEN + ":ALLREADS:MALLREADS"     # (the writer's defaults)
        for name, col in zip(report["columns"], cols):
            if col != ["."]:
                assert len(col) == len(fmt)
                assert ("|" in col[0]) == (name == "HG004") and ("|" in col[1]) == (name == "HG004"), line
    assert all(e["sample_ploidy"] == [1, 1, 2] for e in report["loci"]) and len(report["loci"]) == 40
    # the same through a dict; independent of the chunks and of the producer thread
    as_dict, out_d = _run(gpu_ctx, trio, "men_dict", sample_ploidy={("HG002", "chr1"): 1, ("HG003", "chr1"): 1}, chunk_loci=None)
    assert open(out_d, "rb").read() == open(out, "rb").read() and strip_timing(as_dict) == strip_timing(report)
    for name, kw in (("men_8", dict(chunk_loci=8)), ("men_serial", dict(chunk_loci=8, overlap=False))):
        rep, o = _run(gpu_ctx, trio, name, sample_ploidy=men, **kw)
        assert open(o, "rb").read() == open(out, "rb").read() and strip_timing(rep) == strip_timing(report), name
        assert rep["timing"]["chunks"] > 1


def test_driver_uniform_files_are_the_existing_options(gpu_ctx, trio):
    everyone = _ploidy_file(trio, "all.tsv", [(s, "chr1", 1) for s in SAMPLES])
    a, out_a = _run(gpu_ctx, trio, "all_haploid", sample_ploidy=everyone)
    b, out_b = _run(gpu_ctx, trio, "haploid_chrs", haploid_chrs=("chr1",))
    assert open(out_a, "rb").read() == open(out_b, "rb").read() and a["loci"] == b["loci"]
    assert all(e["sample_ploidy"] == [1, 1, 1] for e in a["loci"])
    # the file wins over --haploid-chrs for the pairs it names
    c, out_c = _run(gpu_ctx, trio, "back_to_two", haploid_chrs=("chr1",), sample_ploidy=_ploidy_file(trio, "two.tsv", [(s, "chr1", 2) for s in SAMPLES]))
    empty = _ploidy_file(trio, "empty.tsv", [])
    d, out_d = _run(gpu_ctx, trio, "empty", sample_ploidy=empty)
    e, out_e = _run(gpu_ctx, trio, "none")
    assert open(out_d, "rb").read() == open(out_e, "rb").read() == open(out_c, "rb").read() and d["loci"] == e["loci"] == c["loci"]
    assert all(x["sample_ploidy"] == [2, 2, 2] for x in e["loci"])
    bad = call.genotype_regions(gpu_ctx, BAMS, trio["ref"], trio["bed"], str(trio["dir"] / "bad.vcf"),
                                sample_ploidy=_ploidy_file(trio, "bad.tsv", [("HG005", "chr1", 1)]))
    assert bad["error"] and "HG005" in bad["error"] and bad["loci"] == []
