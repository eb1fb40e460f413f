"""CPU: the per-locus ploidy entry points (ltr_plan_posteriors_ploidy, ltr_plan_genotype_ploidy, ltr_ll_genotype_ploidy,
ltr_genotype_result_haploid) are exported, declared and bound; the ABI is still 6 and no struct the batched consumers take has
grown; and the host formatter prints the six-field FORMAT for a haploid locus and the ten-field one for a diploid locus, which
is what ltr_genotype_result_vcf_records relies on when it formats every locus with its own ploidy."""
import ctypes as C
import os

import numpy as np

from longtr_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ltr_plan_posteriors_ploidy", "ltr_plan_genotype_ploidy", "ltr_ll_genotype_ploidy", "ltr_genotype_result_haploid")


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ltr_gpu.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and name + "(" in hdr, name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.ltr_plan_posteriors_ploidy.argtypes) == 6 and len(L.ltr_plan_genotype_ploidy.argtypes) == 5
    assert len(L.ltr_ll_genotype_ploidy.argtypes) == 6 and L.ltr_genotype_result_haploid.restype is C.c_int32
    for text in ("genotyper_bam_processor.cpp:248", "When given, pb->haploid is not read"):
        assert text in hdr                                       # the reference citation and the rule travel with the declarations
    assert L.ltr_genotype_result_haploid(None, 0) < 0            # a bad result / index: negative, nothing dereferenced


def test_abi_version_and_struct_sizes_are_the_parents():
    assert _lib.lib().ltr_abi_version() == 6
    # sizeof as the binding of the commit before this feature gives them: nothing grew
    want = {"PosteriorBatch": 72, "GenotypeBatch": 32, "FieldsRequest": 24, "LocusFields": 136}
    assert {k: C.sizeof(getattr(_abi, k)) for k in want} == want


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    lb, gb, pb = _abi.LlBatch(), _abi.GenotypeBatch(), _abi.PosteriorBatch()
    gb.pb = C.pointer(pb)
    lh = np.ones(4, dtype=np.uint8)
    plh = lh.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(0x1000)                                    # never dereferenced: the NULL argument is found first
    for ctx, plb, pgb in ((None, lb, gb), (fake, None, gb), (fake, lb, None)):
        h = C.c_void_p(0x1234)
        rc = L.ltr_ll_genotype_ploidy(ctx, None if plb is None else C.byref(plb), None if pgb is None else C.byref(pgb), None, plh, C.byref(h))
        assert rc == _abi.LTR_ERR_INVALID and not h.value
    h = C.c_void_p(0x1234)
    assert L.ltr_plan_genotype_ploidy(None, C.byref(gb), None, plh, C.byref(h)) == _abi.LTR_ERR_INVALID and not h.value
    assert L.ltr_plan_posteriors_ploidy(None, C.byref(pb), plh, None, None, None) == _abi.LTR_ERR_INVALID


def _hand_built(haploid):
    """One locus by hand: a repeat block of three alleles between two flanks, one sample, two reads."""
    lflank, rflank = b"ACGTTGCAAGCTTAGC", b"GGATCCTTAGCAATCG"
    alleles = [b"CAG" * 5, b"CAG" * 4, b"CAG" * 7]
    s0 = 1000
    s1, e1 = s0 + len(lflank), s0 + len(lflank) + len(alleles[0])
    blocks = [dict(start=s0, end=s1, is_repeat=False, period=0, alleles=[lflank]),
              dict(start=s1, end=e1, is_repeat=True, period=3, alleles=alleles),
              dict(start=e1, end=e1 + len(rflank), is_repeat=False, period=0, alleles=[rflank])]
    V, S, R = 3, 1, 2
    chrom = (b"T" * 100 + lflank + alleles[0] + rflank + b"A" * 100)
    d = dict(chrom="chrX" if haploid else "chr1", region_start=s1, region_stop=e1, name="HAND", motif="CAG", period_str="3",
             chrom_seq=chrom, chrom_seq_start=s0 - 100, blocks=blocks, block=1,
             log_aln_probs=np.zeros((R, V)), log_p1=np.zeros(R), log_p2=np.zeros(R), sample_label=np.zeros(R, dtype=np.int32), alns=None,
             log_sample_posteriors=np.zeros((S, V, V)), sample_total_ll=np.zeros(S), best_haplotypes=np.zeros((S, 2), dtype=np.int32),
             sample_names=["S0"], haploid=haploid)
    n_gl, n_pgl = (V, V) if haploid else (V * (V + 1) // 2, V * V)
    gls = -np.arange(n_gl, dtype=np.float64)[None, :].copy()
    gls[0, 2 if haploid else 5] = 0.5                            # allele 2 (haploid) / genotype 2/2 (diploid) is the best
    f = dict(S=S, R=R, V=V, block=1, n_gl=n_gl, n_pgl=n_pgl, best_gts=np.array([[2, 2]], dtype=np.int32),
             log_phased=np.log([0.9]), log_unphased=np.log([0.95]), hap_log_phased=np.log([0.9]), hap_log_unphased=np.log([0.95]),
             gl_diffs=np.array([1.5]), gls=gls, pls=np.minimum(-10 * (gls - gls.max()), 999).astype(np.int32),
             phased_gls=-np.arange(n_pgl, dtype=np.float64)[None, :], n_aligned=np.array([2], dtype=np.int32), n_snp=np.array([0], dtype=np.int32),
             n_s1=np.array([0], dtype=np.int32), n_s2=np.array([0], dtype=np.int32), read_allele=np.array([2, 2], dtype=np.int32))
    return _abi.PackedVcfLocus(d), f


def test_formatter_prints_six_fields_haploid_and_ten_fields_diploid():
    hap_pv, hap_f = _hand_built(True)
    dip_pv, dip_f = _hand_built(False)
    plain = _abi.vcf_options(output_allreads=0, output_mallreads=0)
    assert _lib.vcf_record_from_fields(hap_pv, hap_f, plain)[0].split("\t")[8] == "GT:GB:Q:DP:DFLANKINDEL:GLDIFF"
    assert _lib.vcf_record_from_fields(dip_pv, dip_f, plain)[0].split("\t")[8] == "GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF"
    opt = _abi.vcf_options(output_gls=1, output_pls=1, output_phased_gls=1, output_allreads=0, output_mallreads=0)
    hap = _lib.vcf_record_from_fields(hap_pv, hap_f, opt)[0].split("\t")
    dip = _lib.vcf_record_from_fields(dip_pv, dip_f, opt)[0].split("\t")
    assert hap[8] == "GT:GB:Q:DP:DFLANKINDEL:GLDIFF:GL:PL", hap[8]         # (PHASEDGL is not applicable to a haploid call)
    assert dip[8] == "GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF:GL:PL:PHASEDGL", dip[8]
    hs, ds = dict(zip(hap[8].split(":"), hap[9].split(":"))), dict(zip(dip[8].split(":"), dip[9].split(":")))
    assert len(hap[9].split(":")) == 8 and len(dip[9].split(":")) == 13
    assert hs["GT"] == "2" and ds["GT"] in ("2|2", "2/2")
    assert len(hs["GL"].split(",")) == 3 and len(hs["PL"].split(",")) == 3          # V
    assert len(ds["GL"].split(",")) == 6 and len(ds["PL"].split(",")) == 6 and len(ds["PHASEDGL"].split(",")) == 9   # V(V+1)/2, V*V
    # the widths must fit the ploidy of the description: fields of the other ploidy are refused
    for pv, f in ((hap_pv, dip_f), (dip_pv, hap_f)):
        try:
            _lib.vcf_record_from_fields(pv, f, opt)
        except _lib.LtrError as e:
            assert e.code == _abi.LTR_ERR_INVALID
        else:
            raise AssertionError("fields of the other ploidy were accepted")
