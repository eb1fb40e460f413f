"""The two halves of ltr_vcf_record (longtr_amd/csrc/ltr_vcf.cpp): ltr_vcf_fields, the arithmetic write_vcf_record does before
it prints (seq_stutter_genotyper.cpp:916-1043), and ltr_vcf_record_from_fields, the text.  CPU only: the random loci of
test_vcf_record.py's generator, against ltr_vcf_record itself, the C restatement (oracle/ltr_oracle_vcf.c, ltr_oracle.c) and
numpy restatements of calc_gl_diff / calc_PLs."""
import itertools

import numpy as np
import pytest

import oracle_lib as ol
import vcf_fields_util as vu
from longtr_amd import _abi, _lib
from test_vcf_record import _locus

SWITCHES = ["output_gls", "output_pls", "output_phased_gls", "output_allreads", "output_mallreads", "output_filters", "output_haplotype_data"]


def _cases(seed=71, n=60):
    """test_vcf_record.py's loci: diploid and haploid, a deleted allele, phased and not, sample filters, other output samples."""
    rng = np.random.default_rng(seed)
    for trial in range(n):
        haploid = trial % 5 == 4
        d, H = _locus(rng, int(rng.integers(8, 90)), int(rng.integers(1, 7)), int(rng.integers(1, 6)), int(rng.integers(6, 25)),
                      int(rng.integers(1, 4)), haploid=haploid, deleted_allele=(trial % 7 == 3), phased=(trial % 3 != 0))
        S = len(d["sample_names"])
        if trial % 4 == 1:
            d["sample_filter"] = ["" if s else "LOW_QUAL" for s in range(S)]
        if trial % 6 == 2:
            d["out_sample_names"] = ["S0", "ABSENT"] + ["S%d" % s for s in range(1, S)]
        yield trial, d, H, haploid


def test_record_from_fields_equals_record_byte_for_byte():
    n, seen = 0, set()
    for trial, d, H, haploid in _cases():
        pv = _abi.PackedVcfLocus(d)
        f = _lib.vcf_fields(pv)
        for bits in itertools.product((0, 1), repeat=len(SWITCHES)):
            opt = _abi.vcf_options(**dict(zip(SWITCHES, bits)))
            got, pos = _lib.vcf_record_from_fields(pv, f, opt)
            want, wpos = _lib.vcf_record(pv, opt)
            assert got == want and pos == wpos, (trial, bits, got, want)
            if sum(bits) in (0, 1, 6, 7):                        # the restatement on every switch alone, on and off
                assert (got, pos) == ol.oracle_vcf_record(pv, opt), (trial, bits)
            n += 1
        assert _lib.vcf_record_from_fields(pv, f) == _lib.vcf_record(pv)               # NULL options: the defaults
        seen.add((haploid, "sample_filter" in d, "out_sample_names" in d))
    assert n == 60 * 128 and {s[0] for s in seen} == {False, True} and any(s[1] for s in seen) and any(s[2] for s in seen)


def test_fields_equal_the_restatement_bit_for_bit():
    for trial, d, H, haploid in _cases(seed=73, n=40):
        pv = _abi.PackedVcfLocus(d)
        f = _lib.vcf_fields(pv)
        V, S, R = len(d["blocks"][1]["alleles"]), len(d["sample_names"]), len(d["log_p1"])
        assert (f["S"], f["R"], f["V"], f["block"]) == (S, R, V, 1)
        assert f["n_gl"] == (V if haploid else V * (V + 1) // 2) and f["n_pgl"] == (V if haploid else V * V)
        h2a = ol.oracle_haps_to_alleles(d["blocks"], 1)
        o = ol.oracle_extract_genotypes(d["log_sample_posteriors"], d["sample_total_ll"], d["best_haplotypes"], h2a, V, haploid)
        assert np.array_equal(f["best_gts"], o["best_gts"])
        for mine, theirs in (("log_phased", "log_phased_posteriors"), ("log_unphased", "log_unphased_posteriors"),
                             ("hap_log_phased", "hap_log_phased_posteriors"), ("hap_log_unphased", "hap_log_unphased_posteriors"),
                             ("gls", "gls"), ("gl_diffs", "gl_diffs"), ("phased_gls", "phased_gls")):
            assert np.array_equal(vu.bits(f[mine]), vu.bits(o[theirs])), (trial, mine)
        assert np.array_equal(f["pls"], o["pls"])
        vu.check_self_consistent(f, H, haploid)
        # per-read bookkeeping (:929-1043): the strand haplotype's allele, the reads with phasing information
        lab, p1, p2, ll, best = d["sample_label"], np.asarray(d["log_p1"]), np.asarray(d["log_p2"]), d["log_aln_probs"], d["best_haplotypes"]
        for s in range(S):
            mine = lab == s
            snp = np.abs(p1 - p2) > 1e-10
            assert f["n_aligned"][s] == mine.sum() and f["n_snp"][s] == (mine & snp).sum()
            assert f["n_s1"][s] == (mine & snp & (p1 > p2)).sum() and f["n_s2"][s] == (mine & snp & ~(p1 > p2)).sum()
        for r in range(R):
            ha, hb = best[lab[r]]
            hap = ha if (haploid or ha == hb or p1[r] + ll[r, ha] > p2[r] + ll[r, hb]) else hb
            assert f["read_allele"][r] == h2a[hap], (trial, r)
        # the want switches only drop pointers
        g = _lib.vcf_fields(pv, want=())
        assert g["gls"] is None and g["pls"] is None and g["phased_gls"] is None
        assert all(np.array_equal(g[k], f[k]) for k in vu.EXACT) and np.array_equal(vu.bits(g["gl_diffs"]), vu.bits(f["gl_diffs"]))


def test_bad_fields_are_refused_and_nothing_is_written():
    import ctypes as C
    rng = np.random.default_rng(5)
    d, H = _locus(rng, 30, 3, 3, 12, 2)
    pv = _abi.PackedVcfLocus(d)
    good = _lib.vcf_fields(pv)
    all_on = _abi.vcf_options(output_gls=1, output_pls=1, output_phased_gls=1)
    L = _lib.lib()

    def refused(fields, opt=None):
        buf = C.create_string_buffer(b"\x7f" * 4096, 4096)
        pos = C.c_int32(-7)
        if fields is None:
            ref = None
        else:
            st, keep = _abi.LocusFields.from_dict(fields)
            ref = C.byref(st)
        n = L.ltr_vcf_record_from_fields(C.byref(pv.struct), ref, None if opt is None else C.byref(opt), buf, len(buf), C.byref(pos))
        assert n == _abi.LTR_ERR_INVALID, n
        assert buf.raw == b"\x7f" * 4096 and pos.value == -7      # no write

    refused(None)
    for k in ("S", "R", "V"):
        refused(dict(good, **{k: good[k] + 1}))
        refused(dict(good, **{k: good[k] - 1}))
    bad = dict(good, best_gts=good["best_gts"].copy())
    bad["best_gts"][0, 1] = good["V"]
    refused(bad)
    bad = dict(good, read_allele=good["read_allele"].copy())
    bad["read_allele"][-1] = good["V"]
    refused(bad)
    bad["read_allele"][-1] = -1
    refused(bad)
    for k in ("best_gts", "log_phased", "log_unphased", "gl_diffs", "n_aligned", "n_snp", "n_s1", "n_s2", "read_allele"):
        refused(dict(good, **{k: None}))
    for k in ("gls", "pls", "phased_gls"):                        # a switch whose array was not computed
        refused(dict(good, **{k: None}), all_on)
        assert _lib.vcf_record_from_fields(pv, dict(good, **{k: None}))[0] == _lib.vcf_record(pv)[0]   # ... is fine when it is off
    with pytest.raises(_lib.LtrError):
        _lib.vcf_record_from_fields(pv, None)
    # the formatter does not read the matrices the fields were made from
    v = pv.struct
    for k in ("log_aln_probs", "log_p1", "log_p2", "log_sample_posteriors", "sample_total_ll", "best_haplotypes"):
        setattr(v, k, None)
    assert _lib.vcf_record_from_fields(pv, good, all_on)[0] == ol.oracle_vcf_record(_abi.PackedVcfLocus(d), all_on)[0]
    with pytest.raises(_lib.LtrError):                           # ... and ltr_vcf_fields does need them
        _lib.vcf_fields(pv)
