"""include/ltr_gpu_ploidy.h against longtr_amd/_abi.PLOIDY_SIGNATURES, the binding's sample_haploid= checks and the --sample-ploidy
file of the driver.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from longtr_amd import _abi, _genotype, _lib, call
from test_abi_signatures import check_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ltr_plan_posteriors_sample_ploidy", "ltr_plan_genotype_sample_ploidy", "ltr_ll_genotype_sample_ploidy",
         "ltr_genotype_result_sample_haploid"]


def declarations():
    src = open(os.path.join(ROOT, "include", "ltr_gpu_ploidy.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^[ \t]*#[^\n]*", "", src, flags=re.M)        # preprocessor lines
    src = src.replace('extern "C" {', "")
    return [(" ".join(m.group(1).split()), m.group(2), [" ".join(p.split()) for p in m.group(3).split(",")])
            for m in re.finditer(r"([A-Za-z_][\w \t\n\*]*?)\b(ltr_\w+)\s*\(([^()]*)\)\s*;", src)]


def test_the_header_names_exactly_the_four_functions():
    decls = declarations()
    assert [d[1] for d in decls] == NAMES == list(_abi.PLOIDY_SIGNATURES)
    assert not set(NAMES) & set(_abi.SIGNATURES) and not set(NAMES) & set(_abi.HOOK_SIGNATURES) and not set(NAMES) & set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "ltr_gpu_ploidy.h")).read()
    assert '#include "ltr_gpu.h"' in src and "typedef" not in src and "LTR_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for ret, name, params in decls:
        restype, argtypes = _abi.PLOIDY_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        check_type(ret, restype, name)
        for i, (p, ct) in enumerate(zip(params, argtypes)):
            m = re.match(r"(.*?)(\w+)\s*$", p)
            check_type(m.group(1), ct, (name, i))
    assert [p.split()[-1].lstrip("*") for p in decls[1][2]] == ["plan", "gb", "fr", "sample_haploid", "out"]
    assert decls[3][0] == "int32_t" and len(decls[3][2]) == 3


def test_lib_binds_them_with_the_tables_types():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.PLOIDY_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # bad handles are refused without a device
    assert L.ltr_genotype_result_sample_haploid(None, 0, 0) < 0
    assert L.ltr_plan_genotype_sample_ploidy(None, None, None, None, None) == _abi.LTR_ERR_INVALID
    assert L.ltr_ll_genotype_sample_ploidy(None, None, None, None, None, None) == _abi.LTR_ERR_INVALID
    assert L.ltr_plan_posteriors_sample_ploidy(None, None, None, None, None, None) == _abi.LTR_ERR_INVALID


def test_sample_haploid_is_checked_by_the_binding():
    ns = np.asarray([2, 1, 3], dtype=np.int32)
    flat = _genotype._sample_haploid([[1, 0], [1], [0, 5, 0]], ns)
    assert flat.dtype == np.uint8 and flat[:6].tolist() == [1, 0, 1, 0, 1, 0]
    with pytest.raises(_lib.LtrError) as e:                      # the ploidy is given once
        _genotype._sample_haploid([[1, 0], [1], [0, 1, 0]], ns, locus_haploid=[0, 1, 0])
    assert e.value.code == _abi.LTR_ERR_INVALID and "locus_haploid" in str(e.value)
    for wrong, text in (([[1, 0], [1]], "one array per locus"), ([[1, 0], [1, 1], [0, 1, 0]], "locus 1 has 1 samples, got 2"),
                        ([[1], [1], [0, 1, 0]], "locus 0 has 2 samples, got 1")):
        with pytest.raises(_lib.LtrError) as e:
            _genotype._sample_haploid(wrong, ns)
        assert e.value.code == _abi.LTR_ERR_INVALID and text in str(e.value), str(e.value)
    import inspect
    from longtr_amd import _context
    for fn in (_genotype.Plan.posteriors, _genotype.Plan.genotype, _genotype.Plan.genotype_packed, _genotype.Plan.genotype_fields,
               _context.Context.genotype_ll):
        p = inspect.signature(fn).parameters
        assert "sample_haploid" in p and p["sample_haploid"].default is None and "locus_haploid" in p, fn


def _write(tmp_path, text, name="ploidy.tsv"):
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_the_ploidy_file(tmp_path):
    path = _write(tmp_path, "# sample\tchrom\tploidy\nHG002\tchrX\t1\n\nHG003\tchrX\t1   # the father\nHG004\tchrX\t2\nHG002\tchrY\t1\n")
    table = call.read_sample_ploidy(path, samples=["HG002", "HG003", "HG004"])
    assert table == {("HG002", "chrX"): 1, ("HG003", "chrX"): 1, ("HG004", "chrX"): 2, ("HG002", "chrY"): 1}
    assert call.read_sample_ploidy(None) == {} and call.read_sample_ploidy(_write(tmp_path, "# nothing\n\n", "empty.tsv")) == {}
    assert call.read_sample_ploidy({("A", "chr1"): 1}) == {("A", "chr1"): 1}
    # a pair the file does not name follows --haploid-chrs; a pair it names does not
    hap = {"chrX", "chrY"}
    assert call.sample_ploidy(table, hap, "HG004", "chrX") == 2 and call.sample_ploidy(table, hap, "HG004", "chrY") == 1
    assert call.sample_ploidy(table, hap, "HG003", "chr1") == 2 and call.sample_ploidy(table, set(), "HG002", "chrX") == 1
    for text, needle in (("HG002\tchrX\t0\n", "ploidy is 1 or 2"), ("HG002\tchrX\t3\n", "ploidy is 1 or 2"), ("HG002\tchrX\n", "expected"),
                         ("HG002 chrX 1\n", "expected"), ("HG002\tchrX\t1\t9\n", "expected"), ("HG002\t\t1\n", "expected"),
                         ("HG002\tchrX\tone\n", "ploidy is 1 or 2")):
        with pytest.raises(_lib.LtrError) as e:
            call.read_sample_ploidy(_write(tmp_path, "HG003\tchrX\t1\n" + text, "bad.tsv"))
        assert e.value.code == _abi.LTR_ERR_INVALID and needle in str(e.value) and ":2:" in str(e.value), str(e.value)
    with pytest.raises(_lib.LtrError) as e:
        call.read_sample_ploidy(path, samples=["HG002", "HG003"])
    assert e.value.code == _abi.LTR_ERR_INVALID and "HG004" in str(e.value) and "none of the BAMs" in str(e.value)
    for bad in ({("A", "chr1"): 0}, {("A", "chr1"): 3}, {("A", "chr1"): True}, {"A": 1}, {("A",): 1}):
        with pytest.raises(_lib.LtrError):
            call.read_sample_ploidy(bad)


def test_the_option_is_checked_before_anything_is_opened(tmp_path):
    assert call.DEFAULTS["sample_ploidy"] is None
    bad = _write(tmp_path, "HG002\tchrX\t4\n")
    with pytest.raises(_lib.LtrError) as e:                      # no context, no BAM, no reference: none of them is reached
        call.genotype_regions(None, ["/nonexistent.bam"], None, [], str(tmp_path / "out.vcf"), sample_ploidy=bad)
    assert e.value.code == _abi.LTR_ERR_INVALID and "ploidy is 1 or 2" in str(e.value)
    args = call.make_parser().parse_args(["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf", "--sample-ploidy", bad])
    with pytest.raises(_lib.LtrError):
        call.options_from_args(args)
    good = _write(tmp_path, "HG002\tchrX\t1\n")
    args = call.make_parser().parse_args(["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf", "--sample-ploidy", good,
                                          "--haploid-chrs", "chrY"])
    o = call.options_from_args(args)
    assert o["sample_ploidy"] == {("HG002", "chrX"): 1} and o["haploid_chrs"] == ("chrY",) and set(o) <= set(call.DEFAULTS)
    assert call.options_from_args(call.make_parser().parse_args(["--bams", "a.bam", "--fasta", "f.fa", "--regions", "r.bed", "--tr-vcf", "o.vcf"]))["sample_ploidy"] is None


def test_help_lists_the_option():
    text = call.make_parser().format_help()
    assert "--sample-ploidy" in text and "<ploidy.tsv>" in text
