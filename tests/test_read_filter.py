"""ltr_filter_reads (include/ltr_filter.h) against the Python restatement of the same reference lines (tests/read_filter_util.py):
the bundled trio BAMs at every region of the bundled BED, and one hand-made record per edge.  No GPU."""
import ctypes as C
import os
import re

import pytest

import read_filter_util as U
from longtr_amd import _filter, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "bam")
SAMPLES = ["HG002", "HG003", "HG004"]


def bundled_regions():
    out = []
    for line in open(os.path.join(DATA, "test_regions_hg38.bed")):
        c = line.split()
        if len(c) >= 3:
            out.append((c[0], int(c[1]) - 1, int(c[2])))          # readRegions stores START 0-based (region.cpp:26-65)
    return out


@pytest.fixture(scope="module")
def trio():
    """(read groups, [(region, records)...]): the records of every region, file by file, fetched once."""
    bam = _lib.Bam([os.path.join(DATA, f"{s}_sample_reads.bam") for s in SAMPLES], merge_by_position=False)
    rgs = bam.read_groups()
    loci = [((c, a, b), bam.fetch(c, max(0, a - 1000), b + 1000, tags=("RG", "XA"))) for c, a, b in bundled_regions()]
    bam.close()
    assert len(loci) >= 30 and sum(len(r) for _, r in loci) > 500
    return rgs, loci


def same(lib, ref):
    assert lib["verdicts"] == ref["verdicts"]
    assert lib["passing"] == ref["passing"]                      # output order, sample index, PF
    assert lib["samples"] == ref["samples"]
    assert lib["counters"] == ref["counters"]
    assert lib["too_many_reads"] == ref["too_many_reads"]


def moved_thresholds(trio):
    _, loci = trio
    (_, a, b), recs = loci[0]
    over = [r for r in recs if r["pos"] < b and r["end_pos"] >= a and r["seq"]]
    assert over
    all_fail = max(U.mean_quality(r["qual"]) for r in over) + 1
    return [dict(), dict(min_mapq=61), dict(min_mean_qual=all_fail), dict(require_spanning=0), dict(min_flank=0), dict(min_flank=500)]


def test_bundled_trio_equals_the_restatement(trio):
    rgs, loci = trio
    seen = set()
    for k, options in enumerate(moved_thresholds(trio)):
        passed = pf_set = 0
        for (chrom, a, b), recs in loci:
            ref = U.filter_reads(recs, a, b, read_groups=rgs, **options)
            same(_filter.filter_reads(recs, a, b, _filter.filter_options(**options), read_groups=rgs), ref)
            seen.update(ref["verdicts"])
            passed += len(ref["passing"])
            pf_set += sum(pf for _, _, pf in ref["passing"])
        if k == 0:
            assert passed > 300 and pf_set > 0                   # the defaults keep most of the trio's reads
            default_passed, default_pf = passed, pf_set
        if options == dict(min_mapq=61):
            assert passed == 0                                   # MAPQ is at most 60: the threshold bites everywhere
        if "min_mean_qual" in options:
            (_, a, b), recs = loci[0]
            assert U.filter_reads(recs, a, b, read_groups=rgs, **options)["passing"] == [] and passed < default_passed
        if options == dict(require_spanning=0):
            assert passed >= default_passed
        if options == dict(min_flank=0):
            assert passed == default_passed and pf_set == passed
        if options == dict(min_flank=500):
            assert passed == default_passed and pf_set < default_pf
    assert {"PASS", "OUTSIDE", "LOW_MAPQ", "LOW_BASE_QUALS"} <= seen


def test_bundled_trio_by_file_samples(trio):
    """--bam-samps: the sample of a read is that of its file."""
    _, loci = trio
    names = ["c", "a", "b"]
    for (chrom, a, b), recs in loci[:8]:
        ref = U.filter_reads(recs, a, b, file_samples=names)
        same(_filter.filter_reads(recs, a, b, file_samples=names), ref)
        assert set(ref["samples"]) <= set(names)


CASES = U.hand_made_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made_edge(case):
    name, recs, options, tables, want = case
    if want.get("error"):
        with pytest.raises(U.FilterDie) as e:
            U.filter_reads(recs, U.START, U.STOP, **tables, **options)
        assert str(e.value) == want["error"]
        with pytest.raises(_lib.LtrError) as e:
            _filter.filter_reads(recs, U.START, U.STOP, _filter.filter_options(**options), **tables)
        assert e.value.code == -1 and want["error"] in str(e.value)
        return
    ref = U.filter_reads(recs, U.START, U.STOP, **tables, **options)
    got = _filter.filter_reads(recs, U.START, U.STOP, _filter.filter_options(**options), **tables)
    same(got, ref)
    assert got["verdicts"] == want["verdicts"]                   # and both say what the case was made to show
    assert [(i, pf) for i, _, pf in got["passing"]] == want["passing"]
    assert got["too_many_reads"] == want.get("too_many_reads", False)


def test_eleven_files_sort_as_strings():
    """"10_" and "11_" sort before "2_": files ten and eleven are handed out LAST (the walk is from the back)."""
    name, recs, options, tables, want = next(c for c in CASES if c[0] == "eleven_files_key_order")
    got = _filter.filter_reads(recs, U.START, U.STOP, **tables)
    assert got["samples"] == ["F8", "F7", "F6", "F5", "F4", "F3", "F2", "F1", "F0", "F10", "F9"]


def test_defaults_are_the_reference_s():
    o = _filter.filter_options()
    assert (o.min_mapq, o.min_mean_qual, o.require_spanning, o.min_flank, o.max_total_reads, chr(o.base_qual_trim)) == (20, 30.0, 1, 5, 1000000, "5")
    assert {k: getattr(o, k) if k != "base_qual_trim" else chr(o.base_qual_trim) for k in U.DEFAULTS} == U.DEFAULTS


def test_signature_table_matches_the_header():
    """Every function include/ltr_filter.h declares is in _filter.FILTER_SIGNATURES with as many parameters, and is exported."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltr_filter.h")).read(), flags=re.S)
    decls = {m.group(1): [p for p in m.group(2).split(",") if p.strip() not in ("", "void")]
             for m in re.finditer(r"\b(ltr_filter_\w+)\s*\(([^()]*)\)\s*;", src)}
    assert set(decls) == set(_filter.FILTER_SIGNATURES) and len(decls) == 14
    L = _filter.filter_lib()
    for name, params in decls.items():
        restype, argtypes = _filter.FILTER_SIGNATURES[name]
        assert len(argtypes) == len(params), name
        for p, ct in zip(params, argtypes):
            assert ("*" in p) == (ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer)), (name, p)
        assert getattr(L, name).argtypes == argtypes
    assert [L.ltr_filter_verdict_name(i).decode() for i in range(len(_filter.VERDICTS))] == list(_filter.VERDICTS)
    assert L.ltr_filter_verdict_name(99) == b""


def test_gpu_library_is_untouched():
    """The filter is a library of its own: it adds nothing to libltr_gpu.so's table or ABI version."""
    assert not [n for n in _lib.SIGNATURES if n.startswith("ltr_filter")]
    assert _lib.lib().ltr_abi_version() == 6
