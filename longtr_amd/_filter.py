"""The reference's read filter for one region (include/ltr_filter.h, libltr_filter.so: host only, no GPU needed)."""
import ctypes as C
import os

import numpy as np

from ._abi import LTR_ERR_INVALID
from ._build import FILTER_LIB_PATH
from ._loader import LtrError

VERDICTS = ("PASS", "OUTSIDE", "NOT_SCANNED", "SKIPPED", "HARD_CLIPPED", "HAS_N_BASES", "LOW_BASE_QUALS", "LOW_MAPQ", "NOT_SPANNING",
            "NO_UNIQUE_MAPPING", "DUPLICATE_NAME", "PAIRED_UNSUPPORTED")
COUNTERS = ("overlapped", "hard_clipped", "has_n", "low_mapq", "low_qual", "not_spanning", "not_unique", "passed", "paired_unsupported")


class FilterOptions(C.Structure):
    """struct ltr_filter_options."""

    _fields_ = [("min_mapq", C.c_int32), ("min_mean_qual", C.c_double), ("require_spanning", C.c_int32), ("min_flank", C.c_int32),
                ("max_total_reads", C.c_int32), ("base_qual_trim", C.c_int32)]


class FilterRecord(C.Structure):
    """struct ltr_filter_record."""

    _fields_ = [("name", C.c_char_p), ("file_index", C.c_int32), ("pos", C.c_int32), ("end_pos", C.c_int32), ("mapq", C.c_int32),
                ("flag", C.c_int32), ("length", C.c_int32), ("bases", C.c_char_p), ("quals", C.c_char_p), ("n_cigar", C.c_int32),
                ("cigar_type", C.c_char_p), ("rg", C.c_char_p), ("has_xa", C.c_int32)]


class FilterSamples(C.Structure):
    """struct ltr_filter_samples."""

    _fields_ = [("use_rgs", C.c_int32), ("n_rg", C.c_int32), ("rg_id", C.POINTER(C.c_char_p)), ("rg_sample", C.POINTER(C.c_char_p)),
                ("rg_file", C.POINTER(C.c_int32)), ("n_files", C.c_int32), ("file_sample", C.POINTER(C.c_char_p))]


_vp, _i32 = C.c_void_p, C.c_int32
# name -> (return type, [parameter types]) of every function include/ltr_filter.h declares (tests/test_read_filter.py holds it to the header)
FILTER_SIGNATURES = {
    "ltr_filter_default_options": (None, [C.POINTER(FilterOptions)]),
    "ltr_filter_reads": (C.c_int, [C.POINTER(FilterRecord), _i32, _i32, _i32, C.POINTER(FilterOptions), C.POINTER(FilterSamples),
                                   C.POINTER(_vp), C.c_char_p, C.c_int]),
    "ltr_filter_result_free": (None, [_vp]),
    "ltr_filter_result_n_records": (_i32, [_vp]),
    "ltr_filter_result_verdicts": (C.POINTER(C.c_uint8), [_vp]),
    "ltr_filter_result_n_passing": (_i32, [_vp]),
    "ltr_filter_result_pass_record": (C.POINTER(C.c_int32), [_vp]),
    "ltr_filter_result_pass_sample": (C.POINTER(C.c_int32), [_vp]),
    "ltr_filter_result_pass_pf": (C.POINTER(C.c_uint8), [_vp]),
    "ltr_filter_result_n_samples": (_i32, [_vp]),
    "ltr_filter_result_sample_name": (C.c_char_p, [_vp, _i32]),
    "ltr_filter_result_counters": (C.POINTER(C.c_int32), [_vp]),
    "ltr_filter_result_too_many_reads": (_i32, [_vp]),
    "ltr_filter_verdict_name": (C.c_char_p, [_i32]),
}

_flib = None


def filter_lib():
    global _flib
    if _flib is None:
        if not os.path.exists(FILTER_LIB_PATH):
            raise ImportError(f"{FILTER_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(FILTER_LIB_PATH)
        for name, (ret, params) in FILTER_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ret, params
        _flib = L
    return _flib


def filter_options(**kw):
    """The reference's defaults (bam_processor.h:82-101) with any of min_mapq, min_mean_qual, require_spanning, min_flank,
    max_total_reads, base_qual_trim (a character or its code) replaced."""
    o = FilterOptions()
    filter_lib().ltr_filter_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(FilterOptions._fields_):
            raise TypeError(f"filter_options: no option {k}")
        setattr(o, k, ord(v) if k == "base_qual_trim" and isinstance(v, str) else v)
    return o


def _enc(s):
    return s if isinstance(s, bytes) else s.encode("latin-1")


def filter_reads(records, region_start, region_stop, options=None, read_groups=None, file_samples=None):
    """ltr_filter_reads.  records: the dicts Bam.fetch(..., tags=("RG", "XA")) returns for
    (chrom, max(0, start - 1000), stop + 1000) of a Bam opened with merge_by_position=False.
    read_groups: Bam.read_groups() -- the sample of a read is its RG tag's SM; or file_samples: one sample name per file (--bam-samps).
    Returns dict(verdicts=[names], passing=[(record index, sample index, PF)...] in output order, samples=[names],
    counters=dict, too_many_reads=bool)."""
    if (read_groups is None) == (file_samples is None):
        raise LtrError(LTR_ERR_INVALID, "filter_reads: give read_groups or file_samples")
    L = filter_lib()
    n = len(records)
    arr = (FilterRecord * max(n, 1))()
    keep = []
    for i, r in enumerate(records):
        ct = bytes(ord(t) for t, _ in r["cigar"])
        rg = r.get("RG")
        vals = (_enc(r["name"]), _enc(r["seq"]), _enc(r["qual"]), ct, None if rg is None else _enc(str(rg)))
        keep.append(vals)
        a = arr[i]
        a.name, a.file_index, a.pos, a.end_pos, a.mapq, a.flag = vals[0], r["file"], r["pos"], r["end_pos"], r["mapq"], r["flag"]
        a.length, a.bases, a.quals, a.n_cigar, a.cigar_type, a.rg, a.has_xa = len(vals[1]), vals[1], vals[2], len(ct), ct, vals[4], int("XA" in r)
    s = FilterSamples()
    if read_groups is not None:
        ids = (C.c_char_p * max(len(read_groups), 1))(*[_enc(g["id"]) for g in read_groups])
        sms = (C.c_char_p * max(len(read_groups), 1))(*[_enc(g["sample"]) for g in read_groups])
        files = np.asarray([g["file"] for g in read_groups], dtype=np.int32) if read_groups else np.zeros(1, dtype=np.int32)
        s.use_rgs, s.n_rg, s.rg_id, s.rg_sample, s.rg_file = 1, len(read_groups), ids, sms, files.ctypes.data_as(C.POINTER(C.c_int32))
    else:
        fs = (C.c_char_p * max(len(file_samples), 1))(*[_enc(x) for x in file_samples])
        s.use_rgs, s.n_files, s.file_sample = 0, len(file_samples), fs
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = L.ltr_filter_reads(arr, n, int(region_start), int(region_stop), None if options is None else C.byref(options), C.byref(s),
                            C.byref(h), err, len(err))
    if rc != 0:
        raise LtrError(rc, err.value.decode(errors="replace"))
    try:
        v, k = L.ltr_filter_result_verdicts(h), L.ltr_filter_result_n_passing(h)
        pr, ps, pf = L.ltr_filter_result_pass_record(h), L.ltr_filter_result_pass_sample(h), L.ltr_filter_result_pass_pf(h)
        cn = L.ltr_filter_result_counters(h)
        return dict(verdicts=[VERDICTS[v[i]] for i in range(n)], passing=[(pr[i], ps[i], bool(pf[i])) for i in range(k)],
                    samples=[L.ltr_filter_result_sample_name(h, i).decode() for i in range(L.ltr_filter_result_n_samples(h))],
                    counters={name: cn[i] for i, name in enumerate(COUNTERS)}, too_many_reads=bool(L.ltr_filter_result_too_many_reads(h)))
    finally:
        L.ltr_filter_result_free(h)
