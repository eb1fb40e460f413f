"""Helpers of test_vcf_fields.py / test_gpu_plan_fields.py: numpy restatements of Genotyper::calc_gl_diff (genotyper.cpp:109-130)
and calc_PLs (:102-107) -- selection, subtraction, truncation, no libm -- and the comparison of two fields images."""
import numpy as np

EXACT = ("best_gts", "n_aligned", "n_snp", "n_s1", "n_s2", "read_allele")
ARRAYS = EXACT + ("log_phased", "log_unphased", "hap_log_phased", "hap_log_unphased", "gl_diffs", "gls", "pls", "phased_gls")


def calc_gl_diff(gls, gt, n_haps, haploid):
    """One sample: gls [n_gl], gt (a, b)."""
    if n_haps == 1:
        return -1000.0
    max_gl = gls.max()
    below = gls[gls < max_gl]
    second = below.max() if below.size else max_gl
    a, b = int(gt[0]), int(gt[1])
    idx = a if haploid else max(a, b) * (max(a, b) + 1) // 2 + min(a, b)
    return max_gl - second if abs(max_gl - gls[idx]) < 1e-10 else gls[idx] - max_gl


def calc_pls(gls):
    """One sample: (int)(-10 * (gl - max)), truncated toward zero, capped at 999."""
    v = np.trunc(-10 * (gls - gls.max()))
    return np.minimum(v, 999).astype(np.int32)


def check_self_consistent(f, n_haps, haploid):
    """gl_diffs and pls bit-identical to the restatements applied to the image's OWN gls and best_gts."""
    for s in range(f["S"]):
        d = calc_gl_diff(f["gls"][s], f["best_gts"][s], n_haps, haploid)
        assert np.float64(d).view(np.uint64) == f["gl_diffs"][s:s + 1].view(np.uint64)[0], (s, d, f["gl_diffs"][s])
        if f["pls"] is not None:
            assert np.array_equal(calc_pls(f["gls"][s]), f["pls"][s]), s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
