"""Phasing priors of reads from a phased SNP VCF (include/ltr_snp.h, libltr_snp.so: host only, no GPU needed).

The library reads no file: PhasedSnps hands it the text the tabix-indexed reader of libltr_gpu.so delivers."""
import ctypes as C
import gzip
import os

import numpy as np

from ._abi import LTR_ERR_INVALID, SNP_SIGNATURES, SnpRead
from ._build import SNP_LIB_PATH
from ._formats import VcfPanel, tbi_parse
from ._loader import LtrError, _p

MAX_MATE_DIST = 1000      # the window of SNPs either side of a region (snp_bam_processor.cpp:61)
SKIP_PADDING = 15         # snp_bam_processor.h:54
N_QUALITIES = 42          # LTR_SNP_N_QUALITIES

_slib = None


def snp_lib():
    global _slib
    if _slib is None:
        if not os.path.exists(SNP_LIB_PATH):
            raise ImportError(f"{SNP_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(SNP_LIB_PATH)
        for name, (ret, params) in SNP_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ret, params
        _slib = L
    return _slib


def quality_tables():
    """Test hook: (log_correct, log_error), the two tables of BaseQuality (index = quality - '!')."""
    c, e = np.zeros(N_QUALITIES), np.zeros(N_QUALITIES)
    snp_lib().ltr_snp_debug_quality_tables(_p(c), _p(e))
    return c, e


def _enc(s):
    return s if isinstance(s, bytes) else s.encode()


def _raw(s):                                                     # bases and qualities: one byte per character
    return s if isinstance(s, bytes) else s.encode("latin-1")


class SnpSet:
    """ltr_snp_set: the phased heterozygous SNPs of one window, per sample column of the VCF."""

    def __init__(self, header_line, record_lines, skip_regions=(), skip_padding=SKIP_PADDING):
        """header_line: the #CHROM line.  record_lines: the records' text (lines ending in \\n) or a list of lines.
        skip_regions: (start, stop) pairs, as the region file gives them."""
        self._h = None
        text = _enc(record_lines) if isinstance(record_lines, (str, bytes)) else b"".join(_enc(t) + b"\n" for t in record_lines)
        a = np.asarray([s for s, _ in skip_regions], dtype=np.int32)
        b = np.asarray([s for _, s in skip_regions], dtype=np.int32)
        h, err = C.c_void_p(), C.create_string_buffer(1024)
        rc = snp_lib().ltr_snp_set_create(_enc(header_line), text, len(text), _p(a), _p(b), len(a), int(skip_padding), C.byref(h), err, len(err))
        if rc != 0:
            raise LtrError(rc, err.value.decode(errors="replace"))
        self._h = h

    def close(self):
        if self._h:
            snp_lib().ltr_snp_set_free(self._h)
            self._h = None

    def __del__(self):
        try:                                                     # (interpreter shutdown, or an __init__ that did not finish)
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def samples(self):
        L = snp_lib()
        return [L.ltr_snp_set_sample_name(self._h, i).decode() for i in range(L.ltr_snp_set_n_samples(self._h))]

    @property
    def n_valid_snps(self):
        return int(snp_lib().ltr_snp_set_n_valid_snps(self._h))

    def sample_index(self, name):
        """The column of a sample name (the last of several columns of that name), -1 when the VCF has none."""
        return int(snp_lib().ltr_snp_set_sample_index(self._h, _enc(name)))

    def snps(self, column):
        """[(pos 0-based, base_one, base_two)...] of a column, in the order the sums run."""
        L = snp_lib()
        n = L.ltr_snp_set_n_snps(self._h, int(column))
        if n < 0:
            raise LtrError(LTR_ERR_INVALID, f"SnpSet.snps: no column {column}")
        pos, b1, b2 = np.zeros(max(n, 1), dtype=np.int32), C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(n, 1))
        n = L.ltr_snp_set_snps(self._h, int(column), _p(pos), b1, b2, n)
        return [(int(pos[i]), b1.raw[i:i + 1].decode("latin-1"), b2.raw[i:i + 1].decode("latin-1")) for i in range(n)]

    def priors(self, column, reads, counts=None):
        """ltr_snp_phasing_priors: (log_p1, log_p2) of the reads of ONE sample against a column (-1: zeros).  reads: dicts with pos,
        end_pos, bases, quals (bytes or str, Phred + 33) and cigar [(type, length)...].  counts: an int32 array of 3 that is added to
        (bases equal to base_one, to base_two, to neither)."""
        n = len(reads)
        arr, keep = (SnpRead * max(n, 1))(), []
        for i, r in enumerate(reads):
            ct = bytes(ord(t) for t, _ in r["cigar"])
            cn = np.asarray([k for _, k in r["cigar"]], dtype=np.int32)
            vals = (_raw(r["bases"]), _raw(r["quals"]), ct, cn)
            keep.append(vals)
            a = arr[i]
            a.pos, a.end_pos, a.length, a.bases, a.quals = r["pos"], r["end_pos"], len(vals[0]), vals[0], vals[1]
            a.n_cigar, a.cigar_type, a.cigar_num = len(ct), ct, cn.ctypes.data_as(C.POINTER(C.c_int32))
        p1, p2, err = np.zeros(n), np.zeros(n), C.create_string_buffer(512)
        if counts is not None and not (isinstance(counts, np.ndarray) and counts.dtype == np.int32 and counts.size == 3 and counts.flags.c_contiguous):
            raise LtrError(LTR_ERR_INVALID, "SnpSet.priors: counts is a contiguous int32 array of 3")
        rc = snp_lib().ltr_snp_phasing_priors(self._h, int(column), arr, n, _p(p1), _p(p2), _p(counts), err, len(err))
        if rc != 0:
            raise LtrError(rc, err.value.decode(errors="replace"))
        return p1, p2


def snp_window(region_start, region_stop):
    """The 0-based half-open interval of SNPs of a region: the reference asks tabix for chrom:a-b, 1-based and closed, with
    a = start - 1000 if start > 1000 else 1 and b = stop + 1000 (snp_bam_processor.cpp:61)."""
    a = region_start - MAX_MATE_DIST if region_start > MAX_MATE_DIST else 1
    return a - 1, region_stop + MAX_MATE_DIST


class PhasedSnps:
    """A bgzipped, tabix-indexed VCF of phased SNPs (--phased-snps).  The record lines of a window come from the tabix query of
    ltr_vcf_reader (VcfPanel.query_lines), the #CHROM line from the start of the BGZF stream, the chromosomes from the index."""

    def __init__(self, path):
        self.path, self._panel = path, None
        self._panel = VcfPanel(path)                             # (refuses a file that is not BGZF, has no or a stale .tbi, or does not start like a VCF)
        try:
            self.chromosomes = tbi_parse(os.fsdecode(path) + ".tbi")["names"]
            self.header_line = None
            with gzip.open(path, "rb") as fh:                    # (a BGZF file is a gzip file of many members)
                for line in fh:
                    if not line.startswith(b"#"):
                        break
                    if line.startswith(b"#CHROM"):
                        self.header_line = line.decode(errors="replace").rstrip("\r\n")
                        break
            if self.header_line is None:
                raise LtrError(LTR_ERR_INVALID, f"{path}: no #CHROM line")
            self.samples = self.header_line.split("\t")[9:]
        except BaseException:
            self.close()
            raise

    def close(self):
        if self._panel is not None:
            self._panel.close()
            self._panel = None

    def has_chromosome(self, chrom):
        return chrom in self.chromosomes

    def window(self, chrom, region_start, region_stop, skip_padding=SKIP_PADDING):
        """The SnpSet of a region: the SNPs within 1000 bp of it that are not within skip_padding of it."""
        lo, hi = snp_window(region_start, region_stop)
        return SnpSet(self.header_line, self._panel.query_lines(chrom, lo, hi), [(region_start, region_stop)], skip_padding)

    def priors(self, snp_set, sample_name, raw_reads, counts=None):
        """(log_p1, log_p2) of one sample's reads; zeros for a sample the VCF does not hold."""
        return snp_set.priors(snp_set.sample_index(sample_name), raw_reads, counts)
