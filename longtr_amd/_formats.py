"""The on-disk formats (ltr_io.cpp, ltr_bam.cpp, ltr_vcf_in.cpp; host only, no GPU needed): region files, FASTA, VCF out and in, tabix, BAM."""
import ctypes as C
import os

import numpy as np

from ._abi import BamRecord
from ._loader import Handle, LtrError, _p, lib, open_handle, text_call


def read_regions(path, max_regions=0xffffffff, chrom_limit=None, order=False):
    """ltr_read_regions (+ ltr_region_set_order): list of dicts chrom / start / stop / motif / name / period / period_str;
    the reference's "Region file contains N regions" count comes back as the second value."""
    L = lib()
    h = open_handle(L.ltr_read_regions, os.fsencode(path), int(max_regions), None if not chrom_limit else chrom_limit.encode())
    try:
        if order:
            L.ltr_region_set_order(h)
        out = []
        for i in range(L.ltr_region_set_size(h)):
            out.append(dict(chrom=L.ltr_region_chrom(h, i).decode(), start=L.ltr_region_start(h, i), stop=L.ltr_region_stop(h, i),
                            motif=L.ltr_region_motif(h, i).decode(), name=L.ltr_region_name(h, i).decode(),
                            period=L.ltr_region_period(h, i), period_str=L.ltr_region_period_str(h, i).decode()))
        return out, int(L.ltr_region_set_lines_read(h))
    finally:
        L.ltr_region_set_free(h)


class Fasta(Handle):
    """ltr_fasta: FastaReader (one indexed FASTA file or a directory of *.fa)."""

    _free = "ltr_fasta_close"

    def __init__(self, path):
        self._h = open_handle(lib().ltr_fasta_open, os.fsencode(path))

    def names(self):
        return [lib().ltr_fasta_seq_name(self._h, i).decode() for i in range(lib().ltr_fasta_num_seqs(self._h))]

    def seq_len(self, chrom):
        return int(lib().ltr_fasta_seq_len(self._h, chrom.encode()))

    def fetch(self, chrom, start, end):
        """0-based, end inclusive (FastaReader::get_sequence)."""
        cap = max(int(end) - max(int(start), 0) + 2, 1)
        buf = C.create_string_buffer(cap)
        err = C.create_string_buffer(1024)
        n = lib().ltr_fasta_fetch(self._h, chrom.encode(), int(start), int(end), buf, cap, err, len(err))
        if n < 0:
            raise LtrError(int(n), err.value.decode(errors="replace"))
        return buf.raw[:n].decode()

    def contig_lines(self):
        return text_call("ltr_fasta_contig_lines", 1 << 20, lambda buf, cap: lib().ltr_fasta_contig_lines(self._h, buf, cap))


def vcf_header(fasta_path, full_command, contig_lines, sample_names, options=None):
    """ltr_vcf_header = Genotyper::get_vcf_header (genotyper.cpp:258-336)."""
    names = (C.c_char_p * max(len(sample_names), 1))(*[n.encode() for n in sample_names])
    cap = 1 << 16
    cl = None if contig_lines is None else contig_lines.encode()
    cap += len(cl or b"") + len(fasta_path) + len(full_command) + sum(len(n) + 1 for n in sample_names)
    return text_call("ltr_vcf_header", cap, lambda buf, cap: lib().ltr_vcf_header(
        fasta_path.encode(), full_command.encode(), cl, C.byref(options) if options is not None else None, names, len(sample_names), buf, cap))


class VcfWriter:
    """ltr_vcf_writer: the reference's position-ordered VCFWriter (BGZF for *.gz / *.bgz paths)."""

    def __init__(self, path):
        self._h = C.c_void_p()
        rc = lib().ltr_vcf_writer_open(os.fsencode(path), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise LtrError(rc, "ltr_vcf_writer_open")

    def header(self, text):
        rc = lib().ltr_vcf_writer_header(self._h, text.encode())
        if rc != 0:
            raise LtrError(rc, "ltr_vcf_writer_header")

    def add_record(self, chrom, pos, text):
        rc = lib().ltr_vcf_writer_add_record(self._h, chrom.encode(), int(pos), text.encode())
        if rc != 0:
            raise LtrError(rc, "ltr_vcf_writer_add_record")

    def close(self):
        if self._h:
            h, self._h = self._h, None
            rc = lib().ltr_vcf_writer_close(h)
            if rc != 0:
                raise LtrError(rc, "ltr_vcf_writer_close")


class VcfPanel(Handle):
    """ltr_vcf_reader: a bgzipped, tabix-indexed VCF of TR alleles (--ref-vcf).  alleles(chrom, start, stop) = read_vcf_alleles:
    (pos, [REF, ALT...]) with pos 0-based, or None when the panel has no record of the region."""

    _free = "ltr_vcf_reader_close"

    def __init__(self, path):
        self._h = open_handle(lib().ltr_vcf_reader_open, os.fsencode(path), err_cap=2048)
        self._cap = 1 << 16

    def alleles(self, chrom, start, stop):
        L = lib()
        while True:
            buf = C.create_string_buffer(self._cap)
            off = np.zeros(self._cap + 1, dtype=np.int64)
            pos, n = C.c_int32(-1), C.c_int32(0)
            rc = L.ltr_vcf_read_alleles(self._h, chrom.encode(), int(start), int(stop), C.byref(pos), buf, self._cap, _p(off), C.byref(n))
            if rc == 1:
                raw = buf.raw
                return pos.value, [raw[off[i]:off[i + 1]].decode() for i in range(n.value)]
            if rc == 0:
                return None
            if self._cap >= 1 << 22:
                raise LtrError(rc, f"ltr_vcf_read_alleles {chrom}:{start}-{stop}")
            self._cap <<= 2                                      # (a too small buffer is the same status as a malformed record)

    def query_lines(self, chrom, start, end):
        """Test hook: the text lines of the records whose interval overlaps [start, end)."""
        cap = 1 << 20
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().ltr_debug_vcf_query(self._h, chrom.encode(), int(start), int(end), buf, cap)
            if n >= 0:
                return buf.raw[:n].decode().splitlines()
            if cap >= 1 << 28:
                raise LtrError(int(n), "ltr_debug_vcf_query")
            cap <<= 2


def vcf_index(path):
    """ltr_vcf_index (tabix -p vcf): writes path + ".tbi" for a position-sorted BGZF VCF."""
    rc = lib().ltr_vcf_index(os.fsencode(path))
    if rc != 0:
        raise LtrError(rc, f"ltr_vcf_index {path}")


def tbi_parse(tbi_path, max_refs=4096):
    """Test hook ltr_debug_tbi_parse: dict(format, col_seq, col_beg, col_end, meta, skip, names, bins, chunks) or LtrError."""
    header, counts = np.zeros(6, dtype=np.int32), np.zeros(2 * max_refs, dtype=np.int64)
    names = C.create_string_buffer(1 << 20)
    n = lib().ltr_debug_tbi_parse(os.fsencode(tbi_path), _p(header), _p(counts), max_refs, names, len(names))
    if n < 0:
        raise LtrError(n, f"ltr_debug_tbi_parse {tbi_path}")
    d = dict(zip(("format", "col_seq", "col_beg", "col_end", "meta", "skip"), (int(x) for x in header)))
    d["names"] = [x.decode() for x in names.raw.split(b"\0")[:n]]
    d["bins"], d["chunks"] = [int(x) for x in counts[0:2 * min(n, max_refs):2]], [int(x) for x in counts[1:2 * min(n, max_refs):2]]
    return d


class Bam(Handle):
    """ltr_bam: indexed BAM files read as one stream (BamCramMultiReader)."""

    _free = "ltr_bam_close"

    def __init__(self, paths, merge_by_position=True):
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        self._h = open_handle(lib().ltr_bam_open, arr, len(paths), int(bool(merge_by_position)), err_cap=2048)

    def refs(self):
        L = lib()
        return [(L.ltr_bam_ref_name(self._h, i).decode(), int(L.ltr_bam_ref_len(self._h, i))) for i in range(L.ltr_bam_num_refs(self._h))]

    def read_groups(self):
        L = lib()
        return [dict(id=L.ltr_bam_read_group_id(self._h, i).decode(), sample=L.ltr_bam_read_group_sample(self._h, i).decode(),
                     library=L.ltr_bam_read_group_library(self._h, i).decode(), file=L.ltr_bam_read_group_file(self._h, i))
                for i in range(L.ltr_bam_num_read_groups(self._h))]

    def fetch(self, chrom, start, end, tags=()):
        """SetRegion + GetNextAlignment until the stream ends: list of dicts."""
        L = lib()
        rc = L.ltr_bam_set_region(self._h, chrom.encode(), int(start), int(end))
        if rc != 0:
            raise LtrError(rc, "ltr_bam_set_region")
        out, rec = [], BamRecord()
        while True:
            rc = L.ltr_bam_next(self._h, C.byref(rec))
            if rc == 0:
                return out
            if rc < 0:
                raise LtrError(rc, "ltr_bam_next")
            d = dict(name=rec.name.decode(), file=rec.file_index, ref_id=rec.ref_id, pos=rec.pos, end_pos=rec.end_pos, mapq=rec.mapq, flag=rec.flag,
                     mate_ref_id=rec.mate_ref_id, mate_pos=rec.mate_pos, tlen=rec.tlen, seq=rec.bases[:rec.length].decode() if rec.length else "",
                     qual=rec.quals[:rec.length].decode("latin-1") if rec.length else "",
                     cigar=[(rec.cigar_type[k:k + 1].decode(), rec.cigar_num[k]) for k in range(rec.n_cigar)])
            for t in tags:
                v = C.c_int64()
                if L.ltr_bam_aux_int(C.byref(rec), t.encode(), C.byref(v)):
                    d[t] = int(v.value)
                else:
                    sv = L.ltr_bam_aux_string(C.byref(rec), t.encode())
                    if sv is not None:
                        d[t] = sv.decode()
            out.append(d)
