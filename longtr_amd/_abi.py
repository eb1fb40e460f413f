"""ctypes mirror of include/ltr_gpu.h (structs + flattening helpers + the signature of every function).

Pure data-layout code: no compute lives here.  The product binding
(longtr_amd/_lib.py and the modules behind it) uses these structs; the test-side
checker reuses them so that the same flattened inputs go to both sides.
SIGNATURES at the end is the one place a C signature is written down in Python:
_loader.lib() applies it to the loaded library once, through bind().
"""
import ctypes as C

import numpy as np

LTR_OK = 0
LTR_ERR_INVALID = -1
LTR_ERR_NO_DEVICE = -2
LTR_ERR_HIP = -3
LTR_ERR_NOMEM = -4
LTR_ERR_CIGAR = -5
LTR_ERR_UNSUPPORTED = -6

LTR_IMPOSSIBLE = -1000000000.0
LTR_ABORT_SCORE = -700.0


class AlignParams(C.Structure):
    """struct ltr_align_params (reference: AlignmentModel, HapAligner.h:12-37)."""

    _fields_ = [
        ("log_ins_to_ins", C.c_float),
        ("log_ins_to_match", C.c_float),
        ("log_del_to_del", C.c_float),
        ("log_del_to_match", C.c_float),
        ("log_match_to_match", C.c_float),
        ("log_match_to_ins", C.c_float),
        ("log_match_to_del", C.c_float),
        ("indel_flank_len", C.c_int32),
        ("use_short_path", C.c_int32),
    ]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


def default_params():
    """Defaults of HapAligner.h:118 (double literals narrowed to float) + INDEL_FLANK_LEN 5."""
    p = AlignParams()
    vals = (-1.0, -0.458675, -1.0, -0.458675, -0.00005800168, -10.448214728, -10.448214728)
    for (name, _), v in zip(AlignParams._fields_[:7], vals):
        setattr(p, name, float(np.float32(v)))
    p.indel_flank_len = 5
    p.use_short_path = 0
    return p


def make_params(values7, indel_flank_len=5, use_short_path=0):
    """--alignment-params a,b,c,d,e,f,g (strings parsed like std::stof -> float32)."""
    p = AlignParams()
    for (name, _), v in zip(AlignParams._fields_[:7], values7):
        setattr(p, name, float(np.float32(v)))
    p.indel_flank_len = indel_flank_len
    p.use_short_path = use_short_path
    return p


class LocusBatch(C.Structure):
    """struct ltr_locus_batch."""

    _fields_ = [
        ("n_loci", C.c_int64),
        ("locus_read_off", C.POINTER(C.c_int64)),
        ("locus_hap_off", C.POINTER(C.c_int64)),
        ("n_reads", C.c_int64),
        ("read_bytes", C.POINTER(C.c_uint8)),
        ("read_off", C.POINTER(C.c_int64)),
        ("n_haps", C.c_int64),
        ("hap_bytes", C.POINTER(C.c_uint8)),
        ("hap_off", C.POINTER(C.c_int64)),
        ("realign_read", C.POINTER(C.c_uint8)),
        ("realign_hap", C.POINTER(C.c_uint8)),
    ]


class GenotypeFields(C.Structure):
    """struct ltr_genotype_fields (every pointer optional)."""

    _fields_ = [
        ("best_gts", C.c_void_p),
        ("log_phased_posteriors", C.c_void_p),
        ("log_unphased_posteriors", C.c_void_p),
        ("hap_log_phased_posteriors", C.c_void_p),
        ("hap_log_unphased_posteriors", C.c_void_p),
        ("gls", C.c_void_p),
        ("gl_diffs", C.c_void_p),
        ("pls", C.c_void_p),
        ("phased_gls", C.c_void_p),
    ]


def genotype_field_buffers(n_samples, n_variants, haploid, want=("gls", "gl_diffs", "pls", "phased_gls")):
    """Allocate numpy outputs for ltr_extract_genotypes; returns (GenotypeFields, dict of arrays)."""
    import numpy as np
    S, V = n_samples, n_variants
    n_gl = V if haploid else V * (V + 1) // 2
    n_pgl = V if haploid else V * V
    arrs = {
        "best_gts": np.full((S, 2), -1, dtype=np.int32),
        "log_phased_posteriors": np.full(S, np.nan), "log_unphased_posteriors": np.full(S, np.nan),
        "hap_log_phased_posteriors": np.full(S, np.nan), "hap_log_unphased_posteriors": np.full(S, np.nan),
    }
    if "gls" in want:
        arrs["gls"] = np.full((S, n_gl), np.nan)
    if "gl_diffs" in want:
        arrs["gl_diffs"] = np.full(S, np.nan)
    if "pls" in want:
        arrs["pls"] = np.full((S, n_gl), -1, dtype=np.int32)
    if "phased_gls" in want:
        arrs["phased_gls"] = np.full((S, n_pgl), np.nan)
    f = GenotypeFields()
    for k, a in arrs.items():
        setattr(f, k, a.ctypes.data_as(C.c_void_p))
    return f, arrs


class PosteriorBatch(C.Structure):
    """struct ltr_posterior_batch."""

    _fields_ = [
        ("n_loci", C.c_int64),
        ("locus_read_off", C.POINTER(C.c_int64)),
        ("n_reads", C.c_int64),
        ("pool_index", C.POINTER(C.c_int32)),
        ("log_p1", C.POINTER(C.c_double)),
        ("log_p2", C.POINTER(C.c_double)),
        ("sample_label", C.POINTER(C.c_int32)),
        ("n_samples", C.POINTER(C.c_int32)),
        ("haploid", C.c_int32),
    ]


class HaplotypeBlocks(C.Structure):
    """struct ltr_haplotype_blocks."""

    _fields_ = [
        ("n_blocks", C.c_int32),
        ("block_start", C.POINTER(C.c_int32)),
        ("block_end", C.POINTER(C.c_int32)),
        ("is_repeat", C.POINTER(C.c_uint8)),
        ("period", C.POINTER(C.c_int32)),
        ("n_alleles", C.POINTER(C.c_int32)),
        ("allele_bytes", C.POINTER(C.c_uint8)),
        ("allele_off", C.POINTER(C.c_int64)),
    ]


class GenotypeBatch(C.Structure):
    """struct ltr_genotype_batch."""

    _fields_ = [
        ("pb", C.POINTER(PosteriorBatch)),
        ("haps", C.POINTER(C.POINTER(HaplotypeBlocks))),
        ("sample_filtered", C.POINTER(C.c_uint8)),
        ("prune", C.c_int32),
        ("want_read_ll", C.c_int32),
    ]


class FieldsRequest(C.Structure):
    """struct ltr_fields_request."""

    _fields_ = [("block", C.POINTER(C.c_int32)), ("want_gls", C.c_int32), ("want_pls", C.c_int32), ("want_phased_gls", C.c_int32),
                ("want_posteriors", C.c_int32)]


class LlBatch(C.Structure):
    """struct ltr_ll_batch."""

    _fields_ = [("log_aln_probs", C.POINTER(C.POINTER(C.c_double))), ("seed_positions", C.POINTER(C.POINTER(C.c_int32))),
                ("n_haps", C.POINTER(C.c_int32))]


class SeqGroups(C.Structure):
    """struct ltr_seq_groups."""

    _fields_ = [("n_groups", C.c_int64), ("group_seq_off", C.POINTER(C.c_int64)), ("n_seqs", C.c_int64), ("seq_bytes", C.POINTER(C.c_uint8)),
                ("seq_off", C.POINTER(C.c_int64))]


class HapBuildLocus(C.Structure):
    """struct ltr_hap_build_locus."""

    _fields_ = [("rs", C.c_void_p), ("n_samples", C.c_int32), ("region_start", C.c_int32), ("region_stop", C.c_int32), ("period", C.c_int32),
                ("chrom_seq", C.POINTER(C.c_uint8)), ("chrom_seq_start", C.c_int64), ("chrom_seq_len", C.c_int64), ("chrom_len", C.c_int64)]


class LocusFields(C.Structure):
    """struct ltr_locus_fields."""

    _I32, _F64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    _fields_ = [("S", C.c_int32), ("R", C.c_int32), ("V", C.c_int32), ("block", C.c_int32), ("n_gl", C.c_int32), ("n_pgl", C.c_int32),
                ("best_gts", _I32), ("log_phased", _F64), ("log_unphased", _F64), ("hap_log_phased", _F64), ("hap_log_unphased", _F64),
                ("gl_diffs", _F64), ("gls", _F64), ("pls", _I32), ("phased_gls", _F64),
                ("n_aligned", _I32), ("n_snp", _I32), ("n_s1", _I32), ("n_s2", _I32), ("read_allele", _I32)]

    _SHAPES = dict(best_gts=lambda f: (f.S, 2), log_phased=lambda f: (f.S,), log_unphased=lambda f: (f.S,), hap_log_phased=lambda f: (f.S,),
                   hap_log_unphased=lambda f: (f.S,), gl_diffs=lambda f: (f.S,), gls=lambda f: (f.S, f.n_gl), pls=lambda f: (f.S, f.n_gl),
                   phased_gls=lambda f: (f.S, f.n_pgl), n_aligned=lambda f: (f.S,), n_snp=lambda f: (f.S,), n_s1=lambda f: (f.S,),
                   n_s2=lambda f: (f.S,), read_allele=lambda f: (f.R,))

    def to_dict(self):
        """Copies: dict(S, R, V, block, n_gl, n_pgl, <array name>: numpy array or None)."""
        import numpy as np
        d = dict(S=self.S, R=self.R, V=self.V, block=self.block, n_gl=self.n_gl, n_pgl=self.n_pgl)
        for name, shape in self._SHAPES.items():
            ptr, sh = getattr(self, name), shape(self)
            dt = np.int32 if name in ("best_gts", "pls", "n_aligned", "n_snp", "n_s1", "n_s2", "read_allele") else np.float64
            if not ptr:
                d[name] = None
            elif int(np.prod(sh)) == 0:
                d[name] = np.zeros(sh, dtype=dt)
            else:
                d[name] = np.ctypeslib.as_array(ptr, shape=(int(np.prod(sh)),)).astype(dt, copy=True).reshape(sh)
        return d

    @classmethod
    def from_dict(cls, d):
        """(struct, the arrays it points into) from a to_dict() image (None = NULL)."""
        import numpy as np
        f, keep = cls(), []
        for k in ("S", "R", "V", "block", "n_gl", "n_pgl"):
            setattr(f, k, int(d[k]))
        for name in cls._SHAPES:
            a = d.get(name)
            if a is None:
                continue
            dt = np.int32 if name in ("best_gts", "pls", "n_aligned", "n_snp", "n_s1", "n_s2", "read_allele") else np.float64
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size == 0:
                a = np.zeros(1, dtype=dt)                        # (a valid pointer for an empty array)
            keep.append(a)
            setattr(f, name, a.ctypes.data_as(cls._I32 if dt == np.int32 else cls._F64))
        return f, keep


def blocks_from_struct(b):
    """A struct ltr_haplotype_blocks as the list of dicts PackedHaplotype takes."""
    blocks, k = [], 0
    for i in range(b.n_blocks):
        al = []
        for _ in range(b.n_alleles[i]):
            al.append(bytes(b.allele_bytes[b.allele_off[k]:b.allele_off[k + 1]]))
            k += 1
        blocks.append(dict(start=b.block_start[i], end=b.block_end[i], is_repeat=bool(b.is_repeat[i]), period=b.period[i], alleles=al))
    return blocks


class Alignment(C.Structure):
    """struct ltr_alignment (reference: class Alignment, AlignmentData.h:28-140)."""

    _fields_ = [
        ("start", C.c_int32),
        ("stop", C.c_int32),
        ("seq", C.POINTER(C.c_uint8)),
        ("seq_len", C.c_int32),
        ("n_cigar", C.c_int32),
        ("cigar_type", C.c_char_p),
        ("cigar_num", C.POINTER(C.c_int32)),
        ("qual", C.POINTER(C.c_uint8)),
    ]


class StutterParams(C.Structure):
    """struct ltr_stutter_params (reference: StutterModel, stutter_model.h:35-62)."""

    _fields_ = [("in_geom", C.c_double), ("in_up", C.c_double), ("in_down", C.c_double),
                ("out_geom", C.c_double), ("out_up", C.c_double), ("out_down", C.c_double)]


def default_stutter_params():
    """hipstr_main.cpp:140,362-363: the CLI always installs this fixed model."""
    return StutterParams(0.95, 0.05, 0.05, 0.95, 0.01, 0.01)


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def _concat(seqs):
    """list of bytes -> (uint8 array, int64 offsets[n+1])."""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs])
    buf = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if off[-1] > 0 else np.zeros(1, dtype=np.uint8)
    return buf, off


class PackedBatch:
    """Flattened loci: keeps the numpy buffers alive next to the ctypes struct."""

    def __init__(self, loci, realign_read=None, realign_hap=None):
        """loci: list of (reads: list[bytes], haps: list[bytes])."""
        reads, haps = [], []
        lro, lho = [0], [0]
        for rs, hs in loci:
            reads.extend(rs)
            haps.extend(hs)
            lro.append(len(reads))
            lho.append(len(haps))
        self.locus_read_off = np.asarray(lro, dtype=np.int64)
        self.locus_hap_off = np.asarray(lho, dtype=np.int64)
        self.read_bytes, self.read_off = _concat(reads)
        self.hap_bytes, self.hap_off = _concat(haps)
        self.realign_read = None if realign_read is None else np.ascontiguousarray(realign_read, dtype=np.uint8)
        self.realign_hap = None if realign_hap is None else np.ascontiguousarray(realign_hap, dtype=np.uint8)
        self.n_loci = len(loci)
        self.n_reads = len(reads)
        self.n_haps = len(haps)
        P = np.diff(self.locus_read_off)
        H = np.diff(self.locus_hap_off)
        self.ll_off = np.zeros(self.n_loci + 1, dtype=np.int64)
        self.ll_off[1:] = np.cumsum(P * H)
        self.ll_size = int(self.ll_off[-1])
        b = LocusBatch()
        b.n_loci = self.n_loci
        b.locus_read_off = _ptr(self.locus_read_off, C.c_int64)
        b.locus_hap_off = _ptr(self.locus_hap_off, C.c_int64)
        b.n_reads = self.n_reads
        b.read_bytes = _ptr(self.read_bytes, C.c_uint8)
        b.read_off = _ptr(self.read_off, C.c_int64)
        b.n_haps = self.n_haps
        b.hap_bytes = _ptr(self.hap_bytes, C.c_uint8)
        b.hap_off = _ptr(self.hap_off, C.c_int64)
        b.realign_read = _ptr(self.realign_read, C.c_uint8) if self.realign_read is not None else None
        b.realign_hap = _ptr(self.realign_hap, C.c_uint8) if self.realign_hap is not None else None
        self.struct = b

    def locus_matrix(self, ll, l):
        """View of locus l's [P x H] matrix inside a flat LL buffer."""
        P = int(self.locus_read_off[l + 1] - self.locus_read_off[l])
        H = int(self.locus_hap_off[l + 1] - self.locus_hap_off[l])
        return ll[self.ll_off[l]:self.ll_off[l + 1]].reshape(P, H)


class PackedHaplotype:
    """blocks: list of dict(start, end, is_repeat, period, alleles=[bytes, ...])."""

    def __init__(self, blocks):
        self.blocks = blocks
        nb = len(blocks)
        self.block_start = np.asarray([b["start"] for b in blocks], dtype=np.int32)
        self.block_end = np.asarray([b["end"] for b in blocks], dtype=np.int32)
        self.is_repeat = np.asarray([1 if b.get("is_repeat") else 0 for b in blocks], dtype=np.uint8)
        self.period = np.asarray([b.get("period", 0) for b in blocks], dtype=np.int32)
        self.n_alleles = np.asarray([len(b["alleles"]) for b in blocks], dtype=np.int32)
        seqs = [a for b in blocks for a in b["alleles"]]
        self.allele_bytes, self.allele_off = _concat(seqs)
        h = HaplotypeBlocks()
        h.n_blocks = nb
        h.block_start = _ptr(self.block_start, C.c_int32)
        h.block_end = _ptr(self.block_end, C.c_int32)
        h.is_repeat = _ptr(self.is_repeat, C.c_uint8)
        h.period = _ptr(self.period, C.c_int32)
        h.n_alleles = _ptr(self.n_alleles, C.c_int32)
        h.allele_bytes = _ptr(self.allele_bytes, C.c_uint8)
        h.allele_off = _ptr(self.allele_off, C.c_int64)
        self.struct = h

    @property
    def num_combs(self):
        return int(np.prod(self.n_alleles.astype(np.int64)))


class PackedAlignments:
    """alns: list of dict(start, stop, seq=bytes, cigar=[(type_char, num), ...])."""

    def __init__(self, alns):
        self.alns = alns
        n = len(alns)
        self._keep = []
        arr = (Alignment * max(n, 1))()
        for i, a in enumerate(alns):
            seq = np.frombuffer(a["seq"], dtype=np.uint8).copy() if len(a["seq"]) else np.zeros(1, dtype=np.uint8)
            ctype = bytes(ord(t) if isinstance(t, str) else t for t, _ in a["cigar"])
            cnum = np.asarray([k for _, k in a["cigar"]], dtype=np.int32) if a["cigar"] else np.zeros(1, dtype=np.int32)
            qual = None
            if a.get("qual") is not None:
                qual = np.frombuffer(a["qual"], dtype=np.uint8).copy() if len(a["qual"]) else np.zeros(1, dtype=np.uint8)
            self._keep.append((seq, ctype, cnum, qual))
            arr[i].start = a["start"]
            arr[i].stop = a["stop"]
            arr[i].seq = _ptr(seq, C.c_uint8)
            arr[i].seq_len = len(a["seq"])
            arr[i].n_cigar = len(a["cigar"])
            arr[i].cigar_type = ctype
            arr[i].cigar_num = _ptr(cnum, C.c_int32)
            arr[i].qual = _ptr(qual, C.c_uint8) if qual is not None else None
        self.array = arr
        self.n = n


class Locus(C.Structure):
    """struct ltr_locus."""

    _fields_ = [("hap", C.POINTER(HaplotypeBlocks)), ("alns", C.POINTER(Alignment)), ("n_alns", C.c_int32),
                ("second_mate", C.POINTER(C.c_uint8)), ("realign_to_hap", C.POINTER(C.c_uint8)),
                ("realign_pool", C.POINTER(C.c_uint8)), ("copy_read", C.POINTER(C.c_uint8))]


class Timers(C.Structure):
    """struct ltr_timers."""

    _fields_ = [("hap_build_s", C.c_double), ("hap_aln_s", C.c_double), ("posterior_s", C.c_double), ("dp_kernel_ms", C.c_double),
                ("hap_build_calls", C.c_int64), ("hap_aln_calls", C.c_int64), ("posterior_calls", C.c_int64),
                ("nw_kernel_ms", C.c_double), ("short_kernel_ms", C.c_double), ("dp_cells", C.c_double), ("dp_pairs", C.c_int64)]


class VcfOptions(C.Structure):
    """struct ltr_vcf_options (Genotyper's output switches, genotyper.cpp:339-346)."""

    _fields_ = [("output_gls", C.c_int32), ("output_pls", C.c_int32), ("output_phased_gls", C.c_int32), ("output_allreads", C.c_int32),
                ("output_mallreads", C.c_int32), ("output_filters", C.c_int32), ("output_haplotype_data", C.c_int32),
                ("max_flank_indel_frac", C.c_float)]


def vcf_options(**kw):
    o = VcfOptions(0, 0, 0, 1, 1, 0, 0, 0.15)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class VcfLocus(C.Structure):
    """struct ltr_vcf_locus."""

    _fields_ = [("chrom", C.c_char_p), ("region_start", C.c_int32), ("region_stop", C.c_int32), ("name", C.c_char_p),
                ("motif", C.c_char_p), ("period_str", C.c_char_p), ("chrom_seq", C.POINTER(C.c_uint8)),
                ("chrom_seq_start", C.c_int64), ("chrom_seq_len", C.c_int64), ("hap", C.POINTER(HaplotypeBlocks)),
                ("block", C.c_int32), ("inexact_allele", C.POINTER(C.c_uint8)), ("n_reads", C.c_int32), ("n_samples", C.c_int32),
                ("haploid", C.c_int32), ("log_aln_probs", C.POINTER(C.c_double)), ("log_p1", C.POINTER(C.c_double)),
                ("log_p2", C.POINTER(C.c_double)), ("sample_label", C.POINTER(C.c_int32)), ("alns", C.POINTER(Alignment)),
                ("aln_deleted", C.POINTER(C.c_uint8)), ("log_sample_posteriors", C.POINTER(C.c_double)),
                ("sample_total_ll", C.POINTER(C.c_double)), ("best_haplotypes", C.POINTER(C.c_int32)),
                ("n_p1s", C.POINTER(C.c_int32)), ("n_p2s", C.POINTER(C.c_int32)), ("sample_names", C.POINTER(C.c_char_p)),
                ("sample_filter", C.POINTER(C.c_char_p)), ("n_out_samples", C.c_int32), ("out_sample_names", C.POINTER(C.c_char_p))]


class PackedVcfLocus:
    """Keeps every buffer of a ltr_vcf_locus alive.  d: dict with the struct's fields as python / numpy values
    (blocks = haplotype block dicts, alns = alignment dicts, strings as str)."""

    def __init__(self, d):
        self.d = d
        self.ph = PackedHaplotype(d["blocks"])
        self.pa = PackedAlignments(d["alns"]) if d.get("alns") is not None else None
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        self.keep = dict(ll=f64(d["log_aln_probs"]), p1=f64(d["log_p1"]), p2=f64(d["log_p2"]), lab=i32(d["sample_label"]),
                         post=f64(d["log_sample_posteriors"]), stl=f64(d["sample_total_ll"]), best=i32(d["best_haplotypes"]),
                         chrom_seq=np.frombuffer(d["chrom_seq"], dtype=np.uint8).copy())
        S = len(d["sample_names"])
        names = (C.c_char_p * S)(*[n.encode() for n in d["sample_names"]])
        v = VcfLocus()
        v.chrom = d["chrom"].encode()
        v.region_start, v.region_stop = d["region_start"], d["region_stop"]
        v.name = d.get("name", "").encode()
        v.motif = d.get("motif", "").encode()
        v.period_str = d.get("period_str", "").encode()
        v.chrom_seq = _ptr(self.keep["chrom_seq"], C.c_uint8)
        v.chrom_seq_start, v.chrom_seq_len = d.get("chrom_seq_start", 0), len(d["chrom_seq"])
        v.hap = C.pointer(self.ph.struct)
        v.block = d["block"]
        if d.get("inexact_allele") is not None:
            self.keep["inexact"] = u8(d["inexact_allele"])
            v.inexact_allele = _ptr(self.keep["inexact"], C.c_uint8)
        v.n_reads, v.n_samples, v.haploid = len(self.keep["p1"]), S, int(bool(d.get("haploid", False)))
        v.log_aln_probs = _ptr(self.keep["ll"], C.c_double)
        v.log_p1, v.log_p2 = _ptr(self.keep["p1"], C.c_double), _ptr(self.keep["p2"], C.c_double)
        v.sample_label = _ptr(self.keep["lab"], C.c_int32)
        if self.pa is not None:
            v.alns = self.pa.array
        if d.get("aln_deleted") is not None:
            self.keep["del"] = u8(d["aln_deleted"])
            v.aln_deleted = _ptr(self.keep["del"], C.c_uint8)
        v.log_sample_posteriors = _ptr(self.keep["post"], C.c_double)
        v.sample_total_ll = _ptr(self.keep["stl"], C.c_double)
        v.best_haplotypes = _ptr(self.keep["best"], C.c_int32)
        for k in ("n_p1s", "n_p2s"):
            if d.get(k) is not None:
                self.keep[k] = i32(d[k])
                setattr(v, k, _ptr(self.keep[k], C.c_int32))
        self.keep["names"] = names
        v.sample_names = names
        if d.get("sample_filter") is not None:
            self.keep["filt"] = (C.c_char_p * S)(*[(x or "").encode() for x in d["sample_filter"]])
            v.sample_filter = self.keep["filt"]
        if d.get("out_sample_names"):
            n = len(d["out_sample_names"])
            self.keep["out"] = (C.c_char_p * n)(*[x.encode() for x in d["out_sample_names"]])
            v.n_out_samples, v.out_sample_names = n, self.keep["out"]
        self.struct = v


class RawAlignment(C.Structure):
    """struct ltr_raw_alignment (BamAlignment fields the path reads)."""

    _fields_ = [("pos", C.c_int32), ("end_pos", C.c_int32), ("bases", C.POINTER(C.c_uint8)), ("quals", C.POINTER(C.c_uint8)),
                ("length", C.c_int32), ("n_cigar", C.c_int32), ("cigar_type", C.c_char_p), ("cigar_num", C.POINTER(C.c_int32)),
                ("sample", C.c_int32), ("haplotype_tag", C.c_int32), ("reverse", C.c_uint8), ("use_for_hap_generation", C.c_uint8)]


class BamRecord(C.Structure):
    """struct ltr_bam_record."""

    _fields_ = [("name", C.c_char_p), ("file_index", C.c_int32), ("ref_id", C.c_int32), ("pos", C.c_int32), ("end_pos", C.c_int32),
                ("mapq", C.c_int32), ("flag", C.c_int32), ("mate_ref_id", C.c_int32), ("mate_pos", C.c_int32), ("tlen", C.c_int32),
                ("length", C.c_int32), ("bases", C.c_char_p), ("quals", C.c_char_p), ("n_cigar", C.c_int32), ("cigar_type", C.c_char_p),
                ("cigar_num", C.POINTER(C.c_int32)), ("aux", C.POINTER(C.c_uint8)), ("aux_len", C.c_int32)]


# ---- the C signatures ---------------------------------------------------------------------------------
# name -> (return type, [parameter types]) for every function include/ltr_gpu.h declares, written from the header
# (tests/test_abi_signatures.py parses the header and holds this table to it).  Scalars have the header's width and kind.
# Pointers: a struct with a mirror above is POINTER(that struct); an opaque handle (ltr_ctx*, ltr_plan*, ...) and any
# buffer of numbers is c_void_p, which takes a numpy address, byref(), a ctypes array or None alike; handle** is
# POINTER(c_void_p); char* is c_char_p, except text the library allocates (ltr_genotype_result_vcf_records ->
# ltr_vcf_text_free), which stays a c_void_p so that it is never copied into a bytes object.  A returned pointer is typed.
_P = C.POINTER
_vp, _str, _int, _sz = C.c_void_p, C.c_char_p, C.c_int, C.c_size_t
_u8, _i32, _u32, _i64, _f32, _f64 = C.c_uint8, C.c_int32, C.c_uint32, C.c_int64, C.c_float, C.c_double

SIGNATURES = {
    "ltr_default_params": (None, [_P(AlignParams)]),
    "ltr_default_stutter_params": (None, [_P(StutterParams)]),
    "ltr_ctx_set_stutter_params": (_int, [_vp, _P(StutterParams)]),
    "ltr_ctx_set_pair_packing": (_int, [_vp, _int]),
    "ltr_ctx_set_debug": (_int, [_vp, _str, _f64]),
    "ltr_ctx_wg_first_pass": (_int, [_vp, _vp, _vp]),
    "ltr_ctx_create": (_int, [_int, _P(_vp)]),
    "ltr_ctx_destroy": (None, [_vp]),
    "ltr_ctx_set_params": (_int, [_vp, _P(AlignParams)]),
    "ltr_last_error": (_str, [_vp]),
    "ltr_ctx_device_info": (_int, [_vp, _str, _int, _vp, _vp]),
    "ltr_align_batch": (_int, [_vp, _P(LocusBatch), _vp, _vp]),
    "ltr_plan_create": (_int, [_vp, _P(LocusBatch), _P(_vp)]),
    "ltr_plan_destroy": (None, [_vp]),
    "ltr_plan_num_pairs": (_i64, [_vp]),
    "ltr_plan_ll_size": (_i64, [_vp]),
    "ltr_plan_cells": (_f64, [_vp]),
    "ltr_plan_input_bytes": (_f64, [_vp]),
    "ltr_plan_execute": (_int, [_vp, _vp, _vp]),
    "ltr_plan_fetch": (_int, [_vp, _vp, _vp]),
    "ltr_plan_last_kernel_ms": (_int, [_vp, _vp, _vp]),
    "ltr_num_kernels": (_int, []),
    "ltr_kernel_lanes_per_pair": (_int, [_int]),
    "ltr_kernel_family": (_int, [_int]),
    "ltr_plan_set_timing": (_int, [_vp, _int]),
    "ltr_plan_kernel_stats": (_int, [_vp, _int, _vp, _vp, _vp, _vp]),
    "ltr_plan_kernel_ranges": (_int, [_vp, _int, _vp, _vp, _vp]),
    "ltr_plan_debug_wave_clocks": (_int, [_vp, _vp, _i64]),
    "ltr_plan_debug_entries": (_int, [_vp, _vp, _vp, _vp, _vp, _int]),
    "ltr_plan_kernel_class": (_int, [_vp]),
    "ltr_plan_family_stats": (_int, [_vp, _vp]),
    "ltr_plan_family_spine_stats": (_int, [_vp, _vp]),
    "ltr_process_reads": (_int, [_vp, _P(HaplotypeBlocks), _vp, _P(Alignment), _i32, _i32, _vp, _vp, _vp]),
    "ltr_calc_hap_aln_probs": (_int, [_vp, _P(Locus), _i64, _P(_vp), _P(_vp)]),
    "ltr_haplotype_num_combs": (_i64, [_P(HaplotypeBlocks)]),
    "ltr_haplotype_seq": (_i64, [_P(HaplotypeBlocks), _i64, _vp, _i64]),
    "ltr_trim_alignment": (_int, [_P(Alignment), _i32, _i32, _i32, _vp, _vp]),
    "ltr_pool_reads": (_i32, [_P(_vp), _vp, _i32, _vp]),
    "ltr_scatter_pool_probs": (_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ltr_posteriors": (_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ltr_plan_posteriors": (_int, [_vp, _P(PosteriorBatch), _vp, _vp, _vp]),
    "ltr_extract_genotypes": (_int, [_i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _P(GenotypeFields)]),
    "ltr_ctx_timers": (_int, [_vp, _P(Timers), _int]),
    "ltr_haps_to_alleles": (_int, [_P(HaplotypeBlocks), _i32, _vp]),
    "ltr_unused_alleles": (_i32, [_i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp]),
    "ltr_remap_haplotypes": (_int, [_P(HaplotypeBlocks), _P(HaplotypeBlocks), _vp, _vp]),
    "ltr_remap_aln_probs": (_int, [_vp, _i32, _i32, _vp, _i32, _vp]),
    "ltr_default_vcf_options": (None, [_P(VcfOptions)]),
    "ltr_get_alleles": (_i32, [_P(VcfLocus), _vp, _str, _i64, _vp]),
    "ltr_vcf_record": (_i64, [_P(VcfLocus), _P(VcfOptions), _str, _i64, _vp]),
    "ltr_vcf_header": (_i64, [_str, _str, _str, _P(VcfOptions), _P(_str), _i32, _str, _i64]),
    "ltr_haplotype_aln_info_capacity": (_i64, [_vp, _i64]),
    "ltr_haplotype_align_to_ref": (_int, [_vp, _vp, _i64, _str, _i64, _vp]),
    "ltr_left_align_reads": (_int, [_P(RawAlignment), _i32, _i32, _i32, _i32, _vp, _i64, _i64, _P(_vp)]),
    "ltr_phasing_priors": (_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "ltr_read_set_size": (_i32, [_vp]),
    "ltr_read_set_alignments": (_P(Alignment), [_vp]),
    "ltr_read_set_alignment_strings": (_P(_str), [_vp]),
    "ltr_read_set_deleted": (_P(_u8), [_vp]),
    "ltr_read_set_source": (_P(_i32), [_vp]),
    "ltr_read_set_sample": (_P(_i32), [_vp]),
    "ltr_read_set_n_p1s": (_P(_i32), [_vp]),
    "ltr_read_set_n_p2s": (_P(_i32), [_vp]),
    "ltr_read_set_fail_count": (_i32, [_vp]),
    "ltr_read_set_free": (None, [_vp]),
    "ltr_extract_sequence": (_i64, [_vp, _i32, _i32, _i32, _vp, _i64]),
    "ltr_build_haplotype": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _i64, _i32, _P(_vp)]),
    "ltr_build_vcf_haplotype": (_int, [_vp, _vp, _i32, _str, _vp, _i32, _i32, _vp, _i64, _i64, _i64, _P(_vp)]),
    "ltr_hap_result_blocks": (_P(HaplotypeBlocks), [_vp]),
    "ltr_hap_result_failure": (_str, [_vp]),
    "ltr_hap_result_unplaced_reads": (_i32, [_vp]),
    "ltr_hap_result_samples_needing_clustering": (_i32, [_vp]),
    "ltr_hap_result_free": (None, [_vp]),
    "ltr_version": (_str, []),
    "ltr_abi_version": (_int, []),
    "ltr_ctx_timers_n": (_int, [_vp, _vp, _sz, _int]),
    "ltr_ctx_short_kernel_split": (_int, [_vp, _vp, _int]),
    "ltr_ctx_set_host_threads": (_int, [_vp, _int]),
    "ltr_ctx_host_threads": (_int, [_vp]),
    "ltr_host_threads_rule": (_int, [_int]),
    "ltr_debug_parallel_threads": (_int, [_int, _i64, _int]),
    "ltr_debug_prep_ahead_rule": (_int, [_int]),
    "ltr_debug_num_classes": (_int, []),
    "ltr_debug_class_info": (_int, [_int, _vp, _vp, _vp, _vp]),
    "ltr_debug_classify": (_int, [_P(AlignParams), _int, _int, _i64, _i64, _i32, _i32, _i32, _int, _vp, _vp, _vp]),
    "ltr_debug_sort_by_class": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp]),
    "ltr_debug_pair_costs": (_int, [_P(AlignParams), _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "ltr_debug_threshold_table": (_int, [_f32, _vp, _i64]),
    "ltr_debug_calc_seed_base": (_int, [_vp, _vp]),          # (struct pointers; the test-side checker passes them as plain addresses)
    "ltr_read_regions": (_int, [_str, _u32, _str, _P(_vp), _str, _int]),
    "ltr_region_set_size": (_i64, [_vp]),
    "ltr_region_set_lines_read": (_i32, [_vp]),
    "ltr_region_set_order": (None, [_vp]),
    "ltr_region_set_free": (None, [_vp]),
    "ltr_region_chrom": (_str, [_vp, _i64]),
    "ltr_region_name": (_str, [_vp, _i64]),
    "ltr_region_motif": (_str, [_vp, _i64]),
    "ltr_region_period_str": (_str, [_vp, _i64]),
    "ltr_region_start": (_i32, [_vp, _i64]),
    "ltr_region_stop": (_i32, [_vp, _i64]),
    "ltr_region_period": (_i32, [_vp, _i64]),
    "ltr_fasta_open": (_int, [_str, _P(_vp), _str, _int]),
    "ltr_fasta_close": (None, [_vp]),
    "ltr_fasta_num_seqs": (_i64, [_vp]),
    "ltr_fasta_seq_name": (_str, [_vp, _i64]),
    "ltr_fasta_seq_len": (_i64, [_vp, _str]),
    "ltr_fasta_fetch": (_i64, [_vp, _str, _i64, _i64, _str, _i64, _str, _int]),
    "ltr_fasta_contig_lines": (_i64, [_vp, _str, _i64]),
    "ltr_vcf_writer_open": (_int, [_str, _P(_vp)]),
    "ltr_vcf_writer_header": (_int, [_vp, _str]),
    "ltr_vcf_writer_add_record": (_int, [_vp, _str, _i32, _str]),
    "ltr_vcf_writer_close": (_int, [_vp]),
    "ltr_bam_open": (_int, [_P(_str), _i32, _i32, _P(_vp), _str, _int]),
    "ltr_bam_close": (None, [_vp]),
    "ltr_bam_num_refs": (_i32, [_vp]),
    "ltr_bam_ref_name": (_str, [_vp, _i32]),
    "ltr_bam_ref_len": (_i64, [_vp, _i32]),
    "ltr_bam_num_read_groups": (_i32, [_vp]),
    "ltr_bam_read_group_id": (_str, [_vp, _i32]),
    "ltr_bam_read_group_sample": (_str, [_vp, _i32]),
    "ltr_bam_read_group_library": (_str, [_vp, _i32]),
    "ltr_bam_read_group_file": (_i32, [_vp, _i32]),
    "ltr_bam_set_region": (_int, [_vp, _str, _i32, _i32]),
    "ltr_bam_next": (_int, [_vp, _P(BamRecord)]),
    "ltr_bam_aux_int": (_int, [_P(BamRecord), _str, _vp]),
    "ltr_bam_aux_float": (_int, [_P(BamRecord), _str, _vp]),
    "ltr_bam_aux_char": (_int, [_P(BamRecord), _str, _vp]),
    "ltr_bam_aux_string": (_str, [_P(BamRecord), _str]),
    "ltr_vcf_reader_open": (_int, [_str, _P(_vp), _str, _int]),
    "ltr_vcf_reader_close": (None, [_vp]),
    "ltr_vcf_read_alleles": (_int, [_vp, _str, _i32, _i32, _vp, _str, _i64, _vp, _vp]),
    "ltr_vcf_index": (_int, [_str]),
    "ltr_debug_vcf_query": (_i64, [_vp, _str, _i64, _i64, _str, _i64]),
    "ltr_debug_tbi_parse": (_i32, [_str, _vp, _vp, _i32, _str, _i64]),
    "ltr_prune_hap_blocks": (_int, [_P(HaplotypeBlocks), _i32, _vp, _i32, _P(_vp)]),
    "ltr_plan_genotype": (_int, [_vp, _P(GenotypeBatch), _P(_vp)]),
    "ltr_genotype_result_free": (None, [_vp]),
    "ltr_genotype_result_n_loci": (_i64, [_vp]),
    "ltr_genotype_result_n_haps": (_i32, [_vp, _i64]),
    "ltr_genotype_result_new_to_old": (_P(_i32), [_vp, _i64]),
    "ltr_genotype_result_allele_mapping": (_P(_i32), [_vp, _i64]),
    "ltr_genotype_result_removed": (_i32, [_vp, _i64, _i32, _P(_P(_i32))]),
    "ltr_genotype_result_num_aff_blocks": (_i32, [_vp, _i64]),
    "ltr_genotype_result_num_aff_alleles": (_i32, [_vp, _i64]),
    "ltr_genotype_result_blocks": (_P(HaplotypeBlocks), [_vp, _i64]),
    "ltr_genotype_result_log_sample_posteriors": (_P(_f64), [_vp, _i64]),
    "ltr_genotype_result_sample_total_ll": (_P(_f64), [_vp, _i64]),
    "ltr_genotype_result_gts": (_P(_i32), [_vp, _i64]),
    "ltr_genotype_result_read_ll": (_P(_f64), [_vp, _i64]),
    "ltr_plan_genotype_fields": (_int, [_vp, _P(GenotypeBatch), _P(FieldsRequest), _P(_vp)]),
    "ltr_genotype_result_fields": (_int, [_vp, _i64, _P(LocusFields)]),
    "ltr_genotype_result_vcf_records": (_int, [_vp, _P(VcfLocus), _P(VcfOptions), _P(_vp), _vp, _vp]),
    "ltr_vcf_text_free": (None, [_vp]),
    "ltr_vcf_fields": (_int, [_P(VcfLocus), _i32, _i32, _i32, _P(_vp)]),
    "ltr_vcf_field_set_view": (_P(LocusFields), [_vp]),
    "ltr_vcf_field_set_free": (None, [_vp]),
    "ltr_vcf_record_from_fields": (_i64, [_P(VcfLocus), _P(LocusFields), _P(VcfOptions), _str, _i64, _vp]),
    "ltr_ll_genotype": (_int, [_vp, _P(LlBatch), _P(GenotypeBatch), _P(FieldsRequest), _P(_vp)]),
    "ltr_plan_posteriors_ploidy": (_int, [_vp, _P(PosteriorBatch), _vp, _vp, _vp, _vp]),
    "ltr_plan_genotype_ploidy": (_int, [_vp, _P(GenotypeBatch), _P(FieldsRequest), _vp, _P(_vp)]),
    "ltr_ll_genotype_ploidy": (_int, [_vp, _P(LlBatch), _P(GenotypeBatch), _P(FieldsRequest), _vp, _P(_vp)]),
    "ltr_genotype_result_haploid": (_i32, [_vp, _i64]),
    "ltr_edit_distances": (_int, [_vp, _P(SeqGroups), _i32, _vp, _vp]),
    "ltr_cluster_sequences": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _P(_vp)]),
    "ltr_cluster_result_threshold": (_i32, [_vp]),
    "ltr_cluster_result_n_clusters": (_i32, [_vp]),
    "ltr_cluster_result_centroids": (_P(_i32), [_vp]),
    "ltr_cluster_result_new_allele": (_P(_u8), [_vp]),
    "ltr_cluster_result_counted": (_P(_u8), [_vp]),
    "ltr_cluster_result_members": (_P(_i32), [_vp, _i32, _vp]),
    "ltr_cluster_result_free": (None, [_vp]),
    "ltr_build_haplotypes_clustered": (_int, [_vp, _P(HapBuildLocus), _i64, _i32, _P(_vp)]),
    "ltr_hap_result_inexact": (_P(_u8), [_vp]),
    "ltr_hap_result_cluster_threshold": (_i32, [_vp, _i32]),
    "ltr_poa_consensus": (_int, [_vp, _P(SeqGroups), _vp, _i64, _vp, _vp]),
    "ltr_poa_consensus_capacity": (_i64, [_P(SeqGroups)]),
    "ltr_build_haplotypes_consensus": (_int, [_vp, _P(HapBuildLocus), _i64, _i32, _P(_vp)]),
    "ltr_hap_result_consensus_rounds": (_i32, [_vp, _i32]),
    "ltr_hap_result_medoid_kept": (_i32, [_vp, _i32]),
}

# The test hooks the library exports without declaring them in the public header (csrc/ltr_plan.h, csrc/ltr_internal.h, csrc/ltr_short.h).
HOOK_SIGNATURES = {
    "ltr_debug_describe_batch": (_int, [_P(AlignParams), _int, _int, _P(LocusBatch), _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _str, _int]),
    "ltr_debug_threshold_groups": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "ltr_debug_plan_schedule": (_int, [_P(AlignParams), _int, _int, _P(LocusBatch), _vp, _vp, _vp, _vp, _int, _vp, _vp, _int, _vp, _int, _vp]),
    "ltr_debug_short_geometry": (_int, [_i32, _i32, _i32, _i32, _i32, _vp]),
    "ltr_debug_plan_families": (_int, [_P(AlignParams), _int, _int, _P(LocusBatch), _vp, _vp, _int, _vp, _vp, _int, _vp, _vp]),
    "ltr_debug_plan_family_forks": (_int, [_P(AlignParams), _int, _int, _P(LocusBatch), _vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp]),
    "ltr_debug_chunk_plan": (_int, [_i64, _f64, _vp, _int, _vp, _int, _vp]),
    "ltr_debug_last_launches": (_int, [_vp, _vp, _int, _vp]),
    "ltr_debug_family_wave_clocks": (_int, [_vp, _vp, _i64]),
}


# include/ltr_gpu_ploidy.h: the ploidy per (locus, sample).  A table of its own: SIGNATURES is held to ltr_gpu.h, declaration for
# declaration (tests/test_sample_ploidy_abi.py parses the new header and holds this table to it the same way).
PLOIDY_SIGNATURES = {
    "ltr_plan_posteriors_sample_ploidy": (_int, [_vp, _P(PosteriorBatch), _vp, _vp, _vp, _vp]),
    "ltr_plan_genotype_sample_ploidy": (_int, [_vp, _P(GenotypeBatch), _P(FieldsRequest), _vp, _P(_vp)]),
    "ltr_ll_genotype_sample_ploidy": (_int, [_vp, _P(LlBatch), _P(GenotypeBatch), _P(FieldsRequest), _vp, _P(_vp)]),
    "ltr_genotype_result_sample_haploid": (_i32, [_vp, _i64, _i32]),
}


class SnpRead(C.Structure):
    """struct ltr_snp_read (include/ltr_snp.h)."""

    _fields_ = [("pos", C.c_int32), ("end_pos", C.c_int32), ("length", C.c_int32), ("bases", C.c_char_p), ("quals", C.c_char_p),
                ("n_cigar", C.c_int32), ("cigar_type", C.c_char_p), ("cigar_num", C.POINTER(C.c_int32))]


# include/ltr_snp.h: libltr_snp.so, a host library of its own (longtr_amd/_snp.py loads it; tests/test_snp_phasing.py parses the
# header and holds this table to it).  bind() below is libltr_gpu.so's and does not walk it.
SNP_SIGNATURES = {
    "ltr_snp_set_create": (_int, [_str, _str, _i64, _vp, _vp, _i32, _i32, _P(_vp), _str, _int]),
    "ltr_snp_set_free": (None, [_vp]),
    "ltr_snp_set_n_samples": (_i32, [_vp]),
    "ltr_snp_set_sample_name": (_str, [_vp, _i32]),
    "ltr_snp_set_sample_index": (_i32, [_vp, _str]),
    "ltr_snp_set_n_valid_snps": (_i32, [_vp]),
    "ltr_snp_set_n_snps": (_i32, [_vp, _i32]),
    "ltr_snp_set_snps": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32]),
    "ltr_snp_phasing_priors": (_int, [_vp, _i32, _P(SnpRead), _i32, _vp, _vp, _vp, _str, _int]),
    "ltr_snp_debug_quality_tables": (None, [_vp, _vp]),
}


def bind(L):
    """Give every function of the loaded library its signature: the one walk over the tables."""
    for table in (SIGNATURES, PLOIDY_SIGNATURES, HOOK_SIGNATURES):
        for name, (ret, params) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ret, params
