"""Raw reads -> prepared reads -> candidate haplotypes: ReadSet, edit distances, clustering, consensus (ltr_hap_result)."""
import ctypes as C

import numpy as np

from . import _abi
from ._loader import Handle, LtrError, _p, lib


def pack_seq_groups(groups):
    """ctypes image of an ltr_seq_groups for a list of lists of bytes (+ the offsets of the U x U matrices and their total size)."""
    flat = [bytes(s) for g in groups for s in g]
    seq_off = np.zeros(len(flat) + 1, dtype=np.int64)
    seq_off[1:] = np.cumsum([len(s) for s in flat]) if flat else []
    gso = np.zeros(len(groups) + 1, dtype=np.int64)
    gso[1:] = np.cumsum([len(g) for g in groups]) if groups else []
    raw = np.frombuffer(b"".join(flat) or b"\0", dtype=np.uint8).copy()
    dist_off = np.zeros(len(groups) + 1, dtype=np.int64)
    dist_off[1:] = np.cumsum([len(g) * len(g) for g in groups]) if groups else []
    sg = _abi.SeqGroups()
    sg.n_groups, sg.n_seqs = len(groups), len(flat)
    sg.group_seq_off, sg.seq_off = gso.ctypes.data_as(C.POINTER(C.c_int64)), seq_off.ctypes.data_as(C.POINTER(C.c_int64))
    sg.seq_bytes = raw.ctypes.data_as(C.POINTER(C.c_uint8))
    return dict(sg=sg, dist_off=dist_off, keep=(raw, seq_off, gso))


def edit_distances(ctx, groups, cap, dist=None, packed=None):
    """ltr_edit_distances (ctx None: the call without a context, LTR_ERR_NO_DEVICE).  dist: optional int32 array the matrices are
    written into (left as it is on an error).  Returns the list of U x U matrices (views of one array)."""
    pk = packed or pack_seq_groups(groups)
    off = pk["dist_off"]
    if dist is None:
        dist = np.full(max(int(off[-1]), 1), -1, dtype=np.int32)
    rc = lib().ltr_edit_distances(None if ctx is None else ctx._h, C.byref(pk["sg"]), int(cap), _p(dist), _p(off))
    if rc != 0:
        raise LtrError(rc, lib().ltr_last_error(ctx._h).decode() if ctx is not None else "ltr_edit_distances")
    out = []
    for g in range(len(off) - 1):
        u = int(round((off[g + 1] - off[g]) ** 0.5))
        out.append(dist[off[g]:off[g + 1]].reshape(u, u))
    return out


def poa_consensus(ctx, groups, packed=None, with_status=False, out=None):
    """ltr_poa_consensus (ctx None: the call without a context, LTR_ERR_NO_DEVICE).  groups = list of lists of bytes; per group its
    consensus (bytes), with_status: (consensus list, status list: 1 = over the memory cap, not aligned).  out: optional dict(bytes=uint8
    array, off=int64 array, status=uint8 array) the call writes into (left as they are on an error)."""
    L = lib()
    pk = packed or pack_seq_groups(groups)
    n = pk["sg"].n_groups
    if out is None:
        cap = L.ltr_poa_consensus_capacity(C.byref(pk["sg"]))
        if cap < 0:
            raise LtrError(int(cap), "ltr_poa_consensus_capacity")
        out = dict(bytes=np.zeros(max(int(cap), 1), dtype=np.uint8), off=np.zeros(n + 1, dtype=np.int64), status=np.zeros(max(n, 1), dtype=np.uint8))
        cap = int(cap)
    else:
        cap = out.get("cap", len(out["bytes"]))
    rc = L.ltr_poa_consensus(None if ctx is None else ctx._h, C.byref(pk["sg"]), _p(out["bytes"]), cap, _p(out["off"]), _p(out["status"]))
    if rc != 0:
        raise LtrError(rc, lib().ltr_last_error(ctx._h).decode() if ctx is not None else "ltr_poa_consensus")
    raw, off = out["bytes"].tobytes(), out["off"]
    cons = [raw[off[g]:off[g + 1]] for g in range(n)]
    return (cons, [int(x) for x in out["status"][:n]]) if with_status else cons


def cluster_sequences(seqs, counts, dist, candidates=()):
    """ltr_cluster_sequences (host, no GPU): dict(threshold, clusters=[dict(centroid, members, counted, new_allele)...])."""
    L = lib()

    def pack(strings):
        raw = [bytes(s) for s in strings]
        off = np.zeros(len(raw) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in raw]) if raw else []
        return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), off
    sb, so = pack(seqs)
    cb, co = pack(candidates)
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    d = np.ascontiguousarray(dist, dtype=np.int32)
    if len(cnt) != len(seqs) or d.size != len(seqs) ** 2:
        raise LtrError(_abi.LTR_ERR_INVALID, "cluster_sequences: one count per sequence and a U x U matrix")
    h = C.c_void_p()
    rc = L.ltr_cluster_sequences(_p(sb), _p(so), _p(cnt), len(seqs), _p(d), _p(cb), _p(co), len(candidates), C.byref(h))
    if rc != 0:
        raise LtrError(rc, "ltr_cluster_sequences")
    try:
        n = L.ltr_cluster_result_n_clusters(h)
        ce, nw, ct = L.ltr_cluster_result_centroids(h), L.ltr_cluster_result_new_allele(h), L.ltr_cluster_result_counted(h)
        clusters = []
        for c in range(n):
            k = C.c_int32(0)
            m = L.ltr_cluster_result_members(h, c, C.byref(k))
            clusters.append(dict(centroid=ce[c], members=[m[i] for i in range(k.value)], counted=bool(ct[c]), new_allele=bool(nw[c])))
        return dict(threshold=L.ltr_cluster_result_threshold(h), clusters=clusters)
    finally:
        L.ltr_cluster_result_free(h)


def _hap_result(h, n_samples=None, consensus=False):
    """An ltr_hap_result as dict(blocks=[...] or None, failure, unplaced_reads, samples_needing_clustering); frees it.
    n_samples given (ltr_build_haplotypes_clustered): + inexact, cluster_threshold; consensus (ltr_build_haplotypes_consensus): +
    consensus_rounds, medoid_kept."""
    L = lib()
    out = dict(failure=L.ltr_hap_result_failure(h).decode(), unplaced_reads=L.ltr_hap_result_unplaced_reads(h),
               samples_needing_clustering=L.ltr_hap_result_samples_needing_clustering(h), blocks=None)
    bp = L.ltr_hap_result_blocks(h)
    if bp:
        out["blocks"] = _abi.blocks_from_struct(bp.contents)
    if n_samples is not None:
        ip = L.ltr_hap_result_inexact(h)
        out["inexact"] = [int(ip[i]) for i in range(len(out["blocks"][1]["alleles"]))] if (ip and out["blocks"]) else None
        out["cluster_threshold"] = [L.ltr_hap_result_cluster_threshold(h, s) for s in range(n_samples)]
        if consensus:
            out["consensus_rounds"] = [L.ltr_hap_result_consensus_rounds(h, s) for s in range(n_samples)]
            out["medoid_kept"] = [L.ltr_hap_result_medoid_kept(h, s) for s in range(n_samples)]
    L.ltr_hap_result_free(h)
    return out


class ReadSet(Handle):
    """ltr_read_set: GenotyperBamProcessor::left_align_reads for one locus.  raw: list of dict(pos, end_pos, bases,
    cigar=[(type, num)...], sample=0, hp=0, quals=None, use_for_hap_generation=True)."""

    _free = "ltr_read_set_free"

    def __init__(self, raw, n_samples, region_start, region_stop, chrom_seq, chrom_seq_start=0):
        L = lib()
        n = len(raw)
        arr = (_abi.RawAlignment * max(n, 1))()
        self._keep = []
        for i, r in enumerate(raw):
            b = np.frombuffer(r["bases"], dtype=np.uint8).copy() if len(r["bases"]) else np.zeros(1, dtype=np.uint8)
            q = None if r.get("quals") is None else np.frombuffer(r["quals"], dtype=np.uint8).copy()
            ct = bytes(ord(t) for t, _ in r["cigar"])
            cn = np.asarray([k for _, k in r["cigar"]], dtype=np.int32) if r["cigar"] else np.zeros(1, dtype=np.int32)
            self._keep.append((b, q, ct, cn))
            arr[i].pos, arr[i].end_pos = r["pos"], r["end_pos"]
            arr[i].bases = b.ctypes.data_as(C.POINTER(C.c_uint8))
            arr[i].quals = q.ctypes.data_as(C.POINTER(C.c_uint8)) if q is not None else None
            arr[i].length, arr[i].n_cigar = len(r["bases"]), len(r["cigar"])
            arr[i].cigar_type, arr[i].cigar_num = ct, cn.ctypes.data_as(C.POINTER(C.c_int32))
            arr[i].sample, arr[i].haplotype_tag = r.get("sample", 0), r.get("hp", 0)
            arr[i].reverse, arr[i].use_for_hap_generation = int(r.get("reverse", 0)), int(r.get("use_for_hap_generation", 1))
        self.chrom = np.frombuffer(chrom_seq, dtype=np.uint8).copy()
        self._h = C.c_void_p()
        rc = L.ltr_left_align_reads(arr, n, n_samples, region_start, region_stop, _p(self.chrom), chrom_seq_start, len(self.chrom), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise LtrError(rc, "ltr_left_align_reads")
        self.n_samples = n_samples
        self.size = L.ltr_read_set_size(self._h)
        self.fail_count = L.ltr_read_set_fail_count(self._h)
        self.alignments_ptr = L.ltr_read_set_alignments(self._h)
        av, st, de, so, sa = (L.ltr_read_set_alignments(self._h), L.ltr_read_set_alignment_strings(self._h), L.ltr_read_set_deleted(self._h),
                              L.ltr_read_set_source(self._h), L.ltr_read_set_sample(self._h))
        self.reads = []
        for i in range(self.size):
            a = av[i]
            self.reads.append(dict(start=a.start, stop=a.stop, seq=bytes(a.seq[:a.seq_len]),
                                   cigar=[(chr(a.cigar_type[k]), a.cigar_num[k]) for k in range(a.n_cigar)],
                                   aln=st[i], deleted=bool(de[i]), source=so[i], sample=sa[i],
                                   qual=None if not a.qual else bytes(a.qual[:a.seq_len])))
        p1, p2 = L.ltr_read_set_n_p1s(self._h), L.ltr_read_set_n_p2s(self._h)
        self.n_p1s, self.n_p2s = [p1[s] for s in range(n_samples)], [p2[s] for s in range(n_samples)]

    def extract_sequence(self, i, region_start, region_end):
        buf = np.zeros(1 << 16, dtype=np.uint8)
        n = lib().ltr_extract_sequence(self._h, i, region_start, region_end, _p(buf), len(buf))
        if n < -1:
            raise LtrError(int(n), "ltr_extract_sequence")
        return None if n < 0 else buf[:n].tobytes()

    def build_haplotype(self, region_start, region_stop, period, chrom_seq_start, chrom_len, indel_flank_len=5, ctx=None):
        """ltr_build_haplotype -> dict(blocks=[...] or None, failure, unplaced_reads, samples_needing_clustering)."""
        h = C.c_void_p()
        rc = lib().ltr_build_haplotype(None if ctx is None else ctx._h, self._h, self.n_samples, region_start, region_stop, period, _p(self.chrom),
                                   chrom_seq_start, len(self.chrom), chrom_len, indel_flank_len, C.byref(h))
        if rc != 0:
            raise LtrError(rc, "ltr_build_haplotype")
        return _hap_result(h)

    def build_vcf_haplotype(self, pos, alleles, period, chrom_seq_start, chrom_len, ctx=None):
        """ltr_build_vcf_haplotype (add_vcf_haplotype_block + fuse_haplotype_blocks) for panel alleles (REF first, as
        VcfPanel.alleles gives them) at 0-based pos -> the dict of build_haplotype."""
        raw = [a.encode() if isinstance(a, str) else bytes(a) for a in alleles]
        off = np.zeros(len(raw) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(a) for a in raw]) if raw else []
        h = C.c_void_p()
        rc = lib().ltr_build_vcf_haplotype(None if ctx is None else ctx._h, self._h, int(pos), b"".join(raw), _p(off), len(raw), int(period),
                                       _p(self.chrom), chrom_seq_start, len(self.chrom), chrom_len, C.byref(h))
        if rc != 0:
            raise LtrError(rc, "ltr_build_vcf_haplotype")
        return _hap_result(h)
