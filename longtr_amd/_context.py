"""Context: one ltr_ctx per GPU, and the calls that take it."""
import ctypes as C

import numpy as np

from . import _abi
from ._genotype import GenotypeResult, Plan, _locus_haploid, _sample_haploid
from ._haplotypes import _hap_result, edit_distances, poa_consensus
from ._loader import Handle, LtrError, _p, lib


class Context(Handle):
    """ltr_ctx: one per GPU (pass LOCAL_RANK)."""

    _free = "ltr_ctx_destroy"

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        rc = lib().ltr_ctx_create(int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise LtrError(rc, "ltr_ctx_create failed (no HIP device? the alignment path has no CPU fallback)")
        self.params = _abi.default_params()
        if params is not None:
            self.set_params(params)

    def _check(self, rc):
        if rc != 0:
            raise LtrError(rc, lib().ltr_last_error(self._h).decode())

    def set_params(self, params):
        self._check(lib().ltr_ctx_set_params(self._h, C.byref(params)))
        self.params = params

    def set_pair_packing(self, mode):
        """-1: two pairs per wavefront when the batch is large (default); 0 never; 1 whenever the read fits."""
        self._check(lib().ltr_ctx_set_pair_packing(self._h, int(mode)))

    def set_debug(self, key, value):
        """ltr_ctx_set_debug: measurement switches (fan_lanes, fan_pairs, chunks, chunk_streams, chunk_growth, trace)."""
        self._check(lib().ltr_ctx_set_debug(self._h, key.encode(), float(value)))

    def set_host_threads(self, n):
        """ltr_ctx_set_host_threads: the process's host-thread budget (0 = the rule: affinity mask, cgroup quota, LOCAL_WORLD_SIZE)."""
        self._check(lib().ltr_ctx_set_host_threads(self._h, int(n)))

    def host_threads(self):
        return int(lib().ltr_ctx_host_threads(self._h))

    def short_kernel_split(self, reset=True):
        """ltr_ctx_short_kernel_split: device ms of the seeded path's launches (needs set_debug("short_split", 1))."""
        out = (C.c_double * 4)()
        self._check(lib().ltr_ctx_short_kernel_split(self._h, out, int(reset)))
        return list(out)

    def wg_first_pass(self):
        """ltr_ctx_wg_first_pass: (mode, pairs the last read execute's first pass could not finish, pairs it scored)."""
        a, b = C.c_int64(0), C.c_int64(0)
        rc = lib().ltr_ctx_wg_first_pass(self._h, C.byref(a), C.byref(b))
        if rc < 0:
            self._check(rc)
        return rc, a.value, b.value

    def set_stutter_params(self, sp):
        self._check(lib().ltr_ctx_set_stutter_params(self._h, C.byref(sp)))

    def device_info(self):
        buf = C.create_string_buffer(64)
        ncu, mhz = C.c_int(0), C.c_int(0)
        self._check(lib().ltr_ctx_device_info(self._h, buf, 64, C.byref(ncu), C.byref(mhz)))
        return dict(arch=buf.value.decode(), n_cu=ncu.value, clock_mhz=mhz.value)

    def align_batch(self, batch, out_ll=None):
        """ltr_align_batch: host in, host out.  Returns (ll, seed)."""
        ll = np.full(max(batch.ll_size, 1), np.nan, dtype=np.float64) if out_ll is None else out_ll
        seed = np.full(max(batch.n_reads, 1), -1, dtype=np.int32)
        self._check(lib().ltr_align_batch(self._h, C.byref(batch.struct), _p(ll), _p(seed)))
        return ll[:batch.ll_size], seed[:batch.n_reads]

    def plan(self, batch):
        return Plan(self, batch)

    def process_reads(self, blocks, alns, realign_hap=None, realign_read=None, init_read_index=0):
        """HapAligner::process_reads for one locus (raw alignments + haplotype blocks)."""
        ph = _abi.PackedHaplotype(blocks)
        pa = _abi.PackedAlignments(alns)
        H = ph.num_combs
        probs = np.full((init_read_index + len(alns)) * H, np.nan, dtype=np.float64)
        seeds = np.full(init_read_index + len(alns), -12345, dtype=np.int32)
        rh = None if realign_hap is None else np.ascontiguousarray(realign_hap, dtype=np.uint8)
        rr = None if realign_read is None else np.ascontiguousarray(realign_read, dtype=np.uint8)
        self._check(lib().ltr_process_reads(self._h, C.byref(ph.struct), _p(rh), pa.array, len(alns),
                                            init_read_index, _p(rr), _p(probs), _p(seeds)))
        return probs.reshape(-1, H), seeds

    def pack_haplotypes(self, loci_blocks):
        """ctypes image of the haplotypes of many loci for haplotype_align_to_ref_packed (+ the output buffers)."""
        phs = [_abi.PackedHaplotype(b) for b in loci_blocks]
        arr = (C.POINTER(_abi.HaplotypeBlocks) * max(len(phs), 1))(*[C.pointer(p.struct) for p in phs])
        cap = lib().ltr_haplotype_aln_info_capacity(arr, len(phs))
        if cap < 0:
            raise LtrError(int(cap), "ltr_haplotype_aln_info_capacity")
        nh = sum(p.num_combs for p in phs)
        return dict(phs=phs, arr=arr, n=len(phs), cap=int(cap), buf=C.create_string_buffer(max(int(cap), 1)),
                    off=np.zeros(nh + 1, dtype=np.int64))

    def haplotype_align_to_ref_packed(self, packed, decode=True):
        self._check(lib().ltr_haplotype_align_to_ref(self._h, packed["arr"], packed["n"], packed["buf"], packed["cap"], _p(packed["off"])))
        if not decode:
            return None
        raw, off, out, h = packed["buf"].raw, packed["off"], [], 0
        for p in packed["phs"]:
            out.append([raw[off[h + k]:off[h + k + 1]].decode() for k in range(p.num_combs)])
            h += p.num_combs
        return out

    def haplotype_align_to_ref(self, loci_blocks):
        """ltr_haplotype_align_to_ref: per locus the list of hap_aln_info_ strings (Haplotype::next() order)."""
        return self.haplotype_align_to_ref_packed(self.pack_haplotypes(loci_blocks))

    def timers(self, reset=False):
        """ltr_ctx_timers: the reference's hap-build / hap-align / posterior clocks (+ DP kernel device time)."""
        t = _abi.Timers()
        self._check(lib().ltr_ctx_timers(self._h, C.byref(t), int(bool(reset))))
        return {f: getattr(t, f) for f, _ in _abi.Timers._fields_}

    @staticmethod
    def pack_loci(loci, out_init=None, contiguous=False):
        """ctypes image of a list of (blocks, alns[, second_mate[, masks]]) for ltr_calc_hap_aln_probs;
        masks = dict(realign_to_hap=, realign_pool=, copy_read=) (each optional).  out_init: optional list of
        [R x H] arrays the output matrices start from (cells a mask leaves untouched keep these values).
        contiguous: the per-locus matrices are slices of ONE array ("flat", offsets "flat_off"): what a rank hands to the gather."""
        keep, arr = [], (_abi.Locus * max(len(loci), 1))()
        outs = []
        flat = flat_off = None
        if contiguous:
            sizes = [len(item[1]) * _abi.PackedHaplotype(item[0]).num_combs for item in loci]
            flat_off = np.zeros(len(loci) + 1, dtype=np.int64)
            flat_off[1:] = np.cumsum(sizes)
            flat = np.full(max(int(flat_off[-1]), 1), np.nan, dtype=np.float64)
        pp = (C.c_void_p * max(len(loci), 1))()
        sp = (C.c_void_p * max(len(loci), 1))()
        for i, item in enumerate(loci):
            blocks, alns = item[0], item[1]
            sm = item[2] if len(item) > 2 else None
            masks = item[3] if len(item) > 3 and item[3] else {}
            ph, pa = _abi.PackedHaplotype(blocks), _abi.PackedAlignments(alns)
            u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
            u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None
            smv = u8(sm)
            mk = [u8(masks.get(k)) for k in ("realign_to_hap", "realign_pool", "copy_read")]
            probs = np.full(len(alns) * ph.num_combs, np.nan, dtype=np.float64) if flat is None else flat[flat_off[i]:flat_off[i + 1]]
            if out_init is not None:
                probs[:] = np.asarray(out_init[i], dtype=np.float64).ravel()
            seeds = np.full(max(len(alns), 1), -12345, dtype=np.int32)
            keep.append((ph, pa, smv, mk))
            arr[i].hap = C.pointer(ph.struct)
            arr[i].alns = pa.array
            arr[i].n_alns = len(alns)
            arr[i].second_mate = u8p(smv)
            arr[i].realign_to_hap, arr[i].realign_pool, arr[i].copy_read = u8p(mk[0]), u8p(mk[1]), u8p(mk[2])
            pp[i] = probs.ctypes.data
            sp[i] = seeds.ctypes.data
            outs.append((probs.reshape(len(alns), ph.num_combs), seeds[:len(alns)]))
        return dict(n=len(loci), arr=arr, pp=pp, sp=sp, outs=outs, keep=keep, flat=flat, flat_off=flat_off)

    def calc_hap_aln_probs_packed(self, packed):
        self._check(lib().ltr_calc_hap_aln_probs(self._h, packed["arr"], packed["n"], packed["pp"], packed["sp"]))
        return packed["outs"]

    def calc_hap_aln_probs(self, loci):
        """ltr_calc_hap_aln_probs.  loci: list of (blocks, alns[, second_mate]).  Returns per locus
        (log_aln_probs [R x H], seed_positions [R])."""
        return self.calc_hap_aln_probs_packed(self.pack_loci(loci))

    def posteriors(self, ll, log_p1, log_p2, sample_label, n_samples, haploid=False):
        ll = np.array(ll, dtype=np.float64, copy=True)
        R, H = ll.shape
        p1 = np.ascontiguousarray(log_p1, dtype=np.float64)
        p2 = np.ascontiguousarray(log_p2, dtype=np.float64)
        sl = np.ascontiguousarray(sample_label, dtype=np.int32)
        post = np.zeros(n_samples * H * H, dtype=np.float64)
        stl = np.zeros(n_samples, dtype=np.float64)
        gts = np.zeros(2 * n_samples, dtype=np.int32)
        tot = C.c_double(0.0)
        self._check(lib().ltr_posteriors(self._h, n_samples, R, H, _p(ll), _p(p1), _p(p2), _p(sl), int(haploid),
                                         _p(post), _p(stl), _p(gts), C.byref(tot)))
        return dict(post=post.reshape(n_samples, H, H), sample_total_ll=stl, gts=gts.reshape(n_samples, 2),
                    total_ll=tot.value, clamped_ll=ll)

    def pack_ll_genotype(self, ll_list, seed_list, loci_blocks, locus_read_off, log_p1, log_p2, sample_label, n_samples, haploid=False,
                         prune=True, want_read_ll=False, sample_filtered=None):
        """ctypes image of the ltr_ll_batch + ltr_genotype_batch of genotype_ll (for repeated calls).  ll_list: per locus the
        [R_l x H_l] matrix (float64, C order: used where it lies, never written) or None for a locus without reads; seed_list:
        None, or per locus the [R_l] seed positions or None (= every read aligned); loci_blocks: per locus the block list, or
        None altogether (prune=False without fields)."""
        n = len(n_samples)
        lro = np.ascontiguousarray(locus_read_off, dtype=np.int64)
        keep = [lro, None, np.ascontiguousarray(log_p1, dtype=np.float64), np.ascontiguousarray(log_p2, dtype=np.float64),
                np.ascontiguousarray(sample_label, dtype=np.int32), np.ascontiguousarray(n_samples, dtype=np.int32)]
        pb = _abi.PosteriorBatch()
        pb.n_loci, pb.n_reads, pb.haploid = n, len(keep[4]), int(haploid)
        pb.locus_read_off = lro.ctypes.data_as(C.POINTER(C.c_int64))
        pb.log_p1, pb.log_p2 = keep[2].ctypes.data_as(C.POINTER(C.c_double)), keep[3].ctypes.data_as(C.POINTER(C.c_double))
        pb.sample_label, pb.n_samples = keep[4].ctypes.data_as(C.POINTER(C.c_int32)), keep[5].ctypes.data_as(C.POINTER(C.c_int32))
        if len(ll_list) != n or (seed_list is not None and len(seed_list) != n) or (loci_blocks is not None and len(loci_blocks) != n):
            raise LtrError(_abi.LTR_ERR_INVALID, "genotype_ll: one matrix / seed array / block list per locus")
        mats = [None if m is None else np.ascontiguousarray(m, dtype=np.float64) for m in ll_list]
        for l, m in enumerate(mats):
            if m is not None and (m.ndim != 2 or m.shape[0] != lro[l + 1] - lro[l]):
                raise LtrError(_abi.LTR_ERR_INVALID, f"genotype_ll: matrix of locus {l} is not [reads x haplotypes]")
        if loci_blocks is not None:
            n_haps = np.asarray([int(np.prod([len(b["alleles"]) for b in bl], dtype=np.int64)) if m is None else m.shape[1]
                                 for m, bl in zip(mats, loci_blocks)], dtype=np.int32)
        else:
            n_haps = np.asarray([1 if m is None else m.shape[1] for m in mats], dtype=np.int32)
        seeds = None if seed_list is None else [None if s is None else np.ascontiguousarray(s, dtype=np.int32) for s in seed_list]
        lb = _abi.LlBatch()
        mp = (C.POINTER(C.c_double) * max(n, 1))(*[None if m is None else m.ctypes.data_as(C.POINTER(C.c_double)) for m in mats])
        sp = None if seeds is None else (C.POINTER(C.c_int32) * max(n, 1))(*[None if s is None else s.ctypes.data_as(C.POINTER(C.c_int32)) for s in seeds])
        lb.log_aln_probs, lb.seed_positions, lb.n_haps = mp, sp, n_haps.ctypes.data_as(C.POINTER(C.c_int32))
        phs = [] if loci_blocks is None else [_abi.PackedHaplotype(b) for b in loci_blocks]
        arr = None if loci_blocks is None else (C.POINTER(_abi.HaplotypeBlocks) * max(n, 1))(*[C.pointer(p.struct) for p in phs])
        sf = None if sample_filtered is None else np.ascontiguousarray(sample_filtered, dtype=np.uint8)
        gb = _abi.GenotypeBatch()
        gb.pb, gb.haps = C.pointer(pb), arr
        gb.sample_filtered = sf.ctypes.data_as(C.POINTER(C.c_uint8)) if sf is not None else None
        gb.prune, gb.want_read_ll = int(bool(prune)), int(bool(want_read_ll))
        return dict(gb=gb, lb=lb, keep=(pb, keep, mats, seeds, n_haps, mp, sp, phs, arr, sf), n_samples=keep[5], locus_read_off=lro,
                    loci_blocks=loci_blocks if loci_blocks is not None else [[dict(alleles=[b""] * int(h))] for h in n_haps])

    def genotype_ll(self, ll_list=None, seed_list=None, loci_blocks=None, locus_read_off=None, log_p1=None, log_p2=None, sample_label=None,
                    n_samples=None, haploid=False, prune=True, want_read_ll=False, fields=None, sample_filtered=None, packed=None, locus_haploid=None,
                    sample_haploid=None):
        """ltr_ll_genotype: what Plan.genotype / Plan.genotype_fields do for a resident plan, on per-read matrices in host
        memory -- the output of calc_hap_aln_probs (any path: plans, the seeded stutter path, mates summed, realign masks).
        fields: None = no VCF fields (as Plan.genotype; posterior blocks are downloaded), or a dict with any of block,
        want_gls, want_pls, want_phased_gls, want_posteriors (as Plan.genotype_fields).  packed: a pack_ll_genotype image.
        locus_haploid: the ploidy of every locus (ltr_ll_genotype_ploidy; `haploid` is then not read), None = `haploid` for all.
        sample_haploid: the ploidy of every (locus, sample), one array of S flags per locus (ltr_ll_genotype_sample_ploidy); not with locus_haploid.
        Returns a GenotypeResult (close() it, or use it as a context manager)."""
        if packed is None:
            packed = self.pack_ll_genotype(ll_list, seed_list, loci_blocks, locus_read_off, log_p1, log_p2, sample_label, n_samples, haploid,
                                           prune, want_read_ll, sample_filtered)
        L = lib()
        fr, blk = None, None
        if fields is not None:
            fr = _abi.FieldsRequest()
            if fields.get("block") is not None:
                blk = np.ascontiguousarray(fields["block"], dtype=np.int32)
                if len(blk) != len(packed["n_samples"]):
                    raise LtrError(_abi.LTR_ERR_INVALID, "genotype_ll: one block index per locus")
                fr.block = blk.ctypes.data_as(C.POINTER(C.c_int32))
            for k in ("want_gls", "want_pls", "want_phased_gls", "want_posteriors"):
                setattr(fr, k, int(bool(fields.get(k, False))))
        h = C.c_void_p()
        pfr = None if fr is None else C.byref(fr)
        if sample_haploid is not None:
            sh = _sample_haploid(sample_haploid, packed["n_samples"], locus_haploid)
            self._check(L.ltr_ll_genotype_sample_ploidy(self._h, C.byref(packed["lb"]), C.byref(packed["gb"]), pfr, _p(sh), C.byref(h)))
        elif locus_haploid is None:
            self._check(L.ltr_ll_genotype(self._h, C.byref(packed["lb"]), C.byref(packed["gb"]), pfr, C.byref(h)))
        else:
            lh = _locus_haploid(locus_haploid, len(packed["n_samples"]))
            self._check(L.ltr_ll_genotype_ploidy(self._h, C.byref(packed["lb"]), C.byref(packed["gb"]), pfr, _p(lh), C.byref(h)))
        return GenotypeResult(self, h, packed, per_sample=sample_haploid is not None)

    def edit_distances(self, groups, cap):
        """ltr_edit_distances: groups = list of lists of bytes; per group the U x U int32 matrix min(levenshtein, cap)."""
        return edit_distances(self, groups, cap)

    def poa_consensus(self, groups, with_status=False):
        """ltr_poa_consensus: groups = list of lists of bytes; per group its partial-order-alignment consensus."""
        return poa_consensus(self, groups, with_status=with_status)

    def build_haplotypes_clustered(self, loci, indel_flank_len=5):
        """ltr_build_haplotypes_clustered.  loci: list of dict(rs=ReadSet, region_start, region_stop, period, chrom_seq_start, chrom_len).
        Per locus the dict of ReadSet.build_haplotype + inexact (per allele of the repeat block, None for a failed construction)
        + cluster_threshold (per sample: accepted T, -1 none, 0 not needed)."""
        return self._build_haplotypes(loci, indel_flank_len, consensus=False)

    def build_haplotypes_consensus(self, loci, indel_flank_len=5):
        """ltr_build_haplotypes_consensus: build_haplotypes_clustered with the partial-order-alignment consensus of a cluster as its
        centre (ltr_poa_consensus).  Per locus the same dict + consensus_rounds and medoid_kept (per sample)."""
        return self._build_haplotypes(loci, indel_flank_len, consensus=True)

    def _build_haplotypes(self, loci, indel_flank_len, consensus):
        L = lib()
        fn = L.ltr_build_haplotypes_consensus if consensus else L.ltr_build_haplotypes_clustered
        arr = (_abi.HapBuildLocus * max(len(loci), 1))()
        for i, l in enumerate(loci):
            rs = l["rs"]
            arr[i].rs, arr[i].n_samples, arr[i].region_start, arr[i].region_stop, arr[i].period = rs._h, rs.n_samples, l["region_start"], l["region_stop"], l["period"]
            arr[i].chrom_seq = rs.chrom.ctypes.data_as(C.POINTER(C.c_uint8))
            arr[i].chrom_seq_start, arr[i].chrom_seq_len, arr[i].chrom_len = l["chrom_seq_start"], len(rs.chrom), l["chrom_len"]
        out = (C.c_void_p * max(len(loci), 1))()
        self._check(fn(self._h, arr, len(loci), int(indel_flank_len), out))
        return [_hap_result(C.c_void_p(out[i]), n_samples=l["rs"].n_samples, consensus=consensus) for i, l in enumerate(loci)]
