"""Plan (one packed batch resident in HBM), GenotypeResult, and the VCF record of a genotyped locus."""
import ctypes as C

import numpy as np

from . import _abi
from ._loader import Handle, LtrError, _p, lib, text_call

FAMILIES = {0: "one-wave", 1: "packed", 2: "workgroup", 3: "exact"}      # ltr_kernel_family()


class Plan(Handle):
    """ltr_plan: one packed batch resident in HBM."""

    _free = "ltr_plan_destroy"

    def __init__(self, ctx, batch):
        self.ctx = ctx
        self.batch = batch
        self._h = C.c_void_p()
        ctx._check(lib().ltr_plan_create(ctx._h, C.byref(batch.struct), C.byref(self._h)))
        self.num_pairs = lib().ltr_plan_num_pairs(self._h)
        self.ll_size = lib().ltr_plan_ll_size(self._h)
        self.cells = lib().ltr_plan_cells(self._h)
        self.input_bytes = lib().ltr_plan_input_bytes(self._h)

    def execute(self, d_out_ptr=None, stream=None):
        self.ctx._check(lib().ltr_plan_execute(self._h, d_out_ptr, stream))

    def fetch(self):
        ll = np.full(max(self.ll_size, 1), np.nan, dtype=np.float64)
        seed = np.full(max(self.batch.n_reads, 1), -1, dtype=np.int32)
        self.ctx._check(lib().ltr_plan_fetch(self._h, _p(ll), _p(seed)))
        return ll[:self.ll_size], seed[:self.batch.n_reads]

    def wait(self):
        self.ctx._check(lib().ltr_plan_fetch(self._h, None, None))

    def last_kernel_ms(self):
        ms, n = C.c_float(0), C.c_int(0)
        self.ctx._check(lib().ltr_plan_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def posteriors(self, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid=False, locus_haploid=None, sample_haploid=None):
        """ltr_plan_posteriors: all loci, from the device-resident LL of the last execute.
        locus_haploid: the ploidy of every locus (ltr_plan_posteriors_ploidy; `haploid` is then not read), None = `haploid` for all.
        sample_haploid: the ploidy of every (locus, sample), one array of S flags per locus (ltr_plan_posteriors_sample_ploidy); not with locus_haploid.
        Returns (post_flat, post_off[units+1], sample_total_ll, gts[units,2]); units = (locus, sample) in order."""
        pb, keep = self._posterior_batch(locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid)
        ns = keep[5]
        H = np.diff(self.batch.locus_hap_off)
        sizes = np.repeat(H * H, ns)
        off = np.zeros(len(sizes) + 1, dtype=np.int64)
        off[1:] = np.cumsum(sizes)
        post = np.zeros(max(int(off[-1]), 1), dtype=np.float64)
        stl = np.zeros(max(len(sizes), 1), dtype=np.float64)
        gts = np.zeros(2 * max(len(sizes), 1), dtype=np.int32)
        if sample_haploid is not None:
            sh = _sample_haploid(sample_haploid, ns, locus_haploid)
            self.ctx._check(lib().ltr_plan_posteriors_sample_ploidy(self._h, C.byref(pb), _p(sh), _p(post), _p(stl), _p(gts)))
        elif locus_haploid is None:
            self.ctx._check(lib().ltr_plan_posteriors(self._h, C.byref(pb), _p(post), _p(stl), _p(gts)))
        else:
            lh = _locus_haploid(locus_haploid, len(ns))
            self.ctx._check(lib().ltr_plan_posteriors_ploidy(self._h, C.byref(pb), _p(lh), _p(post), _p(stl), _p(gts)))
        return post[:off[-1]], off, stl[:len(sizes)], gts[:2 * len(sizes)].reshape(-1, 2)

    def _posterior_batch(self, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid):
        keep = [np.ascontiguousarray(locus_read_off, dtype=np.int64), np.ascontiguousarray(pool_index, dtype=np.int32),
                np.ascontiguousarray(log_p1, dtype=np.float64), np.ascontiguousarray(log_p2, dtype=np.float64),
                np.ascontiguousarray(sample_label, dtype=np.int32), np.ascontiguousarray(n_samples, dtype=np.int32)]
        pb = _abi.PosteriorBatch()
        pb.n_loci = len(keep[5])
        pb.locus_read_off = keep[0].ctypes.data_as(C.POINTER(C.c_int64))
        pb.n_reads = len(keep[1])
        pb.pool_index = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
        pb.log_p1 = keep[2].ctypes.data_as(C.POINTER(C.c_double))
        pb.log_p2 = keep[3].ctypes.data_as(C.POINTER(C.c_double))
        pb.sample_label = keep[4].ctypes.data_as(C.POINTER(C.c_int32))
        pb.n_samples = keep[5].ctypes.data_as(C.POINTER(C.c_int32))
        pb.haploid = int(haploid)
        return pb, keep

    def pack_genotype(self, loci_blocks, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid=False,
                      sample_filtered=None, prune=True, want_read_ll=True):
        """ctypes image of an ltr_genotype_batch (for repeated genotype_packed calls).  loci_blocks: the block list of every
        locus; the other arrays as Plan.posteriors takes them; sample_filtered: optional flat [sum S_l] (call_sample_ not empty)."""
        pb, keep = self._posterior_batch(locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid)
        phs = [_abi.PackedHaplotype(b) for b in loci_blocks]
        arr = (C.POINTER(_abi.HaplotypeBlocks) * max(len(phs), 1))(*[C.pointer(p.struct) for p in phs])
        sf = None if sample_filtered is None else np.ascontiguousarray(sample_filtered, dtype=np.uint8)
        gb = _abi.GenotypeBatch()
        gb.pb = C.pointer(pb)
        gb.haps = arr
        gb.sample_filtered = sf.ctypes.data_as(C.POINTER(C.c_uint8)) if sf is not None else None
        gb.prune, gb.want_read_ll = int(bool(prune)), int(bool(want_read_ll))
        return dict(gb=gb, keep=(pb, keep, phs, arr, sf), n_samples=keep[5], locus_read_off=keep[0], loci_blocks=loci_blocks)

    def genotype_packed(self, packed, decode=True, locus_haploid=None, sample_haploid=None):
        """ltr_plan_genotype on a pack_genotype image.  decode=False: run, free the result, return None (timing).
        locus_haploid: the ploidy of every locus (ltr_plan_genotype_ploidy), None = the image's `haploid` for all.
        sample_haploid: one array of S flags per locus (ltr_plan_genotype_sample_ploidy); not with locus_haploid."""
        L = lib()
        h = C.c_void_p()
        if sample_haploid is not None:
            sh = _sample_haploid(sample_haploid, packed["n_samples"], locus_haploid)
            self.ctx._check(L.ltr_plan_genotype_sample_ploidy(self._h, C.byref(packed["gb"]), None, _p(sh), C.byref(h)))
        elif locus_haploid is None:
            self.ctx._check(L.ltr_plan_genotype(self._h, C.byref(packed["gb"]), C.byref(h)))
        else:
            lh = _locus_haploid(locus_haploid, len(packed["n_samples"]))
            self.ctx._check(L.ltr_plan_genotype_ploidy(self._h, C.byref(packed["gb"]), None, _p(lh), C.byref(h)))
        with GenotypeResult(self.ctx, h, packed, per_sample=sample_haploid is not None) as res:
            if not decode:
                return None
            out = [dict(res.locus(l), haploid=res.haploid(l)) for l in range(res.n_loci)]     # (locus() carries "sample_haploid")
            for d, S in zip(out, packed["n_samples"]):
                if d["post"] is None:                            # (always downloaded here: None is the empty block of a locus without samples)
                    d["post"] = np.zeros((int(S), d["n_haps"], d["n_haps"]))
            return out

    def genotype(self, loci_blocks, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid=False,
                 sample_filtered=None, prune=True, want_read_ll=True, locus_haploid=None, sample_haploid=None):
        """ltr_plan_genotype: SeqStutterGenotyper::genotype after the alignment for every locus of the executed plan --
        posteriors, uncalled alleles pruned once (prune=True), posteriors again over the surviving haplotypes.  Returns per
        locus a dict: n_haps, new_to_old, allele_mapping, removed (per block), num_aff_blocks / num_aff_alleles, blocks (the
        final block list), post [S, H', H'], sample_total_ll [S], gts [S, 2] (new indices), read_ll [R, H'] or None, haploid (0 / 1).
        locus_haploid: the ploidy of every locus (a whole-genome plan with --haploid-chrs), None = `haploid` for all.
        sample_haploid: the ploidy of every (locus, sample), one array of S flags per locus (chrX of a mixed cohort); not with locus_haploid."""
        return self.genotype_packed(self.pack_genotype(loci_blocks, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples,
                                                       haploid, sample_filtered, prune, want_read_ll), locus_haploid=locus_haploid,
                                    sample_haploid=sample_haploid)

    def genotype_fields(self, loci_blocks=None, locus_read_off=None, pool_index=None, log_p1=None, log_p2=None, sample_label=None,
                        n_samples=None, haploid=False, sample_filtered=None, prune=True, want_read_ll=False, block=None,
                        want_gls=False, want_pls=False, want_phased_gls=False, want_posteriors=False, packed=None, locus_haploid=None,
                        sample_haploid=None):
        """ltr_plan_genotype_fields: ltr_plan_genotype and the VCF fields of every locus computed on the device (GT, Q, PQ,
        GLDIFF, DP, DSNP, PSNP, MALLREADS' alleles; GL / PL / PHASEDGL on request).  block: per locus, None = the first repeat
        block.  Posterior blocks / per-read matrices are downloaded only when asked for.  packed: a pack_genotype image (its
        want_read_ll holds).  locus_haploid: the ploidy of every locus (ltr_plan_genotype_ploidy), None = `haploid` for all.
        sample_haploid: one array of S flags per locus (ltr_plan_genotype_sample_ploidy); not with locus_haploid.
        Returns a GenotypeResult (close() it, or use it as a context manager)."""
        if packed is None:
            packed = self.pack_genotype(loci_blocks, locus_read_off, pool_index, log_p1, log_p2, sample_label, n_samples, haploid,
                                        sample_filtered, prune, want_read_ll)
        L = lib()
        fr = _abi.FieldsRequest()
        blk = None if block is None else np.ascontiguousarray(block, dtype=np.int32)
        if blk is not None:
            if len(blk) != len(packed["n_samples"]):
                raise LtrError(-1, "genotype_fields: one block index per locus")
            fr.block = blk.ctypes.data_as(C.POINTER(C.c_int32))
        fr.want_gls, fr.want_pls, fr.want_phased_gls = int(bool(want_gls)), int(bool(want_pls)), int(bool(want_phased_gls))
        fr.want_posteriors = int(bool(want_posteriors))
        h = C.c_void_p()
        if sample_haploid is not None:
            sh = _sample_haploid(sample_haploid, packed["n_samples"], locus_haploid)
            self.ctx._check(L.ltr_plan_genotype_sample_ploidy(self._h, C.byref(packed["gb"]), C.byref(fr), _p(sh), C.byref(h)))
        elif locus_haploid is None:
            self.ctx._check(L.ltr_plan_genotype_fields(self._h, C.byref(packed["gb"]), C.byref(fr), C.byref(h)))
        else:
            lh = _locus_haploid(locus_haploid, len(packed["n_samples"]))
            self.ctx._check(L.ltr_plan_genotype_ploidy(self._h, C.byref(packed["gb"]), C.byref(fr), _p(lh), C.byref(h)))
        return GenotypeResult(self.ctx, h, packed, per_sample=sample_haploid is not None)

    def set_timing(self, on=True):
        """on: False / True (every launch as it is launched) / 2 (the multi-width one-wave launch class by class)."""
        self.ctx._check(lib().ltr_plan_set_timing(self._h, int(on)))

    def wave_clocks(self):
        """(n_waves, 4) uint64: first / last wall clock (100 MHz), pairs scored with the exact body, ticks spent there -- per
        wavefront of the plan kernel (debug knob wave_clock)."""
        buf = np.zeros(4 * 4 * 4096 + 4096 + 256, dtype=np.uint64)
        n = lib().ltr_plan_debug_wave_clocks(self._h, _p(buf), buf.size)
        if n < 0:
            raise LtrError(n, "ltr_plan_debug_wave_clocks")
        k = int(min(buf[4 * n], 4095))
        self.redo_log = [(int(v >> np.uint64(32)), int(v & np.uint64(0xffffffff))) for v in buf[4 * n + 1:4 * n + 1 + k]]   # (n, m) of the pairs that took the exact body
        self.entry_ticks = buf[4 * n + 4096:4 * n + 4096 + 256].copy()       # per entry of the plan kernel's table: ticks of all wavefronts together
        return buf[:4 * n].reshape(n, 4)

    def family_wave_clocks(self):
        """(n_waves, 2) uint64: first / last wall clock (100 MHz) per wavefront of the family launch of the last execute (debug knob
        wave_clock; the same clock as wave_clocks()).  Empty when nothing was recorded: the knob off, or a plan without families."""
        buf = np.zeros(2 * 4 * 4096, dtype=np.uint64)
        n = lib().ltr_debug_family_wave_clocks(self._h, _p(buf), buf.size)
        if n < 0:
            raise LtrError(n, "ltr_debug_family_wave_clocks")
        return buf[:2 * n].reshape(n, 2)

    def family_spine_stats(self):
        """ltr_plan_family_spine_stats: dict(with_spine: families of the plan run along a spine, steps_saved: modelled wavefront
        steps that saves against plain families)."""
        out = np.zeros(2, dtype=np.int64)
        self.ctx._check(lib().ltr_plan_family_spine_stats(self._h, _p(out)))
        return dict(with_spine=int(out[0]), steps_saved=int(out[1]))

    def family_stats(self):
        """ltr_plan_family_stats: dict(families, members) of the plan and, of its last execute, stem_failures (families whose stem
        certificate failed: every member to the exact body), rule_failures / tail_failures (members the acceptance rule / a tail
        certificate sent there)."""
        out = np.zeros(5, dtype=np.int64)
        self.ctx._check(lib().ltr_plan_family_stats(self._h, _p(out)))
        return dict(zip(("families", "members", "stem_failures", "rule_failures", "tail_failures"), (int(v) for v in out)))

    def plan_entries(self):
        """The plan kernel's table in walk order: dicts (kind, strip_width, pairs, cells)."""
        kind, w, npairs, cells = np.zeros(256, np.int32), np.zeros(256, np.int32), np.zeros(256, np.int64), np.zeros(256, np.float64)
        n = lib().ltr_plan_debug_entries(self._h, _p(kind), _p(w), _p(npairs), _p(cells), 256)
        if n < 0:
            raise LtrError(n, "ltr_plan_debug_entries")
        names = {0: "one-wave", 1: "packed", 2: "exact body", 3: "one-wave (chained)"}
        return [dict(kind=names.get(int(kind[i]), "?"), strip_width=int(w[i]), pairs=int(npairs[i]), cells=float(cells[i])) for i in range(min(n, 256))]

    def kernel_stats(self):
        """Per strip-width class: dict(strip_width, pairs, cells, ms) of the last execute."""
        out = []
        plan_cls = lib().ltr_plan_kernel_class(self._h)
        for k in range(lib().ltr_num_kernels()):
            w, n, c, ms = C.c_int(0), C.c_int64(0), C.c_double(0), C.c_float(0)
            self.ctx._check(lib().ltr_plan_kernel_stats(self._h, k, C.byref(w), C.byref(n), C.byref(c), C.byref(ms)))
            d = dict(strip_width=w.value, pairs=n.value, cells=c.value, ms=ms.value,
                     lanes_per_pair=lib().ltr_kernel_lanes_per_pair(k),
                     family=FAMILIES.get(lib().ltr_kernel_family(k), "?"))
            lanes, widths, npairs = (C.c_int32 * 256)(), (C.c_int32 * 256)(), (C.c_int64 * 256)()
            nr = lib().ltr_plan_kernel_ranges(self._h, k, lanes, widths, npairs)
            if nr > 0:                                  # a launch over several classes: (lanes per pair, strip width, pairs) in launch order
                d["ranges"] = [(int(lanes[i]), int(widths[i]), int(npairs[i])) for i in range(nr)]
            if k == plan_cls:
                d["plan_kernel"] = True                 # the one launch of every one-wave class and packed width (ltr_dp_plan.hpp)
            out.append(d)
        return out

    @staticmethod
    def exact_pairs(stats):
        """Pairs the exact (redo) kernels scored in the execute the stats belong to."""
        return sum(k["pairs"] for k in stats if k["family"] == "exact")


def get_alleles(packed_vcf_locus):
    buf = C.create_string_buffer(1 << 20)
    off = np.zeros(1024, dtype=np.int64)
    pos = C.c_int32(0)
    n = lib().ltr_get_alleles(C.byref(packed_vcf_locus.struct), C.byref(pos), buf, len(buf), _p(off))
    if n < 0:
        raise LtrError(n, "ltr_get_alleles")
    raw = buf.raw
    return pos.value, [raw[off[i]:off[i + 1]].decode() for i in range(n)]


def vcf_record(packed_vcf_locus, options=None):
    """ltr_vcf_record: (VCF line, 1-based position)."""
    pos = C.c_int32(0)
    text = text_call("ltr_vcf_record", 1 << 22, lambda buf, cap: lib().ltr_vcf_record(
        C.byref(packed_vcf_locus.struct), None if options is None else C.byref(options), buf, cap, C.byref(pos)))
    return text, pos.value


def vcf_fields(packed_vcf_locus, want=("gls", "pls", "phased_gls")):
    """ltr_vcf_fields: the arithmetic half of ltr_vcf_record on the host -- the LocusFields.to_dict() image."""
    L = lib()
    h = C.c_void_p()
    rc = L.ltr_vcf_fields(C.byref(packed_vcf_locus.struct), int("gls" in want), int("pls" in want), int("phased_gls" in want), C.byref(h))
    if rc != 0:
        raise LtrError(rc, "ltr_vcf_fields")
    try:
        return L.ltr_vcf_field_set_view(h).contents.to_dict()
    finally:
        L.ltr_vcf_field_set_free(h)


def vcf_record_from_fields(packed_vcf_locus, fields, options=None):
    """ltr_vcf_record_from_fields: (VCF line, 1-based position) from a fields image (vcf_fields / GenotypeResult.fields)."""
    if fields is None:
        f, keep, ref = None, None, None
    else:
        f, keep = _abi.LocusFields.from_dict(fields)
        ref = C.byref(f)
    pos = C.c_int32(0)
    text = text_call("ltr_vcf_record_from_fields", 1 << 22, lambda buf, cap: lib().ltr_vcf_record_from_fields(
        C.byref(packed_vcf_locus.struct), ref, None if options is None else C.byref(options), buf, cap, C.byref(pos)))
    return text, pos.value


class GenotypeResult(Handle):
    """A ltr_genotype_result of Plan.genotype_fields / Context.genotype_ll, kept on the library's side until close()."""

    _free = "ltr_genotype_result_free"

    def __init__(self, ctx, handle, packed, per_sample=True):
        """per_sample=False: the call gave no ploidy per sample, so the samples of a locus have the locus's (sample_haploid() then
        asks the library once per locus, not once per sample)."""
        self.ctx, self._h, self._packed, self._per_sample, self._flags = ctx, handle, packed, per_sample, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_loci(self):
        return int(lib().ltr_genotype_result_n_loci(self._h))

    def haploid(self, l):
        """ltr_genotype_result_haploid: the ploidy locus l was genotyped with (0 / 1)."""
        rc = lib().ltr_genotype_result_haploid(self._h, int(l))
        if rc < 0:
            raise LtrError(rc, "ltr_genotype_result_haploid")
        return int(rc)

    def sample_haploid(self, l):
        """ltr_genotype_result_sample_haploid: the ploidy every sample of locus l was genotyped with ([S] of 0 / 1)."""
        if not 0 <= int(l) < self.n_loci:
            raise LtrError(_abi.LTR_ERR_INVALID, "ltr_genotype_result_sample_haploid")
        l = int(l)
        if l not in self._flags:                                 # (asked for by fields() and locus() alike: once per locus)
            S, L = int(self._packed["n_samples"][l]), lib()
            if self._per_sample:
                out = np.asarray([L.ltr_genotype_result_sample_haploid(self._h, l, s) for s in range(S)], dtype=np.int32)
                if (out < 0).any():
                    raise LtrError(int(out.min()), "ltr_genotype_result_sample_haploid")
            else:
                out = np.full(S, self.haploid(l), dtype=np.int32)
            self._flags[l] = out.astype(np.uint8)
        return self._flags[l].copy()

    def fields(self, l):
        """The LocusFields.to_dict() image of locus l (copies) + "sample_haploid" [S]: in a mixed locus (diploid widths) a haploid
        sample's gls / pls row holds its V values first and 0 after them, its phased_gls row 0.0."""
        f = _abi.LocusFields()
        rc = lib().ltr_genotype_result_fields(self._h, int(l), C.byref(f))
        if rc != 0:
            raise LtrError(rc, "ltr_genotype_result_fields")
        return dict(f.to_dict(), sample_haploid=self.sample_haploid(l))

    def locus(self, l):
        """What Plan.genotype returns for locus l: post / read_ll are None when they were not asked for."""
        L, h, packed = lib(), self._h, self._packed
        take = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
        ns, lro = packed["n_samples"], packed["locus_read_off"]
        S, R, Hn = int(ns[l]), int(lro[l + 1] - lro[l]), L.ltr_genotype_result_n_haps(h, l)
        old = packed["loci_blocks"][l]
        Ho = int(np.prod([len(b["alleles"]) for b in old], dtype=np.int64))
        removed = []
        for b in range(len(old)):
            ptr = C.POINTER(C.c_int32)()
            n = L.ltr_genotype_result_removed(h, l, b, C.byref(ptr))
            removed.append([ptr[i] for i in range(n)])
        post, rll = L.ltr_genotype_result_log_sample_posteriors(h, l), L.ltr_genotype_result_read_ll(h, l)
        return dict(
            sample_haploid=self.sample_haploid(l), n_haps=Hn, new_to_old=take(L.ltr_genotype_result_new_to_old(h, l), Hn, np.int32),
            allele_mapping=take(L.ltr_genotype_result_allele_mapping(h, l), Ho, np.int32), removed=removed,
            num_aff_blocks=L.ltr_genotype_result_num_aff_blocks(h, l), num_aff_alleles=L.ltr_genotype_result_num_aff_alleles(h, l),
            blocks=_abi.blocks_from_struct(L.ltr_genotype_result_blocks(h, l).contents) if any(removed) else old,
            post=take(post, S * Hn * Hn, np.float64).reshape(S, Hn, Hn) if post else None,
            sample_total_ll=take(L.ltr_genotype_result_sample_total_ll(h, l), S, np.float64),
            gts=take(L.ltr_genotype_result_gts(h, l), 2 * S, np.int32).reshape(S, 2),
            read_ll=take(rll, R * Hn, np.float64).reshape(R, Hn) if rll else None)

    def vcf_records(self, packed_vcf_loci, options=None):
        """ltr_genotype_result_vcf_records: (list of VCF lines, positions) for every locus, formatted on the worker pool.
        packed_vcf_loci: one _abi.PackedVcfLocus per locus (its blocks / block / haploid are replaced by the result's own)."""
        L = lib()
        n = self.n_loci
        if len(packed_vcf_loci) != n:
            raise LtrError(-1, "vcf_records: one locus description per locus")
        arr = (_abi.VcfLocus * max(n, 1))(*[p.struct for p in packed_vcf_loci])
        text = C.c_void_p()
        off = np.zeros(n + 1, dtype=np.int64)
        pos = np.zeros(max(n, 1), dtype=np.int32)
        self.ctx._check(L.ltr_genotype_result_vcf_records(self._h, arr, None if options is None else C.byref(options), C.byref(text), _p(off), _p(pos)))
        try:
            raw = C.string_at(text, int(off[n]))
        finally:
            L.ltr_vcf_text_free(text)
        return [raw[off[l]:off[l + 1] - 1].decode() for l in range(n)], pos[:n].copy()


def _sample_haploid(sample_haploid, n_samples, locus_haploid=None):
    """The uint8 array of the *_sample_ploidy entry points (unit order) from one array of S_l flags per locus."""
    if locus_haploid is not None:
        raise LtrError(_abi.LTR_ERR_INVALID, "sample_haploid and locus_haploid in one call: give the ploidy once")
    if len(sample_haploid) != len(n_samples):
        raise LtrError(_abi.LTR_ERR_INVALID, f"sample_haploid: one array per locus ({len(n_samples)}), got {len(sample_haploid)}")
    rows = [np.atleast_1d(np.asarray(f)).astype(bool).astype(np.uint8) for f in sample_haploid]
    for l, (f, S) in enumerate(zip(rows, n_samples)):
        if f.shape != (int(S),):
            raise LtrError(_abi.LTR_ERR_INVALID, f"sample_haploid: locus {l} has {int(S)} samples, got {f.size} flags")
    return np.ascontiguousarray(np.concatenate(rows + [np.zeros(1, dtype=np.uint8)]))     # (never empty: a valid address)


def _locus_haploid(locus_haploid, n_loci):
    """The [n_loci] uint8 array of the *_ploidy entry points."""
    lh = np.ascontiguousarray(locus_haploid).astype(bool).astype(np.uint8)
    if lh.shape != (n_loci,):
        raise LtrError(_abi.LTR_ERR_INVALID, "locus_haploid: one entry per locus")
    return lh
