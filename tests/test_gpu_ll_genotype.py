"""-m gpu: ltr_ll_genotype -- the consumer of a resident plan (ltr_plan_genotype / ltr_plan_genotype_fields /
ltr_genotype_result_vcf_records) on per-read matrices in caller memory.  The per-read matrices are scattered out of an executed
plan (ltr_scatter_pool_probs, seq_stutter_genotyper.cpp:526-538), so both paths see the same scores and every number must be
the same BITS: the kernels of the new path differ from the plan's in the row a read takes, not in one operation."""
import ctypes as C

import numpy as np
import pytest

import genotype_util as gt
import vcf_fields_util as vu
from longtr_amd import _abi, _lib, synth
from test_gpu_plan_fields import ALL_OPT, _describe
from test_gpu_plan_genotype import SEED, _big_locus, _filtered

pytestmark = pytest.mark.gpu
WANT = dict(want_gls=True, want_pls=True, want_phased_gls=True, want_posteriors=True)
_CACHE = {}


def _loci():
    """~40 loci: make_case data (H from 2 up, two-block loci, scores below the clamp, samples without reads, filtered samples)
    and, crafted: H = 1, 2, 8 and 9 (8 / 9: the 64- / 256-thread workgroups), a repeat block of 48 alleles (its V x V table is
    beyond the 2 048 doubles of LDS), a locus with a sample that has no read at all."""
    loci = gt.make_case(SEED + 7, n_loci=34, reads=(4, 24))
    rng = np.random.default_rng(97)
    for nall in (2, 2, 8, 9):
        loci.append(_big_locus(rng, nall, 12, 2, False))
    one = loci[-4]                                               # H = 1: a single allele everywhere
    one["blocks"][1]["alleles"] = one["blocks"][1]["alleles"][:1]
    one["haps"] = gt.gray_seqs(one["blocks"])
    loci.append(_big_locus(rng, 48, 60, 3, False, tr_len=150))
    empty = _big_locus(rng, 3, 10, 2, False)
    empty["S"], empty["filt"] = 4, np.zeros(4, dtype=np.uint8)   # samples 2 and 3 have no read
    loci.append(empty)
    loci[0]["filt"][0] = 1
    assert sorted({len(L["haps"]) for L in loci} & {1, 2, 8, 9}) == [1, 2, 8, 9]
    assert len(loci[-2]["blocks"][1]["alleles"]) ** 2 > 2048 and any(L["filt"].any() for L in loci)
    return loci


def _case(ctx):
    """One executed plan for the module: loci, the plan, its arguments, the per-read matrices and seeds scattered out of it.  Every
    pool that holds a read of sample 0 of every second locus is masked out (seed -1, HapAligner.cpp:557-560): that sample has no
    aligned read.  The plan writes its scores into a buffer of our own, so the masked rows hold known values."""
    if "case" in _CACHE:
        return _CACHE["case"]
    hip = C.CDLL("libamdhip64.so")
    loci = _loci()
    mask = []
    for l, L in enumerate(loci):
        keep = np.ones(len(L["pools"]), dtype=np.uint8)
        if l % 2 == 0 and L["S"] > 1:
            keep[np.unique(L["pool_index"][L["lab"] == 0])] = 0
        mask.append(keep)
    _, args = gt.pack(loci)
    batch = _abi.PackedBatch([(L["pools"], L["haps"]) for L in loci], realign_read=np.concatenate(mask))
    plan = ctx.plan(batch)
    nbytes = max(plan.ll_size, 1) * 8
    d_out = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_out), C.c_size_t(nbytes)) == 0
    init, at = np.full(max(plan.ll_size, 1), -50.0), 0
    for L in loci:
        P, H = len(L["pools"]), len(L["haps"])
        init[at:at + P * H].reshape(P, H)[:, H - 1] = 0.0
        at += P * H
    assert hip.hipMemcpy(d_out, C.c_void_p(init.ctypes.data), C.c_size_t(nbytes), 1) == 0 and hip.hipDeviceSynchronize() == 0
    plan.execute(d_out_ptr=d_out)
    plan.wait()
    _, seeds = plan.fetch()
    ll = np.zeros(max(plan.ll_size, 1))
    assert hip.hipMemcpy(C.c_void_p(ll.ctypes.data), d_out, C.c_size_t(nbytes), 2) == 0
    assert (seeds < 0).any() and (ll < -600.0).any()
    mats, rseeds = [], []
    for l, L in enumerate(loci):
        r0 = int(batch.locus_read_off[l])
        M, s = _lib.scatter_pool_probs(batch.locus_matrix(ll, l), seeds[r0:r0 + len(L["pools"])], L["pool_index"], len(L["haps"]))
        mats.append(M)
        rseeds.append(s)
    largs = {k: v for k, v in args.items() if k != "pool_index"}
    case = dict(loci=loci, plan=plan, args=args, largs=largs, mats=mats, seeds=rseeds, blocks=[L["blocks"] for L in loci], d_out=d_out, hip=hip)
    _CACHE["case"] = case
    return case


def _decode(res, case, haploid, records=True):
    """Everything a result hands out, per locus, and the record text."""
    out = dict(loci=[res.locus(l) for l in range(res.n_loci)])
    if records:
        out["fields"] = [res.fields(l) for l in range(res.n_loci)]
        rng = np.random.default_rng(7)
        packed = [_abi.PackedVcfLocus(_describe(l, L, out["loci"][l], haploid, rng)) for l, L in enumerate(case["loci"])]
        out["lines"], out["pos"] = res.vcf_records(packed, _abi.vcf_options(output_pls=1, **ALL_OPT))
    return out


def _plan_reference(ctx, haploid, prune):
    key = ("ref", haploid, prune)
    if key not in _CACHE:
        case = _case(ctx)
        kw = dict(haploid=haploid, sample_filtered=_filtered(case["loci"]), prune=prune, **case["args"])
        with case["plan"].genotype_fields(case["blocks"], want_read_ll=True, **WANT, **kw) as res:
            ref = _decode(res, case, haploid)
        ref["genotype"] = case["plan"].genotype(case["blocks"], want_read_ll=True, **kw)      # ltr_plan_genotype itself
        _CACHE[key] = ref
    return _CACHE[key]


def _same_locus(got, want, l, read_ll=True, post=True):
    for k in ("n_haps", "removed", "num_aff_blocks", "num_aff_alleles"):
        assert got[k] == want[k], (l, k)
    for k in ("new_to_old", "allele_mapping", "gts"):
        assert np.array_equal(got[k], want[k]), (l, k)
    assert np.array_equal(vu.bits(got["sample_total_ll"]), vu.bits(want["sample_total_ll"])), l
    if post:
        assert np.array_equal(vu.bits(got["post"]), vu.bits(want["post"])), l
    else:
        assert got["post"] is None, l
    if read_ll:
        assert np.array_equal(vu.bits(got["read_ll"]), vu.bits(want["read_ll"])), l
    else:
        assert got["read_ll"] is None, l
    assert [b["alleles"] for b in got["blocks"]] == [b["alleles"] for b in want["blocks"]], l


def _same_fields(got, want, l):
    assert all(got[k] == want[k] for k in ("S", "R", "V", "block", "n_gl", "n_pgl")), l
    for k in vu.ARRAYS:
        a, b = got[k], want[k]
        assert (a is None) == (b is None), (l, k)
        if a is not None:
            assert np.array_equal(vu.bits(a), vu.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (l, k)


def _same_result(got, want, read_ll=True, post=True):
    assert len(got["loci"]) == len(want["loci"])
    for l in range(len(want["loci"])):
        _same_locus(got["loci"][l], want["loci"][l], l, read_ll, post)
        if "fields" in got:
            _same_fields(got["fields"][l], want["fields"][l], l)
    if "lines" in got:
        assert [x.encode() for x in got["lines"]] == [x.encode() for x in want["lines"]] and got["pos"].tolist() == want["pos"].tolist()


def _ll_call(ctx, case, haploid, prune, want_read_ll=True, fields=WANT, records=True):
    with ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], haploid=haploid, prune=prune, want_read_ll=want_read_ll,
                         fields=fields, sample_filtered=_filtered(case["loci"]), **case["largs"]) as res:
        assert res.n_loci == len(case["loci"])
        return _decode(res, case, haploid, records)


@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("prune", [True, False])
def test_same_bits_as_the_plan_path(gpu_ctx, haploid, prune):
    case = _case(gpu_ctx)
    ref = _plan_reference(gpu_ctx, haploid, prune)
    # the case reaches the branches: loci that lose an allele and loci that do not, a sample whose reads all have seed -1
    lost = [any(g["removed"]) for g in ref["loci"]]
    assert not prune or (any(lost) and not all(lost))
    assert any((s < 0).all() and len(s) for L, sd in zip(case["loci"], case["seeds"]) for s in [sd[L["lab"] == 0]])
    assert prune or max(f["V"] for f in ref["fields"]) ** 2 > 2048       # the V x V table beyond LDS (pruning shrinks it)
    # with fields: every accessor, every field, the record text
    _same_result(_ll_call(gpu_ctx, case, haploid, prune), ref)
    # fr == NULL: as ltr_plan_genotype (posteriors always there), read_ll off
    got = _ll_call(gpu_ctx, case, haploid, prune, want_read_ll=False, fields=None, records=False)
    for l, want in enumerate(ref["genotype"]):
        _same_locus(got["loci"][l], want, l, read_ll=False)
    # want_posteriors 0: nothing but the fields comes back, the same fields
    got = _ll_call(gpu_ctx, case, haploid, prune, want_read_ll=False, fields=dict(WANT, want_posteriors=False), records=False)
    for l, want in enumerate(ref["loci"]):
        _same_locus(got["loci"][l], want, l, read_ll=False, post=False)
    with gpu_ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], haploid=haploid, prune=prune,
                             fields=dict(WANT, want_posteriors=False), sample_filtered=_filtered(case["loci"]), **case["largs"]) as res:
        for l, want in enumerate(ref["fields"]):
            _same_fields(res.fields(l), want, l)


def test_seeds_decide_and_null_seeds_mean_aligned(gpu_ctx):
    """seed_positions NULL (or a NULL entry) = every read aligned: the masked samples' best pairs then keep alleles alive."""
    case = _case(gpu_ctx)
    ref = _plan_reference(gpu_ctx, False, True)
    kw = dict(sample_filtered=_filtered(case["loci"]), **case["largs"])
    with gpu_ctx.genotype_ll(case["mats"], None, case["blocks"], **kw) as res:
        none = [res.locus(l) for l in range(res.n_loci)]
    some = [None if l % 2 == 0 else s for l, s in enumerate(case["seeds"])]
    with gpu_ctx.genotype_ll(case["mats"], some, case["blocks"], **kw) as res:
        partly = [res.locus(l) for l in range(res.n_loci)]
    assert sum(a["removed"] != b["removed"] for a, b in zip(none, ref["loci"])) >= 1
    for l, (a, b) in enumerate(zip(partly, none)):
        assert a["removed"] == b["removed"] and np.array_equal(a["gts"], b["gts"]), l


def test_upload_chunks_and_thread_budgets(gpu_ctx):
    """The upload in chunks of 1 locus, of 7 loci and in one piece, gathered by 2 and by 16 host threads: the same result."""
    case = _case(gpu_ctx)
    ref = _plan_reference(gpu_ctx, False, True)
    try:
        for chunk, budget in ((1, 16), (7, 2), (7, 16), (0, 2), (10 ** 6, 16)):
            gpu_ctx.set_debug("ll_chunk_loci", chunk)
            gpu_ctx.set_host_threads(budget)
            _same_result(_ll_call(gpu_ctx, case, False, True, records=False), ref)
    finally:
        gpu_ctx.set_debug("ll_chunk_loci", 0)
        gpu_ctx.set_host_threads(0)


def test_input_is_not_written(gpu_ctx):
    case = _case(gpu_ctx)
    mats = [m.copy() for m in case["mats"]]
    before = [m.tobytes() for m in mats]
    assert any((m < -600.0).any() for m in mats)
    with gpu_ctx.genotype_ll(mats, case["seeds"], case["blocks"], want_read_ll=True, fields=WANT, sample_filtered=_filtered(case["loci"]),
                             **case["largs"]) as res:
        l = next(l for l, m in enumerate(mats) if (m < -600.0).any())
        assert res.locus(l)["read_ll"].min() >= -600.0           # ... the clamp happened, on the library's copy
    assert [m.tobytes() for m in mats] == before


def test_short_path_matrices_equal_the_per_locus_composition(gpu_ctx):
    """Period-1 loci scored by the seeded stutter path never enter a plan: their matrices and seeds straight out of
    ltr_calc_hap_aln_probs, one read without a seed.  Reference: ltr_posteriors -> ltr_unused_alleles -> ltr_prune_hap_blocks /
    ltr_remap_haplotypes -> ltr_remap_aln_probs -> ltr_posteriors per locus, bit for bit."""
    import short_util as su
    rng = np.random.default_rng(41)
    loci, inputs = [], []
    for tr, H, R in [(8, 2, 6), (14, 3, 9), (25, 4, 8), (11, 3, 7)]:
        blocks, alns = su.homopolymer_locus(rng, tr, H, R)
        alns[0] = dict(alns[0], cigar=[("X", len(alns[0]["seq"]))])          # no seed: an all-zero row, seed -1
        lab = (np.arange(R) % 2).astype(np.int32)
        lab[0] = 1
        loci.append(dict(blocks=blocks, S=3, lab=lab, p1=-rng.random(R) * 0.01, p2=-rng.random(R) * 0.01, filt=np.zeros(3, dtype=np.uint8),
                         pool_index=np.arange(R, dtype=np.int32)))
        inputs.append((blocks, alns))
    old = gpu_ctx.params
    gpu_ctx.set_params(_abi.make_params(_abi.default_params().as_tuple()[:7], use_short_path=1))
    try:
        outs = gpu_ctx.calc_hap_aln_probs(inputs)
    finally:
        gpu_ctx.set_params(old)
    assert all(s[0] == -1 and (s >= 0).any() for _, s in outs)
    lro = np.zeros(len(loci) + 1, dtype=np.int64)
    lro[1:] = np.cumsum([len(L["lab"]) for L in loci])
    cat = lambda k: np.concatenate([L[k] for L in loci])
    for haploid in (False, True):
        with gpu_ctx.genotype_ll([m for m, _ in outs], [s for _, s in outs], [L["blocks"] for L in loci], lro, cat("p1"), cat("p2"), cat("lab"),
                                 [L["S"] for L in loci], haploid=haploid, want_read_ll=True) as res:
            for l, L in enumerate(loci):
                M, seeds = outs[l]
                want = gt.chain(dict(L, seeds=seeds), M, lambda *a: gpu_ctx.posteriors(a[0], a[1], a[2], a[3], a[4], haploid=a[5]),
                                _lib.unused_alleles, _lib.haps_to_alleles, _lib.remap_haplotypes, _lib.remap_aln_probs, haploid)
                got = res.locus(l)
                assert got["removed"] == want["removed"] and np.array_equal(got["new_to_old"], want["new_to_old"]), l
                assert np.array_equal(got["allele_mapping"], want["allele_mapping"]) and np.array_equal(got["gts"], want["gts"]), l
                for k in ("post", "sample_total_ll", "read_ll"):
                    assert np.array_equal(gt.bits(got[k]), gt.bits(want[k])), (l, k)


def test_errors_launch_nothing_and_name_the_locus(gpu_ctx):
    case = _case(gpu_ctx)
    L = _lib.lib()
    kw = dict(sample_filtered=_filtered(case["loci"]), **case["largs"])

    def fails(text, packed, fr=None):
        h = C.c_void_p(0x1234)
        rc = L.ltr_ll_genotype(gpu_ctx._h, C.byref(packed["lb"]), C.byref(packed["gb"]), None if fr is None else C.byref(fr), C.byref(h))
        msg = L.ltr_last_error(gpu_ctx._h).decode()
        assert rc == _abi.LTR_ERR_INVALID and not h.value and text in msg, (rc, h.value, msg)

    wrong = list(case["blocks"])                                 # n_haps[5] no longer what haps[5] enumerates
    wrong[5] = [dict(b, alleles=list(b["alleles"])) for b in wrong[5]]
    wrong[5][1]["alleles"].append(wrong[5][1]["alleles"][0] + b"ACG")
    fails("locus 5", gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], wrong, **kw))
    holes = list(case["mats"])
    holes[3] = None                                              # a locus with reads and no matrix
    fails("locus 3", gpu_ctx.pack_ll_genotype(holes, case["seeds"], case["blocks"], **kw))
    packed = gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], case["blocks"], prune=False, **kw)
    packed["gb"].haps = None                                      # fine without fields and pruning, not with fr
    with gpu_ctx.genotype_ll(packed=packed) as res:
        assert res.n_loci == len(case["loci"])
    fails("locus 0", packed, _abi.FieldsRequest())
    lab = case["largs"]["sample_label"].copy()
    lab[3] = 99
    fails("out of range", gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], case["blocks"], **dict(kw, sample_label=lab)))
    ref = _plan_reference(gpu_ctx, False, True)                  # and the context is still good
    _same_result(_ll_call(gpu_ctx, case, False, True, records=False), ref)


def test_release_the_module_plan(gpu_ctx):
    """(last in the file: the plan and the score buffer the cases above share go back)"""
    case = _CACHE.pop("case", None)
    _CACHE.clear()
    if case:
        case["plan"].close()
        assert case["hip"].hipFree(case["d_out"]) == 0
