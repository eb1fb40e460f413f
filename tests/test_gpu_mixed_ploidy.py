"""-m gpu: per-locus ploidy (ltr_plan_posteriors_ploidy, ltr_plan_genotype_ploidy, ltr_ll_genotype_ploidy,
ltr_genotype_result_haploid, ltr_genotype_result_vcf_records on a mixed result).  The reference decides ploidy per chromosome
(genotyper_bam_processor.cpp:248 -> :294); a plan cuts across chromosomes.  Loci are independent, so the reference of a mixed
call is the code as it stood: for the same plan and the same scores one uniform call with haploid = 0 and one with haploid = 1
give, per locus, exactly what the mixed call must give for that locus's ploidy.  Every comparison is bit for bit: view(uint64)
on doubles, array_equal on integers, byte equality on text.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import genotype_util as gt
import vcf_fields_util as vu
from longtr_amd import _abi, _lib
from test_gpu_ll_genotype import WANT, _same_fields, _same_locus
from test_gpu_plan_fields import ALL_OPT, _describe
from test_gpu_plan_genotype import _big_locus, _filtered

pytestmark = pytest.mark.gpu
SEED = 106   # chosen on the CPU (oracle DP + oracle chain with the masks below): H reaches 12, pruning removes an allele on 8 of the
#              diploid and 10 of the haploid loci of the pattern, and no sample's two best diplotypes lie within 1e-6
N_LOCI = 24
_CACHE = {}


def _pattern(n):
    """1,0,0,1,1,0,0,1,1,...: both ploidies next to each other, the first and (n = 24) the last locus haploid."""
    return np.asarray([1 if (l + 1) % 4 < 2 else 0 for l in range(n)], dtype=np.uint8)


def _loci():
    """24 small loci: 20 of make_case (H 2 to 12, one to three samples of 4 to 23 reads, two-block loci, scores below the
    clamp, filtered samples) and, crafted: H = 1, H = 9 (the 256-thread workgroups), a locus without a read, and a last one."""
    loci = gt.make_case(SEED, n_loci=20, reads=(4, 24))
    rng = np.random.default_rng(SEED + 1)
    for L in loci:                                               # one to three samples
        if L["S"] > 3:
            L["S"] = 3
            L["lab"] = (L["lab"] % 3).astype(np.int32)
            L["filt"] = L["filt"][:3].copy()
    one = _big_locus(rng, 2, 12, 2, False)                       # H = 1: a single allele everywhere
    one["blocks"][1]["alleles"] = one["blocks"][1]["alleles"][:1]
    one["haps"] = gt.gray_seqs(one["blocks"])
    nine = _big_locus(rng, 9, 12, 2, False)
    empty = _big_locus(rng, 3, 10, 2, False)                     # no read at all: two samples that hold their priors alone
    empty.update(pools=[], pool_index=np.zeros(0, dtype=np.int32), lab=np.zeros(0, dtype=np.int32), p1=np.zeros(0), p2=np.zeros(0))
    last = _big_locus(rng, 4, 16, 3, True)
    loci[3:3] = [one]                                            # haploid in the pattern
    loci[6:6] = [empty]                                          # diploid
    loci += [nine, last]                                         # diploid, haploid
    assert len(loci) == N_LOCI
    H = [len(L["haps"]) for L in loci]
    assert min(H) == 1 and 9 <= max(H) <= 12 and {L["S"] for L in loci} == {1, 2, 3}
    assert sum(len(L["lab"]) == 0 for L in loci) == 1
    return loci


def _masks(loci):
    """Every pool that holds a read of sample 0 of every second locus with more than one sample is masked out (seed -1,
    HapAligner.cpp:557-560): that sample has no aligned read (seq_stutter_genotyper.cpp:262-266)."""
    mask = []
    for l, L in enumerate(loci):
        keep = np.ones(len(L["pools"]), dtype=np.uint8)
        if l % 2 == 0 and L["S"] > 1 and len(L["pools"]):
            keep[np.unique(L["pool_index"][L["lab"] == 0])] = 0
        mask.append(keep)
    return mask


def _initial_scores(loci):
    """What the masked rows keep (the plan writes into a buffer of ours): -50, the last haplotype 0."""
    size = sum(len(L["pools"]) * len(L["haps"]) for L in loci)
    init, at = np.full(max(size, 1), -50.0), 0
    for L in loci:
        P, H = len(L["pools"]), len(L["haps"])
        init[at:at + P * H].reshape(P, H)[:, H - 1] = 0.0
        at += P * H
    return init


def _case(ctx):
    """One executed plan for the module, its per-read matrices and seeds, and the four uniform references of each path
    (haploid 0 / 1 x prune 0 / 1), computed once and shared by the cases below."""
    if "case" in _CACHE:
        return _CACHE["case"]
    hip = C.CDLL("libamdhip64.so")
    loci = _loci()
    _, args = gt.pack(loci)
    batch = _abi.PackedBatch([(L["pools"], L["haps"]) for L in loci], realign_read=np.concatenate(_masks(loci)))
    plan = ctx.plan(batch)
    nbytes = max(plan.ll_size, 1) * 8
    d_out = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_out), C.c_size_t(nbytes)) == 0
    init = _initial_scores(loci)
    assert init.size == max(plan.ll_size, 1)
    assert hip.hipMemcpy(d_out, C.c_void_p(init.ctypes.data), C.c_size_t(nbytes), 1) == 0 and hip.hipDeviceSynchronize() == 0
    plan.execute(d_out_ptr=d_out)
    plan.wait()
    _, seeds = plan.fetch()
    ll = np.zeros(max(plan.ll_size, 1))
    assert hip.hipMemcpy(C.c_void_p(ll.ctypes.data), d_out, C.c_size_t(nbytes), 2) == 0
    assert (seeds < 0).any()
    mats, rseeds = [], []
    for l, L in enumerate(loci):
        if len(L["lab"]) == 0:
            mats.append(None); rseeds.append(None)
            continue
        r0 = int(batch.locus_read_off[l])
        M, s = _lib.scatter_pool_probs(batch.locus_matrix(ll, l), seeds[r0:r0 + len(L["pools"])], L["pool_index"], len(L["haps"]))
        mats.append(M); rseeds.append(s)
    assert any((s[L["lab"] == 0] < 0).all() and (L["lab"] == 0).any() for L, s in zip(loci, rseeds) if s is not None)   # a sample without an aligned read
    case = dict(loci=loci, plan=plan, args=args, largs={k: v for k, v in args.items() if k != "pool_index"}, mats=mats, seeds=rseeds,
                blocks=[L["blocks"] for L in loci], filt=_filtered(loci), pattern=_pattern(len(loci)), d_out=d_out, hip=hip)
    _CACHE["case"] = case
    return case


def _decode(res, case, describe_haploid):
    """Everything a fields result hands out, per locus, and the record text.  describe_haploid(l): what ltr_vcf_locus.haploid says."""
    out = dict(loci=[res.locus(l) for l in range(res.n_loci)], fields=[res.fields(l) for l in range(res.n_loci)],
               haploid=[res.haploid(l) for l in range(res.n_loci)])
    rng = np.random.default_rng(7)
    packed = [_abi.PackedVcfLocus(_describe(l, L, out["loci"][l], describe_haploid(l), rng)) for l, L in enumerate(case["loci"])]
    out["lines"], out["pos"] = res.vcf_records(packed, _abi.vcf_options(output_pls=1, **ALL_OPT))
    return out


def _plan_uniform(ctx, haploid, prune):
    """The reference: the uniform calls through the entry points as they were (ltr_plan_posteriors, ltr_plan_genotype,
    ltr_plan_genotype_fields + records)."""
    key = ("plan", haploid, prune)
    if key not in _CACHE:
        case = _case(ctx)
        kw = dict(haploid=bool(haploid), sample_filtered=case["filt"], prune=bool(prune), **case["args"])
        with case["plan"].genotype_fields(case["blocks"], want_read_ll=True, **WANT, **kw) as res:
            ref = _decode(res, case, lambda l: bool(haploid))
        ref["genotype"] = case["plan"].genotype(case["blocks"], want_read_ll=True, **kw)
        _CACHE[key] = ref
    return _CACHE[key]


def _ll_uniform(ctx, haploid, prune):
    key = ("ll", haploid, prune)
    if key not in _CACHE:
        case = _case(ctx)
        with ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], haploid=bool(haploid), prune=bool(prune), want_read_ll=True,
                             fields=WANT, sample_filtered=case["filt"], **case["largs"]) as res:
            _CACHE[key] = _decode(res, case, lambda l: bool(haploid))
    return _CACHE[key]


def _first_uniform(ctx, haploid):
    key = ("first", haploid)
    if key not in _CACHE:
        case = _case(ctx)
        _CACHE[key] = case["plan"].posteriors(haploid=bool(haploid), **case["args"])
    return _CACHE[key]


def _same_as_uniform(got, refs, pattern, with_fields):
    """Locus l of the mixed result against locus l of the uniform result of its ploidy: every accessor, field and record."""
    assert got["haploid"] == pattern.tolist()
    for l, p in enumerate(pattern):
        want = refs[int(p)]
        _same_locus(got["loci"][l], want["loci"][l], l)
        if with_fields:
            assert got["fields"][l]["n_gl"] == want["fields"][l]["n_gl"] and got["fields"][l]["n_pgl"] == want["fields"][l]["n_pgl"], l
            _same_fields(got["fields"][l], want["fields"][l], l)
            assert got["lines"][l].encode() == want["lines"][l].encode() and got["pos"][l] == want["pos"][l], (l, got["lines"][l], want["lines"][l])


def _pruning_happens(refs, pattern):
    """prune = 1 removes an allele on a haploid and on a diploid locus of the pattern (in the uniform calls), and not everywhere."""
    lost = {p: [l for l in range(len(pattern)) if pattern[l] == p and any(refs[p]["loci"][l]["removed"])] for p in (0, 1)}
    assert lost[0] and lost[1], lost
    assert any(not any(refs[int(p)]["loci"][l]["removed"]) for l, p in enumerate(pattern))
    return lost


def test_the_case_tells_the_ploidies_apart(gpu_ctx):
    """The two uniform references differ on every locus with a read (priors), in the widths of the fields and in FORMAT: a mixed
    call that ignored the array could not match both."""
    case = _case(gpu_ctx)
    dip, hap = _plan_uniform(gpu_ctx, 0, 1), _plan_uniform(gpu_ctx, 1, 1)
    pattern = case["pattern"]
    assert pattern[0] == 1 and pattern[-1] == 1 and pattern.tolist()[:6] == [1, 0, 0, 1, 1, 0] and 0 < pattern.sum() < len(pattern)
    differ = 0
    for l, L in enumerate(case["loci"]):
        d, h = dip["loci"][l], hap["loci"][l]
        if d["n_haps"] > 1 and h["n_haps"] > 1 and len(L["lab"]):     # (with one haplotype left both priors are log 1)
            assert not np.array_equal(vu.bits(d["sample_total_ll"]), vu.bits(h["sample_total_ll"])), l
            differ += 1
        Vd, Vh = dip["fields"][l]["V"], hap["fields"][l]["V"]     # (the ploidies may prune differently)
        assert (dip["fields"][l]["n_gl"], dip["fields"][l]["n_pgl"]) == (Vd * (Vd + 1) // 2, Vd * Vd), l
        assert (hap["fields"][l]["n_gl"], hap["fields"][l]["n_pgl"]) == (Vh, Vh), l
        assert dip["lines"][l].split("\t")[8].startswith("GT:GB:Q:PQ:DP:DSNP:DFLANKINDEL:PDP:PSNP:GLDIFF")
        assert hap["lines"][l].split("\t")[8].startswith("GT:GB:Q:DP:DFLANKINDEL:GLDIFF")
    assert differ >= 4
    _pruning_happens({0: dip, 1: hap}, pattern)


def test_posteriors_of_a_mixed_plan(gpu_ctx):
    """1. ltr_plan_posteriors_ploidy: posteriors, sample_total_ll and gts per locus equal the matching uniform call's."""
    case = _case(gpu_ctx)
    pattern = case["pattern"]
    post, off, stl, gts = case["plan"].posteriors(locus_haploid=pattern, **case["args"])
    refs = {p: _first_uniform(gpu_ctx, p) for p in (0, 1)}
    u = 0
    for l, L in enumerate(case["loci"]):
        rpost, roff, rstl, rgts = refs[int(pattern[l])]
        assert np.array_equal(off, roff)
        a, b = int(off[u]), int(off[u + L["S"]])
        assert np.array_equal(vu.bits(post[a:b]), vu.bits(rpost[a:b])), l
        assert np.array_equal(vu.bits(stl[u:u + L["S"]]), vu.bits(rstl[u:u + L["S"]])), l
        assert np.array_equal(gts[u:u + L["S"]], rgts[u:u + L["S"]]), l
        u += L["S"]
    assert u == len(stl)
    assert not np.array_equal(vu.bits(refs[0][2]), vu.bits(refs[1][2]))


@pytest.mark.parametrize("prune", [0, 1])
def test_genotype_of_a_mixed_plan_without_fields(gpu_ctx, prune):
    """2. ltr_plan_genotype_ploidy, fr = NULL, want_read_ll = 1: every accessor; ltr_genotype_result_haploid returns the pattern."""
    case = _case(gpu_ctx)
    pattern = case["pattern"]
    refs = {p: _plan_uniform(gpu_ctx, p, prune) for p in (0, 1)}
    if prune:
        _pruning_happens(refs, pattern)
    got = case["plan"].genotype(case["blocks"], want_read_ll=True, sample_filtered=case["filt"], prune=bool(prune), locus_haploid=pattern,
                                haploid=bool(prune), **case["args"])          # (`haploid` is not read when the array is given)
    assert [g["haploid"] for g in got] == pattern.tolist()
    for l, p in enumerate(pattern):
        _same_locus(got[l], refs[int(p)]["genotype"][l], l)
    for p in (0, 1):                                             # and the old entry point reports its one flag per locus
        assert [g["haploid"] for g in refs[p]["genotype"]] == [p] * len(pattern) == refs[p]["haploid"]


@pytest.mark.parametrize("prune", [0, 1])
def test_fields_and_records_of_a_mixed_plan(gpu_ctx, prune):
    """3. with a fields request: every member of ltr_locus_fields at the locus's own widths, the record text byte for byte;
    loci[l].haploid is set to the WRONG value on purpose -- it is ignored, the result's ploidy decides."""
    case = _case(gpu_ctx)
    pattern = case["pattern"]
    refs = {p: _plan_uniform(gpu_ctx, p, prune) for p in (0, 1)}
    with case["plan"].genotype_fields(case["blocks"], want_read_ll=True, sample_filtered=case["filt"], prune=bool(prune), locus_haploid=pattern,
                                      **WANT, **case["args"]) as res:
        got = _decode(res, case, lambda l: not pattern[l])
        _same_as_uniform(got, refs, pattern, True)
        # the packed optional arrays lie back to back at each locus's own width
        assert sum(f["gls"].size for f in got["fields"]) == sum(refs[int(p)]["fields"][l]["gls"].size for l, p in enumerate(pattern))
        with pytest.raises(_lib.LtrError):
            res.haploid(len(pattern))
    six = sum(line.split("\t")[8].startswith("GT:GB:Q:DP:") for line in got["lines"])
    assert six == int(pattern.sum())                             # six-field FORMAT on the haploid loci, ten fields on the others


@pytest.mark.parametrize("prune", [0, 1])
def test_ll_genotype_of_mixed_loci(gpu_ctx, prune):
    """4. ltr_ll_genotype_ploidy on the matrices fetched from the same plan: the comparisons of case 3, against the uniform
    ltr_ll_genotype calls (which carry the plan path's bits)."""
    case = _case(gpu_ctx)
    pattern = case["pattern"]
    refs = {p: _ll_uniform(gpu_ctx, p, prune) for p in (0, 1)}
    for p in (0, 1):
        plan_ref = _plan_uniform(gpu_ctx, p, prune)
        for l in range(len(pattern)):
            _same_locus(refs[p]["loci"][l], plan_ref["loci"][l], l)
    with gpu_ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], prune=bool(prune), want_read_ll=True, fields=WANT,
                             sample_filtered=case["filt"], locus_haploid=pattern, **case["largs"]) as res:
        _same_as_uniform(_decode(res, case, lambda l: not pattern[l]), refs, pattern, True)
    with gpu_ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], prune=bool(prune), want_read_ll=True, fields=None,
                             sample_filtered=case["filt"], locus_haploid=pattern, **case["largs"]) as res:      # fr = NULL
        assert [res.haploid(l) for l in range(res.n_loci)] == pattern.tolist()
        for l, p in enumerate(pattern):
            _same_locus(res.locus(l), refs[int(p)]["loci"][l], l)


def test_null_and_constant_arrays_are_the_old_entry_points(gpu_ctx):
    """5. locus_haploid = NULL with pb->haploid 0 and then 1 gives the bits of the old entry point; so do an all-zeros and an
    all-ones array (with pb->haploid set to the opposite: it is not read)."""
    case = _case(gpu_ctx)
    L = _lib.lib()
    plan, n = case["plan"], len(case["loci"])
    fr = _abi.FieldsRequest()
    fr.want_gls = fr.want_pls = fr.want_phased_gls = fr.want_posteriors = 1
    for p in (0, 1):
        ref, ll_ref, first = _plan_uniform(gpu_ctx, p, 1), _ll_uniform(gpu_ctx, p, 1), _first_uniform(gpu_ctx, p)
        const = np.full(n, p, dtype=np.uint8)
        uniform = np.full(n, p, dtype=np.uint8)
        # NULL through the new symbols
        packed = plan.pack_genotype(case["blocks"], haploid=bool(p), sample_filtered=case["filt"], prune=True, want_read_ll=True, **case["args"])
        h = C.c_void_p()
        assert L.ltr_plan_genotype_ploidy(plan._h, C.byref(packed["gb"]), C.byref(fr), None, C.byref(h)) == 0
        with _lib.GenotypeResult(gpu_ctx, h, packed) as res:
            _same_as_uniform(_decode(res, case, lambda l: bool(p)), {p: ref}, uniform, True)
        h = C.c_void_p()
        assert L.ltr_plan_genotype_ploidy(plan._h, C.byref(packed["gb"]), None, None, C.byref(h)) == 0
        with _lib.GenotypeResult(gpu_ctx, h, packed) as res:
            for l in range(n):
                _same_locus(res.locus(l), ref["genotype"][l], l)
        lp = gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], case["blocks"], haploid=bool(p), prune=True, want_read_ll=True,
                                      sample_filtered=case["filt"], **case["largs"])
        h = C.c_void_p()
        assert L.ltr_ll_genotype_ploidy(gpu_ctx._h, C.byref(lp["lb"]), C.byref(lp["gb"]), C.byref(fr), None, C.byref(h)) == 0
        with _lib.GenotypeResult(gpu_ctx, h, lp) as res:
            _same_as_uniform(_decode(res, case, lambda l: bool(p)), {p: ll_ref}, uniform, True)
        post, stl, gts = np.zeros_like(first[0]), np.zeros_like(first[2]), np.zeros(first[3].size, dtype=np.int32)
        assert L.ltr_plan_posteriors_ploidy(plan._h, C.byref(packed["gb"].pb.contents), None, _lib._p(post), _lib._p(stl), _lib._p(gts)) == 0
        assert np.array_equal(vu.bits(post), vu.bits(first[0])) and np.array_equal(vu.bits(stl), vu.bits(first[2])) and np.array_equal(gts.reshape(-1, 2), first[3])
        # a constant array, the batch's own flag saying the opposite
        with plan.genotype_fields(case["blocks"], haploid=not p, want_read_ll=True, sample_filtered=case["filt"], prune=True, locus_haploid=const,
                                  **WANT, **case["args"]) as res:
            _same_as_uniform(_decode(res, case, lambda l: bool(p)), {p: ref}, uniform, True)
        with gpu_ctx.genotype_ll(case["mats"], case["seeds"], case["blocks"], haploid=not p, prune=True, want_read_ll=True, fields=WANT,
                                 sample_filtered=case["filt"], locus_haploid=const, **case["largs"]) as res:
            _same_as_uniform(_decode(res, case, lambda l: bool(p)), {p: ll_ref}, uniform, True)
        got = plan.posteriors(haploid=not p, locus_haploid=const, **case["args"])
        for a, b in zip(got, first):
            assert np.array_equal(vu.bits(a), vu.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def test_errors_are_the_old_ones_and_launch_nothing(gpu_ctx):
    """6. a bad batch with locus_haploid given fails exactly as without it: LTR_ERR_INVALID, the same text, *out left NULL."""
    case = _case(gpu_ctx)
    L = _lib.lib()
    plan, pattern = case["plan"], case["pattern"]
    plh = pattern.ctypes.data_as(C.c_void_p)
    fr = _abi.FieldsRequest()
    lab = case["args"]["sample_label"].copy()
    lab[3] = 99
    pi = case["args"]["pool_index"].copy()
    pi[0] = -1
    wrong = list(case["blocks"])                                 # haps[5] no longer enumerates the plan's haplotypes
    wrong[5] = [dict(b, alleles=list(b["alleles"])) for b in wrong[5]]
    wrong[5][1]["alleles"].append(wrong[5][1]["alleles"][0] + b"ACG")
    kw = dict(sample_filtered=case["filt"], prune=True, want_read_ll=True)

    def both(call, text):
        """call(locus_haploid pointer or None) -> rc with *out; the same status and message either way"""
        seen = []
        for ptr in (None, plh):
            h = C.c_void_p(0x1234)
            rc = call(ptr, h)
            msg = L.ltr_last_error(gpu_ctx._h).decode()
            assert rc == _abi.LTR_ERR_INVALID and not h.value and text in msg, (rc, h.value, msg)
            seen.append(msg)
        assert seen[0] == seen[1]

    for bad, text in ((dict(sample_label=lab), "out of range"), (dict(pool_index=pi), "out of range")):
        packed = plan.pack_genotype(case["blocks"], **kw, **dict(case["args"], **bad))
        both(lambda ptr, h: L.ltr_plan_genotype_ploidy(plan._h, C.byref(packed["gb"]), C.byref(fr), ptr, C.byref(h)), text)
        both(lambda ptr, h: L.ltr_plan_genotype_ploidy(plan._h, C.byref(packed["gb"]), None, ptr, C.byref(h)), text)
    packed = plan.pack_genotype(wrong, **kw, **case["args"])
    both(lambda ptr, h: L.ltr_plan_genotype_ploidy(plan._h, C.byref(packed["gb"]), C.byref(fr), ptr, C.byref(h)), "do not enumerate the plan's")
    short = plan.pack_genotype(case["blocks"][:-1], **kw, **dict(case["args"], n_samples=case["args"]["n_samples"][:-1],
                                                                 locus_read_off=case["args"]["locus_read_off"][:-1]))
    both(lambda ptr, h: L.ltr_plan_genotype_ploidy(plan._h, C.byref(short["gb"]), None, ptr, C.byref(h)), "number of loci")
    lp = gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], wrong, sample_filtered=case["filt"], **case["largs"])
    both(lambda ptr, h: L.ltr_ll_genotype_ploidy(gpu_ctx._h, C.byref(lp["lb"]), C.byref(lp["gb"]), None, ptr, C.byref(h)), "locus 5")
    lp = gpu_ctx.pack_ll_genotype(case["mats"], case["seeds"], case["blocks"], sample_filtered=case["filt"], **dict(case["largs"], sample_label=lab))
    both(lambda ptr, h: L.ltr_ll_genotype_ploidy(gpu_ctx._h, C.byref(lp["lb"]), C.byref(lp["gb"]), C.byref(fr), ptr, C.byref(h)), "out of range")
    with pytest.raises(_lib.LtrError):                           # the binding wants one entry per locus
        plan.genotype(case["blocks"], locus_haploid=pattern[:-1], **case["args"])
    # and the plan and the context are still good
    got = plan.genotype(case["blocks"], want_read_ll=True, sample_filtered=case["filt"], locus_haploid=pattern, **case["args"])
    refs = {p: _plan_uniform(gpu_ctx, p, 1) for p in (0, 1)}
    for l, p in enumerate(pattern):
        _same_locus(got[l], refs[int(p)]["genotype"][l], l)


def test_release_the_module_plan(gpu_ctx):
    """(last in the file: the plan and the score buffer the cases above share go back)"""
    case = _CACHE.pop("case", None)
    _CACHE.clear()
    if case:
        case["plan"].close()
        assert case["hip"].hipFree(case["d_out"]) == 0
