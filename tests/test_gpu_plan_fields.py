"""-m gpu: ltr_plan_genotype_fields -- the passes of ltr_plan_genotype and then, on the posterior blocks where they lie on the
device, what write_vcf_record computes before it prints (ltr_genotype_fields_kernel, ltr_plan_fields.hip) -- and
ltr_genotype_result_vcf_records.  The reference for the fields is ltr_vcf_fields (host) fed with the SAME result's posterior
and per-read bits, so only the device's libm differs from glibc:
  exact          best_gts, n_aligned, n_snp, n_s1, n_s2, read_allele, hap_log_phased (a copy)
  atol 1e-9      log_phased, log_unphased, phased_gls: device exp / log against glibc (the bound of test_gpu_plan_genotype.py
                 and test_gpu_host_path.py for the same functions)
  atol 1e-3      hap_log_unphased, gls: through the FP32 fast_log_sum_exp, whose bit tricks have kinks of that size
                 (the bound of test_gpu_host_path.py for the same approximation)
  bit-identical  gl_diffs, pls against calc_gl_diff / calc_PLs applied to the DEVICE's own gls and best_gts (no libm).
PL is an integer truncation of a GL known to 1e-3 only, so the record comparison with the parent path runs with PL off."""
import importlib.util
import os

import numpy as np
import pytest

import genotype_util as gt
import vcf_fields_util as vu
from longtr_amd import _abi, _lib
from test_gpu_plan_genotype import SEED, _big_locus, _filtered, _plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_KEYS = {"Q", "PQ", "GLDIFF", "GL", "PHASEDGL", "HQ", "PHQ"}
ALL_OPT = dict(output_gls=1, output_phased_gls=1, output_filters=1, output_haplotype_data=1)


def _big_loci():
    """The four shapes of test_tiles_and_large_haplotype_sets; then a repeat block of 48 alleles (a 2 304-entry V x V table: beyond
    the 2 048 doubles kept in LDS, so it lives in the kernel's global workspace) between two small loci, so that one call holds
    units of both workgroup sizes, with and without a workspace slot."""
    rng = np.random.default_rng(93)
    loci = [_big_locus(rng, 9, 2200, 1, True), _big_locus(rng, 20, 40, 2, False), _big_locus(rng, 24, 30, 2, True),
            _big_locus(rng, 33, 6, 1, False, tr_len=120)]
    small = gt.make_case(SEED + 5, n_loci=2)
    wide = _big_locus(rng, 48, 60, 3, False, tr_len=150)
    assert len(wide["blocks"][1]["alleles"]) ** 2 > 2048 and len(small[0]["haps"]) <= 8
    tail = [small[0], wide, small[1]]
    b = bytearray(loci[3]["blocks"][2]["alleles"][0])
    alts = []
    for k in range(31):
        f = bytearray(b)
        f[6 + k % 24] = ord("ACGT"[(("ACGT".index(chr(b[6 + k % 24])) + 1 + k // 24) % 4)])
        alts.append(bytes(f))
    loci[3]["blocks"][2]["alleles"] = [bytes(b)] + alts
    loci[3]["haps"] = gt.gray_seqs(loci[3]["blocks"])
    assert len(set(loci[3]["haps"])) == 1056
    return loci + tail


def _describe(l, L, g, haploid, rng):
    """The ltr_vcf_locus of locus l around the final state g (a Plan.genotype dict)."""
    blocks = g["blocks"]
    s0 = blocks[1]["start"]
    S = L["S"]
    return dict(chrom="chr3", region_start=s0 + 5, region_stop=blocks[1]["end"] - 5, name="L%d" % l, motif="ACG", period_str="3",
                chrom_seq=bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=600)), chrom_seq_start=s0 - 300, blocks=blocks, block=1,
                log_aln_probs=g["read_ll"] if g["read_ll"] is not None else np.zeros((len(L["lab"]), g["n_haps"])), log_p1=L["p1"], log_p2=L["p2"],
                sample_label=L["lab"], alns=None, log_sample_posteriors=g["post"] if g["post"] is not None else np.zeros((S, 1, 1)),
                sample_total_ll=g["sample_total_ll"], best_haplotypes=g["gts"], n_p1s=np.arange(S), n_p2s=np.arange(S)[::-1].copy(),
                sample_names=["S%d" % s for s in range(S)], sample_filter=["LOW" if x else "" for x in L["filt"]], haploid=haploid)


def _same_bits_as_parent(got, want, l):
    for k in ("n_haps", "removed", "num_aff_blocks", "num_aff_alleles"):
        assert got[k] == want[k], (l, k)
    for k in ("new_to_old", "allele_mapping", "gts"):
        assert np.array_equal(got[k], want[k]), (l, k)
    for k in ("post", "sample_total_ll", "read_ll"):
        assert np.array_equal(vu.bits(got[k]), vu.bits(want[k])), (l, k)
    assert [b["alleles"] for b in got["blocks"]] == [b["alleles"] for b in want["blocks"]], l


def _check_fields(dev, host, n_haps, haploid, l, worst):
    assert all(dev[k] == host[k] for k in ("S", "R", "V", "block", "n_gl", "n_pgl")), l
    for k in vu.EXACT:
        assert np.array_equal(dev[k], host[k]), (l, k)
    assert np.array_equal(vu.bits(dev["hap_log_phased"]), vu.bits(host["hap_log_phased"])), l
    for k, tol in (("log_phased", 1e-9), ("log_unphased", 1e-9), ("phased_gls", 1e-9), ("hap_log_unphased", 1e-3), ("gls", 1e-3)):
        d = np.abs(dev[k] - host[k])
        d = d[np.isfinite(d)]
        worst[k] = max(worst.get(k, 0.0), float(d.max()) if d.size else 0.0)
        assert np.allclose(dev[k], host[k], rtol=0, atol=tol, equal_nan=True), (l, k, worst[k])
    vu.check_self_consistent(dev, n_haps, haploid)


def _tokens_agree(new, old, l):
    a, b = new.split("\t"), old.split("\t")
    assert a[:9] == b[:9] and len(a) == len(b), (l, new, old)
    keys = a[8].split(":")
    for ca, cb in zip(a[9:], b[9:]):
        fa, fb = ca.split(":"), cb.split(":")
        assert len(fa) == len(fb), (l, ca, cb)
        if len(fa) != len(keys):                                 # "." : no call
            assert ca == cb, (l, ca, cb)
            continue
        for k, x, y in zip(keys, fa, fb):
            if k in FLOAT_KEYS and x != y:
                assert len(x.split(",")) == len(y.split(",")), (l, k, x, y)
                for p, q in zip(x.split(","), y.split(",")):
                    assert abs(float(p) - float(q)) <= 0.01 + 1e-9, (l, k, x, y)
            elif k not in FLOAT_KEYS:
                assert x == y, (l, k, x, y)


def _run(gpu_ctx, loci, haploid, prune, report):
    plan, batch, args, ll = _plan(gpu_ctx, loci)
    blocks = [L["blocks"] for L in loci]
    kw = dict(haploid=haploid, sample_filtered=_filtered(loci), prune=prune, **args)
    parent = plan.genotype(blocks, want_read_ll=True, **kw)
    rng = np.random.default_rng(7)
    opt = _abi.vcf_options(**ALL_OPT)
    worst = {}
    with plan.genotype_fields(blocks, want_read_ll=True, want_gls=True, want_pls=True, want_phased_gls=True, want_posteriors=True, **kw) as res:
        assert res.n_loci == len(loci)
        full, packed, host = [], [], []
        for l, L in enumerate(loci):
            g = res.locus(l)
            _same_bits_as_parent(g, parent[l], l)                 # 5. the bits of ltr_plan_genotype
            pv = _abi.PackedVcfLocus(_describe(l, L, g, haploid, rng))
            f, h = res.fields(l), _lib.vcf_fields(pv)
            _check_fields(f, h, g["n_haps"], haploid, l, worst)   # 6.
            full.append(f); packed.append(pv); host.append(h)
            report["max_VV"] = max(report.get("max_VV", 0), f["V"] ** 2)
        # 8. the records of the whole result: the per-locus formatter on the same fields, whatever the thread budget
        every = _abi.vcf_options(output_pls=1, **ALL_OPT)        # (every switch on: PL from the device's pls too)
        want = [_lib.vcf_record_from_fields(packed[l], full[l], every) for l in range(len(loci))]
        for budget in (2, 16):
            gpu_ctx.set_host_threads(budget)
            lines, pos = res.vcf_records(packed, every)
            assert lines == [w[0] for w in want] and pos.tolist() == [w[1] for w in want], budget
            assert ":PL:" in lines[0].split("\t")[8] + ":"
        gpu_ctx.set_host_threads(0)                              # back to the rule
        lines, pos = res.vcf_records(packed, opt)
        same = 0
        for l in range(len(loci)):                               # ... and the parent path: ltr_vcf_record on the downloaded matrices
            old = _lib.vcf_record(packed[l], opt)[0]
            _tokens_agree(lines[l], old, l)
            same += lines[l] == old
        report["identical_lines"] = report.get("identical_lines", 0) + same
        report["lines"] = report.get("lines", 0) + len(loci)
    # 7. nothing but the fields downloaded
    with plan.genotype_fields(blocks, want_read_ll=False, want_gls=True, want_pls=True, want_phased_gls=True, want_posteriors=False, **kw) as res:
        for l in range(len(loci)):
            g = res.locus(l)
            assert g["post"] is None and g["read_ll"] is None
            assert np.array_equal(g["gts"], parent[l]["gts"]) and np.array_equal(vu.bits(g["sample_total_ll"]), vu.bits(parent[l]["sample_total_ll"]))
            f = res.fields(l)
            for k in vu.ARRAYS:
                same = np.array_equal(vu.bits(f[k]), vu.bits(full[l][k])) if f[k].dtype == np.float64 else np.array_equal(f[k], full[l][k])
                assert same, (l, k)
    with plan.genotype_fields(blocks, **kw) as res:              # the switches drop the arrays, nothing else
        f = res.fields(0)
        assert f["gls"] is None and f["pls"] is None and f["phased_gls"] is None
        assert np.array_equal(vu.bits(f["gl_diffs"]), vu.bits(full[0]["gl_diffs"]))
    plan.close()
    for k, v in worst.items():
        report[k] = max(report.get(k, 0.0), v)


@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("prune", [True, False])
def test_fields_of_a_plan(gpu_ctx, haploid, prune):
    loci = gt.make_case(SEED)
    assert len(loci) >= 200 and max(len(L["haps"]) for L in loci) >= 12 and {L["S"] for L in loci} == set(range(1, 7))
    report = {}
    _run(gpu_ctx, loci, haploid, prune, report)
    print("plan fields, haploid=%s prune=%s: largest differences %s" % (haploid, prune, report))


@pytest.mark.parametrize("haploid", [False, True])
@pytest.mark.parametrize("prune", [True, False])
def test_fields_of_large_shapes(gpu_ctx, haploid, prune):
    """2 200 reads in one sample, 400 and 2 304 diplotypes, 1 056 haplotypes; and 48 alleles in the reported block, whose V x V table
    goes through the global workspace when nothing is pruned (pruning leaves at most two alleles per sample, so a pruned locus
    of three samples never needs it: the workspace runs in the prune=False cases, diploid and haploid)."""
    report = {}
    loci = _big_loci()
    _run(gpu_ctx, loci, haploid, prune, report)
    assert prune or report["max_VV"] > 2048                      # the workspace branch ran
    print("large shapes, haploid=%s prune=%s: largest differences %s" % (haploid, prune, report))


def test_other_blocks_and_errors_launch_nothing(gpu_ctx):
    loci = gt.make_case(SEED + 2, n_loci=12)
    batch, args = gt.pack(loci)
    plan = gpu_ctx.plan(batch)
    blocks = [L["blocks"] for L in loci]
    L = _lib.lib()

    def fails(text, blocks=blocks, **over):
        with pytest.raises(_lib.LtrError) as e:
            plan.genotype_fields(blocks, **dict(args, **over))
        assert e.value.code == _abi.LTR_ERR_INVALID and text in str(e.value), str(e.value)

    fails("execute the plan first")
    plan.execute()
    fails("block out of range", block=[1] * 5 + [3] + [1] * 6)
    fails("block out of range", block=[1] * 5 + [-1] + [1] * 6)
    lab = args["sample_label"].copy()
    lab[3] = 99
    fails("out of range", sample_label=lab)
    packed = plan.pack_genotype(blocks, prune=False, **args)     # gb->haps NULL: fine for ltr_plan_genotype without pruning, not here
    packed["gb"].haps = None
    assert plan.genotype_packed(packed, decode=False) is None
    import ctypes as C
    h, fr = C.c_void_p(0x1234), _abi.FieldsRequest()
    assert L.ltr_plan_genotype_fields(plan._h, C.byref(packed["gb"]), C.byref(fr), C.byref(h)) == _abi.LTR_ERR_INVALID and not h.value
    assert b"no haplotype blocks" in L.ltr_last_error(gpu_ctx._h)
    h = C.c_void_p(0x1234)
    assert L.ltr_plan_genotype_fields(plan._h, C.byref(packed["gb"]), None, C.byref(h)) == _abi.LTR_ERR_INVALID and not h.value
    # a result of ltr_plan_genotype has no fields; the fields of another block of a two-block locus
    with plan.genotype_fields(blocks, block=[0] * len(loci), want_gls=True, want_read_ll=True, want_posteriors=True, **args) as res:
        for l, Lc in enumerate(loci):
            g, f = res.locus(l), res.fields(l)
            assert f["block"] == 0 and f["V"] == len(g["blocks"][0]["alleles"])
            d = _describe(l, Lc, g, False, np.random.default_rng(1))
            d["block"] = 0
            h = _lib.vcf_fields(_abi.PackedVcfLocus(d))
            assert all(np.array_equal(f[k], h[k]) for k in vu.EXACT), l
        # a locus description that does not fit: the locus is named, nothing handed out
        pvs = [_abi.PackedVcfLocus(_describe(l, Lc, res.locus(l), False, np.random.default_rng(1))) for l, Lc in enumerate(loci)]
        pvs[4].struct.n_samples += 1
        with pytest.raises(_lib.LtrError) as e:
            res.vcf_records(pvs)
        assert e.value.code == _abi.LTR_ERR_INVALID and "locus 4" in str(e.value)
    plan.close()


def test_bundled_trio_with_device_fields(gpu_ctx, tmp_path):
    """examples/real_reads_trio.run(prune=True, device_fields=True): the columns of run(prune=True), floats within one unit of %.2f."""
    spec = importlib.util.spec_from_file_location("real_reads_trio", os.path.join(ROOT, "examples", "real_reads_trio.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    old = [l for l in ex.run(gpu_ctx, str(tmp_path / "old.vcf"), tmp_dir=str(tmp_path), prune=True) if l["status"] == "ok"]
    new = [l for l in ex.run(gpu_ctx, str(tmp_path / "new.vcf"), tmp_dir=str(tmp_path), prune=True, device_fields=True) if l["status"] == "ok"]
    assert len(old) == len(new) >= 5
    for a, b in zip(new, old):
        assert a["region"]["name"] == b["region"]["name"] and a["gt_lens"] == b["gt_lens"]
        _tokens_agree(a["vcf_line"], b["vcf_line"], a["region"]["name"])
    assert (tmp_path / "new.vcf").read_text().count("\n") == (tmp_path / "old.vcf").read_text().count("\n")
