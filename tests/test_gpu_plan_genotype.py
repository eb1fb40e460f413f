"""-m gpu: ltr_plan_genotype (posteriors -> uncalled alleles pruned once -> posteriors over the surviving haplotypes, every
locus of a resident plan) through the C-ABI: bit for bit against the composition of the library's existing entry points
(ltr_plan_posteriors, ltr_unused_alleles, ltr_remap_haplotypes, ltr_remap_aln_probs, ltr_posteriors), and against the CPU
restatements in oracle/ (genotyper.cpp / seq_stutter_genotyper.cpp themselves cannot be compiled here: htslib)."""
import importlib.util
import os

import numpy as np
import pytest

import genotype_util as gt
import oracle_lib as ol
from longtr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 91          # chosen on the CPU (oracle DP + oracle chain): 49 % / 68 % of the loci lose an allele (diploid / haploid), 39 / 48
#                    lose alleles in two blocks, one locus (0.5 %) has a sample whose two best diplotypes lie within 1e-6


def _plan(ctx, loci):
    batch, args = gt.pack(loci)
    plan = ctx.plan(batch)
    plan.execute()
    ll, _ = plan.fetch()
    return plan, batch, args, ll


def _first_pass(plan, args, loci, haploid):
    post, off, stl, gts = plan.posteriors(haploid=haploid, **args)
    out, u = [], 0
    for L in loci:
        S, H = L["S"], len(L["haps"])
        out.append(dict(post=post[off[u]:off[u + S]].reshape(S, H, H).copy(), sample_total_ll=stl[u:u + S].copy(), gts=gts[u:u + S].copy()))
        u += S
    return out


def _filtered(loci):
    return np.concatenate([L["filt"] for L in loci])


def _assert_same_bits(got, want, l):
    assert got["n_haps"] == want["post"].shape[1], l
    assert got["removed"] == want["removed"], l
    assert np.array_equal(got["new_to_old"], want["new_to_old"]) and np.array_equal(got["allele_mapping"], want["allele_mapping"]), l
    assert np.array_equal(got["gts"], want["gts"]), l
    assert np.array_equal(gt.bits(got["post"]), gt.bits(want["post"])), l
    assert np.array_equal(gt.bits(got["sample_total_ll"]), gt.bits(want["sample_total_ll"])), l
    assert np.array_equal(gt.bits(got["read_ll"]), gt.bits(want["read_ll"])), l
    assert [b["alleles"] for b in got["blocks"]] == [b["alleles"] for b in want["blocks"]], l
    assert got["num_aff_blocks"] == sum(1 for r in want["removed"] if r) and got["num_aff_alleles"] == sum(len(r) for r in want["removed"]), l


@pytest.mark.parametrize("haploid", [False, True])
def test_plan_genotype_equals_the_composed_entry_points_and_the_restatement(gpu_ctx, haploid):
    loci = gt.make_case(SEED)
    assert len(loci) >= 200 and min(len(L["haps"]) for L in loci) == 2 and max(len(L["haps"]) for L in loci) >= 12
    assert {L["S"] for L in loci} == set(range(1, 7)) and any(len(L["blocks"][0]["alleles"]) > 1 for L in loci)
    plan, batch, args, ll = _plan(gpu_ctx, loci)
    assert (ll < -600.0).any()
    got = plan.genotype([L["blocks"] for L in loci], haploid=haploid, sample_filtered=_filtered(loci), **args)
    first = _first_pass(plan, args, loci, haploid)
    assert len(got) == len(loci)
    oracle, left_out, unpruned, compared = [], 0, 0, 0
    for l, L in enumerate(loci):
        M = gt.per_read(batch, ll, l, L)
        # 1. bit for bit against the composition of the existing entry points: every locus, no exclusions
        want = gt.product_chain(gpu_ctx, L, M, first[l], haploid)
        _assert_same_bits(got[l], want, l)
        if not any(want["removed"]):                             # nothing to prune: the first pass's bits
            unpruned += 1
            assert np.array_equal(gt.bits(got[l]["post"]), gt.bits(first[l]["post"])), l
        # 2. against the CPU restatement
        o = gt.oracle_chain(L, M, haploid)
        oracle.append(o)
        # A near tie of the FIRST posteriors may change which alleles go (set equality left out for that locus); one of the
        # final posteriors may only change the final pair.  Posteriors and totals are compared wherever the removed sets agree.
        tie1, tie2 = gt.near_tie(L, o["first"]["post"]), gt.near_tie(L, o["post"])
        if tie1:
            left_out += 1                                        # (device libm differs from glibc in the last ulps)
        else:
            assert got[l]["removed"] == o["removed"], l
            if not tie2:
                assert np.array_equal(got[l]["gts"], o["gts"]), l
        if got[l]["removed"] == o["removed"]:
            compared += 1
            assert np.allclose(got[l]["post"], o["post"], rtol=0, atol=1e-9), l
            assert np.allclose(got[l]["sample_total_ll"], o["sample_total_ll"], rtol=0, atol=1e-9), l
    assert compared >= len(loci) - left_out
    assert left_out <= 0.02 * len(loci), left_out
    # 3. the case really prunes (from the oracle's result)
    lose, none, two = gt.prune_stats(loci, oracle)
    assert lose >= 0.25 and none >= 0.25 and two >= 1, (lose, none, two)
    assert unpruned >= 0.2 * len(loci)
    plan.close()


def test_prune_off_returns_the_first_posteriors(gpu_ctx):
    """prune = 0, the --ref-vcf mode (seq_stutter_genotyper.cpp:636): exactly ltr_plan_posteriors' bits, every locus."""
    loci = gt.make_case(SEED + 1, n_loci=60)
    plan, batch, args, ll = _plan(gpu_ctx, loci)
    for haploid in (False, True):
        got = plan.genotype([L["blocks"] for L in loci], haploid=haploid, sample_filtered=_filtered(loci), prune=False, **args)
        first = _first_pass(plan, args, loci, haploid)
        for l, L in enumerate(loci):
            H = len(L["haps"])
            assert got[l]["n_haps"] == H and not any(got[l]["removed"]) and got[l]["num_aff_alleles"] == 0
            assert np.array_equal(got[l]["new_to_old"], np.arange(H)) and got[l]["blocks"] == L["blocks"]
            assert np.array_equal(gt.bits(got[l]["post"]), gt.bits(first[l]["post"]))
            assert np.array_equal(gt.bits(got[l]["sample_total_ll"]), gt.bits(first[l]["sample_total_ll"]))
            assert np.array_equal(got[l]["gts"], first[l]["gts"])
            M = gt.per_read(batch, ll, l, L)
            assert np.array_equal(gt.bits(got[l]["read_ll"]), gt.bits(np.where(M < -600.0, -600.0, M)))
    got = plan.genotype([L["blocks"] for L in loci], prune=False, want_read_ll=False, **args)
    assert all(g["read_ll"] is None for g in got)
    plan.close()


def _big_locus(rng, nall, R, S, two_blocks, tr_len=60):
    L = synth.synth_locus(rng, tr_len, 3, nall, R, sub_rate=0.01, indel_rate=0.004, true_alleles=rng.choice(nall, size=min(nall, 6), replace=False))
    blocks = L.blocks()
    if two_blocks:
        f = bytearray(blocks[0]["alleles"][0])
        f[32] = ord("A") if f[32] != ord("A") else ord("C")
        blocks[0]["alleles"] = [blocks[0]["alleles"][0], bytes(f)]
    pools, pidx = synth.pool_reads(L.trimmed_reads)
    lab = rng.integers(0, S, size=R).astype(np.int32)
    return dict(blocks=blocks, haps=gt.gray_seqs(blocks), pools=pools, pool_index=np.asarray(pidx, dtype=np.int32), S=S, lab=lab,
                p1=-rng.random(R) * 0.01, p2=-rng.random(R) * 0.01, filt=np.zeros(S, dtype=np.uint8))


def test_tiles_and_large_haplotype_sets(gpu_ctx):
    """The shapes the kernel splits: (a) one sample with 2 200 reads over 18 haplotypes -- the reads pass through LDS in many
    tiles; (b) 20 haplotypes: 400 diplotypes for 256 threads; (c) 48 haplotypes: the 2 304-entry matrix is accumulated in the
    posterior buffer and normalised by the second kernel; (d) 1 056 haplotypes: a row wider than a tile.  All bit-identical to
    the composition, pruned and not."""
    rng = np.random.default_rng(93)
    loci = [_big_locus(rng, 9, 2200, 1, True), _big_locus(rng, 20, 40, 2, False), _big_locus(rng, 24, 30, 2, True),
            _big_locus(rng, 33, 6, 1, False, tr_len=120)]
    b = bytearray(loci[3]["blocks"][2]["alleles"][0])            # 33 x 32 haplotypes: the right flank gets 31 alternates
    alts = []
    for k in range(31):
        f = bytearray(b)
        f[6 + k % 24] = ord("ACGT"[(("ACGT".index(chr(b[6 + k % 24])) + 1 + k // 24) % 4)])
        alts.append(bytes(f))
    loci[3]["blocks"][2]["alleles"] = [bytes(b)] + alts
    loci[3]["haps"] = gt.gray_seqs(loci[3]["blocks"])
    assert len(set(loci[3]["haps"])) == 1056
    assert len(loci[0]["haps"]) >= 16 and np.bincount(loci[0]["lab"]).max() >= 2000 and len(loci[1]["haps"]) ** 2 > 256
    plan, batch, args, ll = _plan(gpu_ctx, loci)
    for prune in (True, False):
        got = plan.genotype([L["blocks"] for L in loci], prune=prune, **args)
        first = _first_pass(plan, args, loci, False)
        for l, L in enumerate(loci):
            _assert_same_bits(got[l], gt.product_chain(gpu_ctx, L, gt.per_read(batch, ll, l, L), first[l], False, prune), l)
    plan.close()


def test_aligned_read_comes_from_the_plans_seed_positions(gpu_ctx):
    """A plan built with realign_read masks leaves seed -1 for the masked pools (HapAligner.cpp:557-560): a sample all of whose
    reads are masked has no aligned read (seq_stutter_genotyper.cpp:262-266) and its best pair keeps no allele alive."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")                               # (the runtime the library itself runs on: a zeroed score buffer of our own)
    loci = gt.make_case(SEED + 3, n_loci=40)
    mask = []
    for l, L in enumerate(loci):
        keep = np.ones(len(L["pools"]), dtype=np.uint8)
        if l % 2 == 0 and L["S"] > 1:                            # every pool that holds a read of sample 0 is masked out
            keep[np.unique(L["pool_index"][L["lab"] == 0])] = 0
        mask.append(keep)
    batch, args = gt.pack(loci)
    batch = _abi.PackedBatch([(L["pools"], L["haps"]) for L in loci], realign_read=np.concatenate(mask))
    plan = gpu_ctx.plan(batch)
    nbytes = max(plan.ll_size, 1) * 8
    d_out = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_out), C.c_size_t(nbytes)) == 0
    init, at = np.full(max(plan.ll_size, 1), -50.0), 0           # masked rows are not written: they keep these scores, which
    for L in loci:                                               # make the last haplotype the masked sample's best pair
        P, H = len(L["pools"]), len(L["haps"])
        init[at:at + P * H].reshape(P, H)[:, H - 1] = 0.0
        at += P * H
    assert hip.hipMemcpy(d_out, C.c_void_p(init.ctypes.data), C.c_size_t(nbytes), 1) == 0 and hip.hipDeviceSynchronize() == 0
    plan.execute(d_out_ptr=d_out)
    plan.wait()
    _, seeds = plan.fetch()
    ll = np.zeros(max(plan.ll_size, 1))
    assert hip.hipMemcpy(C.c_void_p(ll.ctypes.data), d_out, C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
    assert (seeds < 0).any()
    first = _first_pass(plan, args, loci, False)
    got = plan.genotype([L["blocks"] for L in loci], sample_filtered=_filtered(loci), **args)
    differs = 0
    for l, L in enumerate(loci):
        r0 = int(batch.locus_read_off[l])
        M = gt.per_read(batch, ll, l, L)
        want = gt.product_chain(gpu_ctx, dict(L, seeds=seeds[r0:r0 + len(L["pools"])]), M, first[l], False)
        _assert_same_bits(got[l], want, l)
        differs += want["removed"] != gt.product_chain(gpu_ctx, L, M, first[l], False)["removed"]
    assert differs >= 1                                          # the seeds did decide something
    plan.close()
    assert hip.hipFree(d_out) == 0


def test_errors_launch_nothing(gpu_ctx):
    loci = gt.make_case(SEED + 2, n_loci=6)
    batch, args = gt.pack(loci)
    plan = gpu_ctx.plan(batch)
    blocks = [L["blocks"] for L in loci]

    def fails(text, blocks=blocks, **over):
        with pytest.raises(_lib.LtrError) as e:
            plan.genotype(blocks, **dict(args, **over))
        assert e.value.code == _abi.LTR_ERR_INVALID and text in str(e.value), str(e.value)

    fails("execute the plan first")
    plan.execute()
    wrong = [b for b in blocks]
    wrong[2] = [dict(b, alleles=list(b["alleles"])) for b in blocks[2]]
    wrong[2][1]["alleles"].append(wrong[2][1]["alleles"][0] + b"ACG")
    fails("do not enumerate the plan's", blocks=wrong)
    lab = args["sample_label"].copy()
    lab[3] = 99
    fails("out of range", sample_label=lab)
    pi = args["pool_index"].copy()
    pi[0] = -1
    fails("out of range", pool_index=pi)
    fails("number of loci", blocks=blocks[:-1], n_samples=args["n_samples"][:-1], locus_read_off=args["locus_read_off"][:-1])
    assert len(plan.genotype(blocks, **args)) == len(loci)       # and the plan is still good
    plan.close()


def test_real_reads_pruned_records(gpu_ctx, tmp_path):
    """examples/real_reads_trio.run(prune=True) on the bundled trio: no ALT allele without a carrier, the calls of the unpruned
    run (by allele length), Mendelian consistency kept, and the record of the pruned state equal to the restatement's."""
    spec = importlib.util.spec_from_file_location("real_reads_trio", os.path.join(ROOT, "examples", "real_reads_trio.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    base = [l for l in ex.run(gpu_ctx, tmp_dir=str(tmp_path)) if l["status"] == "ok"]
    pruned = [l for l in ex.run(gpu_ctx, str(tmp_path / "pruned.vcf"), tmp_dir=str(tmp_path), prune=True) if l["status"] == "ok"]
    assert len(base) == len(pruned) and len(pruned) >= 5
    mendel = lambda g: any((g[0][0] in a and g[0][1] in b) for a, b in ((g[1], g[2]), (g[2], g[1])))
    lost = 0
    for b, p in zip(base, pruned):
        name = p["region"]["name"]
        assert p["gt_lens"] == b["gt_lens"], (name, p["gt_lens"], b["gt_lens"])
        if mendel(b["gt_lens"]):
            assert mendel(p["gt_lens"]), name
        cols = p["vcf_line"].split("\t")
        alts = [] if cols[4] == "." else cols[4].split(",")
        carried = {int(a) for c in cols[9:] for a in c.split(":")[0].replace("/", "|").split("|") if a != "."}
        assert set(range(1, len(alts) + 1)) <= carried, (name, cols[4], [c.split(":")[0] for c in cols[9:]])
        assert p["vcf_line"] == ol.oracle_vcf_record(p["vcf_locus"])[0], name
        lost += sum(len(r) for r in p["removed"])
        assert len(p["blocks"][1]["alleles"]) == len(b["blocks"][1]["alleles"]) - len(p["removed"][1])
    assert lost > 0                                              # the run did prune something
