"""-m gpu: many items per persistent wavefront.  Every DP kernel takes item after item -- a queue word, a static deal, a redo list --
and the crafted edge cases of the other GPU tests are small batches on a large device: each wavefront takes one item and leaves.
Here ltr_ctx_set_debug "grid_cap" holds every launch to one or two workgroups, so that an aborting pair, a failed stem, a non-ACGT
pair, a long pair at the -600 line is FOLLOWED by other items on the same wavefront or workgroup: what a kernel carries over from
one item to the next (LDS rings and flags, note slots, park blocks, boundary strips, trace regions) is then part of the result.
Every score is compared with the oracle bit for bit, and ltr_debug_last_launches shows that the grids really were capped."""
import numpy as np
import pytest

import oracle_lib as ol
from longtr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu

BLOCK_WAVES = 4                                                   # wavefronts per workgroup of the one-wave kernels (kBlockWaves)


def _bits(a):
    return np.asarray(a).view(np.uint64)


def _capped_launches(launches, cap):
    """The read-back of a run under `cap`: at least one launch, none above the cap."""
    assert launches and all(1 <= l["grid"] <= cap for l in launches), launches
    return launches


def _run_plan(ctx, batch, cap, knobs=(), mode=-1, executes=1):
    """One plan under the switches, `executes` times; (scores of every execute, launches of the last, kernel statistics, family
    statistics)."""
    try:
        ctx.set_pair_packing(mode)
        for k, v in dict(knobs).items():
            ctx.set_debug(k, v)
        ctx.set_debug("grid_cap", cap)
        plan = ctx.plan(batch)
        lls = []
        for _ in range(executes):
            plan.execute()
            lls.append(plan.fetch()[0].copy())
        launches = _lib.debug_last_launches(plan=plan)
        stats = plan.kernel_stats()
        fam = dict(plan.family_stats(), **plan.family_spine_stats())
        plan.close()
    finally:
        ctx.set_pair_packing(-1)
        ctx.set_debug("reset", 0)
    return lls, launches, stats, fam


# ---- a. the plan kernel, the multi-width launches, a launch per class -------------------------------------------------------------

@pytest.fixture(scope="module")
def schedule_batch_and_scores(gpu_ctx):
    import test_gpu_plan_schedule as tgs
    batch = tgs.schedule_batch(gpu_ctx.device_info()["n_cu"])
    return batch, ol.oracle_align_batch(batch, _abi.default_params())[0]


@pytest.mark.parametrize("schedule", ["plan kernel", "multi-width", "per class"])
def test_three_schedules_on_one_workgroup(gpu_ctx, schedule_batch_and_scores, schedule):
    import test_gpu_plan_schedule as tgs
    batch, ref = schedule_batch_and_scores
    (ll,), launches, _, _ = _run_plan(gpu_ctx, batch, 1, tgs.SCHEDULES[schedule])
    _capped_launches(launches, 1)
    kinds = {l["kind"] for l in launches}
    assert {"plan kernel": {"plan"}, "multi-width": {"multi", "packed"}, "per class": {"one-wave", "packed"}}[schedule] <= kinds, kinds
    assert "workgroup" in kinds or "threshold" in kinds
    # more items than takers: the launch that holds the filler pairs has thousands for its four wavefronts
    assert max(l["items"] / (l["grid"] * l["takers"]) for l in launches) > 100
    assert np.array_equal(_bits(ll), _bits(ref)), np.flatnonzero(_bits(ll) != _bits(ref))[:8]


# ---- b. edge pairs in sequence -----------------------------------------------------------------------------------------------------

def edge_pair_batch():
    """The pairs that abort or sit at the -600 line and the non-ACGT loci of tests/test_gpu_align.py, each followed by ordinary pairs
    of 40 .. 700 bases."""
    import test_gpu_align as tga
    rng = np.random.default_rng(41)
    edge = tga.hard_pairs() + tga.non_acgt_loci()
    ordinary = tga._near_pairs(rng, [int(m) for m in np.linspace(40, 700, 20)])
    loci = []
    for i in range(max(len(edge), len(ordinary))):
        loci += edge[i:i + 1] + ordinary[i:i + 1]
    return _abi.PackedBatch(loci)


EDGE_MODELS = {"default": None, "ont": synth.ONT_PARAMS, "asymmetric": (-1.5, -0.3, -0.8, -0.6, -0.0001, -7.5, -9.25)}


@pytest.fixture(scope="module")
def edge_pairs_and_scores():
    batch = edge_pair_batch()
    return batch, {name: ol.oracle_align_batch(batch, _abi.make_params(v) if v else _abi.default_params())[0] for name, v in EDGE_MODELS.items()}


@pytest.mark.parametrize("model", list(EDGE_MODELS))
def test_edge_pairs_between_ordinary_pairs(gpu_ctx, edge_pairs_and_scores, model):
    batch, refs = edge_pairs_and_scores
    ref = refs[model]
    try:
        if EDGE_MODELS[model]:
            gpu_ctx.set_params(_abi.make_params(EDGE_MODELS[model]))
        for mode in (-1, 0, 1, 4, 7):
            (ll,), launches, stats, _ = _run_plan(gpu_ctx, batch, 1, mode=mode)
            _capped_launches(launches, 1)
            assert np.array_equal(_bits(ll), _bits(ref)), (mode, np.flatnonzero(_bits(ll) != _bits(ref))[:8])
            assert _lib.Plan.exact_pairs(stats) >= 4, mode       # the exact bodies ran between ordinary pairs
            # many items per wavefront: the 40 non-ACGT pairs and more are scored by the four wavefronts of ONE workgroup (the plan
            # kernel's, in line, or the generic list's launch), and but for mode 4 some first-pass launch holds more pairs than wavefronts
            assert max(k["pairs"] for k in stats if k["family"] == "exact") >= 5 * BLOCK_WAVES, mode
            assert mode == 4 or any(l["items"] > l["grid"] * l["takers"] for l in launches if l["items"] >= 0), (mode, launches)
    finally:
        gpu_ctx.set_params(_abi.default_params())
    if model == "default":
        assert (ref == -700.0).sum() >= 4 and (ref > -600.0).sum() >= 30


# ---- c. the family kernel ----------------------------------------------------------------------------------------------------------

FAILURES = ("stem", "stream", "tails", "rule, plain", "rule, spine")


def family_loci():
    """(loci, {(locus, read): failure kind}): the crafted shapes of tests/test_gpu_families.py and tests/test_gpu_families_spine.py
    in one plan -- strip widths 6, 10, 11, 15, 20 with three park slots at both periods, the shapes of the CPU test, twelve members,
    and one family of each kind of failure.  Every (locus, read) not in the dict is a family whose members are all accepted."""
    import test_gpu_families as tgf
    import test_gpu_families_spine as tgs
    rng = np.random.default_rng(51)
    # (both edges of the narrow widths: cheap families, the last of the launch order -- every failing family has successors)
    cols = [c for c in tgs.EDGE_COLUMNS if c[0] in (321, 384, 577, 640, 641, 960, 1280)]
    assert [w for _, w in cols] == [6, 6, 10, 10, 11, 15, 20]
    edges, _ = tgs.edge_loci(rng, cols)
    shapes, _ = tgs.cpu_shape_loci(rng)
    twelve = tgf.two_and_twelve_loci(rng)
    failing = [("stem", tgf.stem_failure_locus(rng)), ("stream", tgs.failed_stream_locus(rng)[0]), ("tails", tgf.tail_failure_locus(rng)),
               ("rule, plain", tgf.rule_failure_locus(rng)), ("rule, spine", tgs.spine_rule_failure_locus(rng))]
    loci, kinds = [], {}
    clean = edges + shapes + twelve
    # a failing family between clean ones in the batch; the launch order is the library's (modelled cost), checked by the test
    step = len(clean) // len(failing)
    for i, locus in enumerate(clean):
        loci.append(locus)
        if i % step == step - 1 and i // step < len(failing):
            kind, bad = failing[i // step]
            kinds[(len(loci), 0)] = kind                         # (read 0 of each failing locus is the one that fails)
            loci.append(bad)
    assert len(kinds) == len(failing)
    return loci, kinds


def deal(n_families, cap):
    """ltr_dp_family_kernel's static deal: per wavefront of the capped grid the families it runs, in order -- wavefront w of G takes
    w, 2G - 1 - w, 2G + w, .."""
    G = cap * BLOCK_WAVES
    waves = [[] for _ in range(G)]
    for i in range(n_families):
        r, pos = divmod(i, G)
        waves[(G - 1 - pos) if r & 1 else pos].append(i)
    return waves


def family_kinds(batch, formed, kinds):
    """Per family in launch order: (its failure kind or None, runs along a spine)."""
    loc_off = np.concatenate([[0], np.cumsum(np.diff(batch.locus_read_off) * np.diff(batch.locus_hap_off))])
    out = []
    for f in formed["families"]:
        l = int(np.searchsorted(loc_off, f["out_idx"][0], side="right")) - 1
        n_haps = int(batch.locus_hap_off[l + 1] - batch.locus_hap_off[l])
        r = (f["out_idx"][0] - int(loc_off[l])) // n_haps
        assert all(int(loc_off[l]) + r * n_haps <= o < int(loc_off[l]) + (r + 1) * n_haps for o in f["out_idx"])
        out.append((kinds.get((l, r)), f["spine"] >= 0))
    return out


def check_family_sequences(what, cap):
    """Under `cap` every kind of failure is followed on its wavefront by a family whose members are all accepted, and some wavefront
    runs a plain family right after a spine family and the reverse."""
    seen, plain_after_spine, spine_after_plain = set(), False, False
    for wave in deal(len(what), cap):
        for a, b in zip(wave, wave[1:]):
            if what[a][0] is not None and what[b][0] is None:     # (the very next family of that wavefront)
                seen.add(what[a][0])
            plain_after_spine |= what[a][1] and not what[b][1]
            spine_after_plain |= not what[a][1] and what[b][1]
    assert seen == set(FAILURES), (cap, set(FAILURES) - seen)
    assert plain_after_spine and spine_after_plain, cap


FAMILY_KNOBS = dict(families=2, family_spine=1)


def test_family_launch_order_puts_failures_before_accepted_families():
    """The deal of the family test below at the CU count of an MI355X, from the host half of planning alone."""
    loci, kinds = family_loci()
    batch = _abi.PackedBatch(loci)
    formed = _lib.debug_plan_family_forks(batch, n_cu=256, **FAMILY_KNOBS)
    what = family_kinds(batch, formed, kinds)
    assert len(what) >= 24 and sorted(k for k, _ in what if k) == sorted(FAILURES)
    for cap in (1, 2):
        check_family_sequences(what, cap)



@pytest.fixture(scope="module")
def family_plan_and_scores():
    loci, kinds = family_loci()
    batch = _abi.PackedBatch(loci)
    return batch, kinds, ol.oracle_align_batch(batch, _abi.default_params())[0]


@pytest.mark.parametrize("cap", [1, 2])
def test_families_in_sequence_on_four_and_eight_wavefronts(gpu_ctx, family_plan_and_scores, cap):
    batch, kinds, ref = family_plan_and_scores
    formed = _lib.debug_plan_family_forks(batch, n_cu=gpu_ctx.device_info()["n_cu"], **FAMILY_KNOBS)
    what = family_kinds(batch, formed, kinds)
    assert len(what) >= 24 and len(what) > 2 * cap * BLOCK_WAVES    # three rounds and more: both directions of the snake
    check_family_sequences(what, cap)
    (free,), _, _, st_free = _run_plan(gpu_ctx, batch, 0, FAMILY_KNOBS)
    (off,), _, _, st_off = _run_plan(gpu_ctx, batch, cap, dict(families=-1))
    (ll, again), launches, _, st = _run_plan(gpu_ctx, batch, cap, FAMILY_KNOBS, executes=2)
    _capped_launches(launches, cap)
    (fam,) = [l for l in launches if l["kind"] == "family"]
    assert fam["grid"] == cap and fam["takers"] == BLOCK_WAVES and fam["items"] == len(what) == st["families"]
    assert st_off["families"] == 0
    for got, name in ((free, "no cap"), (off, "no families"), (ll, "capped"), (again, "second execute")):
        assert np.array_equal(_bits(got), _bits(ref)), (name, np.flatnonzero(_bits(got) != _bits(ref))[:8])
    assert st == st_free, (st, st_free)
    # one stem; the failed stream's two members and the two random tails; two members of the plain family, four of the spine family
    assert (st["stem_failures"], st["tail_failures"], st["rule_failures"]) == (1, 4, 6), st
    assert st["with_spine"] == formed["with_spine"] > 0


# ---- d. the workgroup kernels ------------------------------------------------------------------------------------------------------

def long_pairs_in_sequence():
    """The pairs of test_long_pairs_abort_uncertain_and_unequal_lengths without the two of 9000 bases (the rolling oracle's time),
    ordered so that in every class a pair that aborts or is uncertain is followed by one that finishes: each edge pair travels with a
    near pair of its own length."""
    import test_gpu_wg as tgw
    rng = np.random.default_rng(61)
    pairs = []
    for r, h in tgw.long_edge_pairs():
        if len(r) == 9000:
            continue
        pairs.append((r, h))
        if len(r) > 1281:
            pairs.append(tgw._near_pair(rng, len(r)))
    pairs.append(tgw._near_pair(rng, 6100))                       # the eight-wave class: three pairs and more on its one workgroup
    return pairs


@pytest.fixture(scope="module")
def long_pairs_and_scores():
    pairs = long_pairs_in_sequence()
    prm = _abi.default_params()
    return pairs, np.asarray([ol.oracle_align_long(h, r, prm, rolling=True) for r, h in pairs])


@pytest.mark.parametrize("first_pass", [1, 2])
def test_long_pairs_in_sequence_on_one_workgroup(gpu_ctx, long_pairs_and_scores, first_pass):
    pairs, want = long_pairs_and_scores
    batch = _abi.PackedBatch([([r], [h]) for r, h in pairs])
    assert (want == -700.0).sum() >= 6 and (want > -600.0).sum() >= 10
    for mode in (-1, 2):
        (ll,), launches, stats, _ = _run_plan(gpu_ctx, batch, 1, dict(wg_first_pass=first_pass), mode=mode)
        _capped_launches(launches, 1)
        assert np.array_equal(_bits(ll), _bits(want)), (mode, np.flatnonzero(_bits(ll) != _bits(want))[:8])
        wg = [l for l in launches if l["kind"] == ("workgroup" if first_pass == 1 else "threshold")]
        assert wg and all(l["takers"] == 1 for l in wg)
        busy = {lanes: max([k["pairs"] for k in stats if k["family"] == "workgroup" and k["lanes_per_pair"] == lanes] or [0]) for lanes in (256, 512)}
        assert busy[256] >= 3 and busy[512] >= 3, (mode, busy)
        if first_pass == 1:
            assert _lib.Plan.exact_pairs(stats) >= 6, mode       # the pairs that abort or are uncertain: through the exact lists
            assert any(l["kind"] == "exact" for l in launches)


# ---- e. haplotype-to-reference Needleman-Wunsch ------------------------------------------------------------------------------------

def test_nw_classes_on_one_workgroup(gpu_ctx):
    import test_nw_hap_to_ref as tnw
    loci, _ = tnw.restatement_loci()
    try:
        gpu_ctx.set_debug("grid_cap", 1)
        got = gpu_ctx.haplotype_align_to_ref([L.blocks() for L in loci])
        launches = _lib.debug_last_launches(ctx=gpu_ctx)
    finally:
        gpu_ctx.set_debug("reset", 0)
    _capped_launches(launches, 1)
    assert sorted(l["cls"] for l in launches) == list(range(6)), launches     # strip widths 4 .. 20 and the workgroup kernel
    for l in launches:
        assert (l["kind"], l["takers"]) == (("nw-wave", BLOCK_WAVES) if l["cls"] < 5 else ("nw-workgroup", 1))
        assert l["items"] > l["grid"] * l["takers"], l            # more tasks than wavefronts (workgroups)
    n = 0
    for L, infos in zip(loci, got):
        haps = L.haplotypes
        assert len(infos) == len(haps)
        for h, info in zip(haps, infos):
            assert info == ol.oracle_nw_aln_info(haps[0], h, L.start, L.start + len(L.lflank)), (len(haps[0]), len(h))
            n += 1
    assert n == sum(l["items"] for l in launches)
