"""The three schedules of a plan (the plan kernel; the multi-width launches; a launch per class) at every timing level on ONE small
batch that reaches every kind of launch: same scores, same totals in the per-class reports, every launch timed under the class it
is listed under.  The shapes the batch has to reach are checked on the CPU first (ltr_debug_plan_schedule)."""
import numpy as np
import pytest

from longtr_amd import _abi, _lib

SCHEDULES = {"plan kernel": dict(), "multi-width": dict(plan_kernel=1, no_multi=-1), "per class": dict(plan_kernel=1, no_multi=1)}


def schedule_batch(n_cu=256):
    """About 40 small loci.  Automatic mode packs short reads only from 32 pairs per CU up, and then every read of up to 640 columns:
    thirty filler loci of 41-base reads make the batch that large, and the one-wave widths below 11 are held by shortcut pairs
    (reads of 300 and 500 bases against a 40-base haplotype: constant score, the one-wave class of their length)."""
    rng = np.random.default_rng(2026)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))

    def locus(m, n_reads, n_haps, stranger=False):
        core = seq(m)
        haps = [seq(30) + core + seq(30)] + [seq(30) + core[:m // 2] + seq(5 + h) + core[m // 2:] + seq(30) for h in range(n_haps - 1)]
        reads = []
        for _ in range(n_reads):
            r = bytearray(core)
            for p in rng.choice(m, size=3, replace=False):
                r[p] = ord("A") if r[p] != ord("A") else ord("C")
            reads.append(bytes(r))
        if stranger:
            reads.append(seq(m))                                # matches nothing: its certificate fails, an exact body scores it
        return reads, haps

    loci = [locus(1201, 2, 2), locus(801, 2, 2, stranger=True)]           # one-wave W = 19, 13
    loci += [([seq(301), seq(301)], [seq(40), seq(40)]), ([seq(501), seq(501)], [seq(40)])]       # shortcuts: one-wave W = 5, 8 (too far from the next width with pairs to be folded into it)
    loci += [locus(601, 2, 2, stranger=True)]                              # packed, 32 lanes x 19
    loci += [locus(1401, 1, 2), locus(2701, 1, 1)]                         # four-wave workgroups (1401: beside the plan kernel two column blocks on one wave)
    n_read = locus(201, 2, 2)
    n_read[0][0] = n_read[0][0][:7] + b"N" + n_read[0][0][8:]              # a byte outside ACGT: starts out in the generic exact list
    loci += [n_read]
    per_filler = -(-(32 * n_cu + 64) // 30)                                # 30 loci of 20 reads: 32 pairs per CU and a few more
    loci += [locus(41, 20, -(-per_filler // 20)) for _ in range(30)]       # packed, 32 lanes x 2
    return _abi.PackedBatch(loci)


def test_the_schedule_batch_reaches_every_kind_of_launch():
    """CPU: the shapes the GPU test below relies on, at the CU count of an MI355X."""
    L = _lib.lib()
    nk = L.ltr_debug_num_classes()
    batch = schedule_batch(256)
    grids = np.full(nk + 3, 512, dtype=np.int32)

    s = _lib.debug_plan_schedule(batch, grids, n_cu=256, **SCHEDULES["per class"])
    assert not s["use_plan"] and s["launches"] == s["by_class"]
    one = sorted(l["W"] for l in s["launches"] if l["kind"] == "one-wave")
    packed = sorted(l["W"] for l in s["launches"] if l["kind"] == "packed")
    assert len([w for w in one if w < 11]) >= 2 and len([w for w in one if w >= 11]) >= 2, one
    assert min(packed) < 13 <= max(packed), packed
    assert [l["pairs"] for l in s["launches"] if l["kind"] == "workgroup" and L.ltr_kernel_lanes_per_pair(l["cls"]) == 256] != []
    assert s["class_first"][nk] - s["class_first"][nk - 6] == 2                      # the non-ACGT pairs
    m = _lib.debug_plan_schedule(batch, grids, n_cu=256, **SCHEDULES["multi-width"])
    assert [l["kind"] for l in m["launches"]].count("multi") == 1 and len(m["by_class"]) > len(m["launches"])
    assert any(l["kind"] == "one-wave" and l["W"] < 11 for l in m["launches"]) and any(l["kind"] == "packed" and l["W"] < 13 for l in m["launches"])
    p = _lib.debug_plan_schedule(batch, grids, n_cu=256)
    assert p["use_plan"] and sorted(l["kind"] for l in p["launches"]) == ["plan", "workgroup"]
    kinds = [e["kind"] for e in p["entries"]]
    assert kinds[0] == 2 and kinds.count(0) >= 4 and kinds.count(1) >= 2              # the starters first; one-wave classes; packed widths


@pytest.mark.gpu
def test_three_schedules_at_three_timing_levels_score_and_report_alike(gpu_ctx):
    import oracle_lib as ol
    batch = schedule_batch(gpu_ctx.device_info()["n_cu"])
    ref, _, _ = ol.oracle_align_batch(batch, gpu_ctx.params)
    L = _lib.lib()
    totals = set()
    for name, knobs in SCHEDULES.items():
        for level in (0, 1, 2):
            try:
                for k, v in knobs.items():
                    gpu_ctx.set_debug(k, v)
                plan = gpu_ctx.plan(batch)
                plan.set_timing(level)
                plan.execute()
                ll, _ = plan.fetch()
                stats = plan.kernel_stats()
                plan_cls = L.ltr_plan_kernel_class(plan._h)
                plan.close()
            finally:
                gpu_ctx.set_debug("reset", 0)
            what = (name, level)
            assert np.array_equal(ll.view(np.uint64), ref.view(np.uint64)), what
            first = [k for k in stats if k["family"] != "exact"]
            totals.add((sum(k["pairs"] for k in first), sum(k["cells"] for k in first)))
            for k in first:
                if "ranges" in k:
                    assert sum(n for _, _, n in k["ranges"]) == k["pairs"], (what, k)
                assert (k["ms"] > 0) == (level > 0 and k["pairs"] > 0), (what, k)
            assert (plan_cls >= 0) == (name == "plan kernel"), what
            if name == "plan kernel":
                assert stats[plan_cls].get("plan_kernel") and len({w for _, w, _ in stats[plan_cls]["ranges"]}) > 4, what
            merged = [k for k in first if len({(lp == 64, w) for lp, w, _ in k.get("ranges", ())}) > 1]
            assert len(merged) == {"plan kernel": 1, "multi-width": 1 if level < 2 else 0, "per class": 0}[name], (what, merged)
    assert len(totals) == 1 and next(iter(totals))[0] == batch.ll_size - 2, totals         # every pair but the two that start out in the generic list
