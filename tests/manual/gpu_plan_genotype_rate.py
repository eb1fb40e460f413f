"""Consumer side of a catalogue plan, timed (MI355X): ltr_plan_genotype against what it replaces.

    python tests/manual/gpu_plan_genotype_rate.py [--loci 100000] [--sub 5000] [--reps 9] [--out profiles/plan_genotype_rate.json]

On the `catalogue` workload's loci (posterior batch as tests/test_gpu_host_path.py::test_plan_posteriors_all_loci_on_device builds
it: 1-3 samples, random labels and HP tags), after the plan has been executed once:
  genotype          ltr_plan_genotype, both passes, download included (with and without the per-read matrices)
  first_pass        ltr_plan_genotype with prune = 0 against ltr_plan_posteriors on the same plan (same output bits)
  baseline          ltr_plan_posteriors + the host loop (ltr_unused_alleles per block, pruned blocks, ltr_remap_haplotypes,
                    ltr_remap_aln_probs) + one ltr_posteriors per affected locus, through the Python binding, on the first --sub
                    loci and scaled to all of them; `posteriors_only` is the time inside the ltr_posteriors calls alone (the
                    part no faster host loop could remove)
  per_H             first_pass and ltr_plan_posteriors again on a plan of their own per H bucket (2, 3, 4, 5-8, 9-12)
--kernels-only runs just those per-bucket calls (5 of each, ltr_plan_posteriors first), for a kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/manual/gpu_plan_genotype_rate.py --kernels-only
    python tests/manual/gpu_plan_genotype_rate.py --parse-trace DIR/.../*_kernel_trace.csv --out profiles/plan_genotype_kernels.json
(--parse-trace needs no GPU: device time of the posterior kernels per bucket, in dispatch order.)
Every figure is the median over --reps back-to-back calls after two warm-up calls (a stream of calls: the device clock is up);
min / max are the spread seen."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from longtr_amd import _abi, _lib, synth  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def parse_trace(path, out_path):
    """Kernel trace of a --kernels-only run -> per bucket (dispatch order) the median device time of the loop kernels
    (ltr_posterior_batch_kernel + its finish kernel) and of ltr_genotype_kernel (+ finish), microseconds."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    runs = []                                                    # consecutive dispatches of one family: [family, device us, calls]
    fam = lambda n: "loop" if "ltr_posterior_batch" in n else ("exp_once" if "ltr_genotype_" in n else None)
    for r in rows:
        f, name = fam(r["Kernel_Name"]), r["Kernel_Name"]
        if f is None:
            continue
        if not runs or runs[-1][0] != f:
            runs.append([f, 0.0, 0])
        runs[-1][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        runs[-1][2] += 0 if "finish" in name else 1              # (a call = one main kernel, + the finish kernel where one runs)
    names = ["2-2", "3-3", "4-4", "5-8", "9-12"]
    out = {}
    for k in range(0, len(runs) - 1, 2):
        b = names[k // 2] if k // 2 < len(names) else str(k // 2)
        out[b] = {runs[k][0] + "_us_per_call": runs[k][1] / max(runs[k][2], 1), runs[k + 1][0] + "_us_per_call": runs[k + 1][1] / max(runs[k + 1][2], 1),
                  "calls": [runs[k][2], runs[k + 1][2]]}
    json.dump(dict(source=os.path.basename(path), device_time_per_call=out), open(out_path, "w"), indent=1)
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--sub", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="one more call of each kind with the library's phase trace on stderr")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--parse-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_genotype_rate.json"))
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a.parse_trace, a.out)
    import genotype_util as gt
    loci, desc = synth.config_loci("catalogue", n_loci=a.loci, workers=16)
    rng = np.random.default_rng(41)
    cases = []
    for L in loci:
        R = len(L.trimmed_reads)
        S = int(rng.integers(1, 4))
        hp = rng.integers(0, 3, size=R)
        pools, pidx = synth.pool_reads(L.trimmed_reads)
        cases.append(dict(blocks=L.blocks(), haps=L.haplotypes, pools=pools, pool_index=np.asarray(pidx, dtype=np.int32), S=S,
                          lab=rng.integers(0, S, size=R).astype(np.int32), p1=np.where(hp == 1, -1e-6, np.where(hp == 2, -1000.0, 0.0)),
                          p2=np.where(hp == 2, -1e-6, np.where(hp == 1, -1000.0, 0.0)), filt=np.zeros(S, dtype=np.uint8)))
    batch, args = gt.pack(cases)
    ctx = _lib.Context(0)
    plan = ctx.plan(batch)
    plan.execute()
    plan.wait()
    n = len(cases)
    H = np.diff(batch.locus_hap_off)
    out = dict(workload=desc, loci=n, reads=int(len(args["pool_index"])), units=int(args["n_samples"].sum()), device=ctx.device_info(),
               host_threads=ctx.host_threads(), H_histogram={int(h): int(c) for h, c in zip(*np.unique(H, return_counts=True))})
    blocks = [c["blocks"] for c in cases]
    L = _lib.lib()

    def bucket_calls(lo, hi, reps, warm):
        """first_pass / ltr_plan_posteriors on a plan of the loci with lo <= H <= hi."""
        sel = [c for c, h in zip(cases, H) if lo <= h <= hi]
        b2, a2 = gt.pack(sel)
        p2 = ctx.plan(b2)
        p2.execute()
        p2.wait()
        h2 = np.diff(b2.locus_hap_off)
        pb2, keep2 = p2._posterior_batch(haploid=False, **a2)
        sz = np.repeat(h2 * h2, a2["n_samples"])
        o = [np.zeros(int(sz.sum())), np.zeros(len(sz)), np.zeros(2 * len(sz), dtype=np.int32)]
        r = dict(loci=len(sel), units=int(len(sz)))
        r["plan_posteriors"] = timed(lambda: ctx._check(L.ltr_plan_posteriors(p2._h, C.byref(pb2), _lib._p(o[0]), _lib._p(o[1]), _lib._p(o[2]))), reps, warm)
        pk = p2.pack_genotype([c["blocks"] for c in sel], prune=False, want_read_ll=False, **a2)
        r["first_pass"] = timed(lambda: p2.genotype_packed(pk, decode=False), reps, warm)
        p2.close()
        return r

    BUCKETS = ((2, 2), (3, 3), (4, 4), (5, 8), (9, 12))
    if a.kernels_only:
        for lo, hi in BUCKETS:
            bucket_calls(lo, hi, 5, 0)
        plan.close()
        ctx.close()
        return
    out["per_H"] = {f"{lo}-{hi}": bucket_calls(lo, hi, a.reps, 2) for lo, hi in BUCKETS}
    res = {}
    for key, kw in (("genotype", dict(prune=True, want_read_ll=False)), ("genotype_with_read_ll", dict(prune=True, want_read_ll=True)),
                    ("first_pass", dict(prune=False, want_read_ll=False))):
        packed = plan.pack_genotype(blocks, **kw, **args)
        res[key] = timed(lambda: plan.genotype_packed(packed, decode=False), a.reps)
        res[key]["loci_per_s"] = n / res[key]["median_ms"] * 1e3
    if a.trace:
        ctx.set_debug("trace", 1)
        for kw in (dict(prune=False, want_read_ll=False), dict(prune=True, want_read_ll=True)):
            plan.genotype_packed(plan.pack_genotype(blocks, **kw, **args), decode=False)
        ctx.set_debug("trace", 0)
    # ltr_plan_posteriors on the same plan, arrays built once
    pb, keep = plan._posterior_batch(haploid=False, **args)
    sizes = np.repeat(H * H, args["n_samples"])
    post, stl, gts = np.zeros(int(sizes.sum())), np.zeros(len(sizes)), np.zeros(2 * len(sizes), dtype=np.int32)
    res["plan_posteriors"] = timed(lambda: ctx._check(L.ltr_plan_posteriors(plan._h, C.byref(pb), _lib._p(post), _lib._p(stl), _lib._p(gts))), a.reps)
    # how many loci the pruning touches
    full = plan.genotype_packed(plan.pack_genotype(blocks, prune=True, want_read_ll=False, **args))
    out["loci_pruned"] = int(sum(1 for g in full if g["num_aff_alleles"]))
    # the composed baseline on a subsample (the parent's entry points through the Python binding)
    sub = min(a.sub, n)
    ll, _ = plan.fetch()
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    inner = [0.0]

    def posteriors(*x):
        t0 = time.perf_counter()
        r = ctx.posteriors(x[0], x[1], x[2], x[3], x[4], haploid=x[5])
        inner[0] += time.perf_counter() - t0
        return r

    def host_loop():
        inner[0] = 0.0
        u = 0
        for l in range(sub):
            c = cases[l]
            S, h = c["S"], int(H[l])
            first = dict(post=post[off[u]:off[u + S]].reshape(S, h, h), sample_total_ll=stl[u:u + S], gts=gts.reshape(-1, 2)[u:u + S])
            u += S
            gt.chain(c, gt.per_read(batch, ll, l, c), posteriors, _lib.unused_alleles, _lib.haps_to_alleles, _lib.remap_haplotypes,
                     _lib.remap_aln_probs, False, True, first=first)

    loop = timed(host_loop, 3, warm=1)
    res["baseline_host_loop_subsample"] = dict(loop, loci=sub, posteriors_only_ms=inner[0] * 1e3)
    scale = n / float(sub)
    res["baseline_scaled"] = dict(total_ms=res["plan_posteriors"]["median_ms"] + loop["median_ms"] * scale,
                                  posteriors_only_ms=res["plan_posteriors"]["median_ms"] + inner[0] * 1e3 * scale, scaled_by=scale)
    out["results"] = res
    spread = res["plan_posteriors"]["max_ms"] - res["plan_posteriors"]["min_ms"]
    out["first_pass_vs_plan_posteriors"] = dict(first_pass_ms=res["first_pass"]["median_ms"], plan_posteriors_ms=res["plan_posteriors"]["median_ms"],
                                                spread_ms=spread, not_slower=bool(res["first_pass"]["median_ms"] <= res["plan_posteriors"]["median_ms"] + spread))
    out["beats_composed_baseline"] = bool(res["genotype_with_read_ll"]["median_ms"] < res["baseline_scaled"]["posteriors_only_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
