"""From a genotyped catalogue plan to VCF records, timed (MI355X): ltr_plan_genotype_fields + ltr_genotype_result_vcf_records
against the composition they replace.

    python tests/manual/gpu_plan_vcf_rate.py [--loci 100000] [--sub 5000] [--reps 9] [--out profiles/plan_vcf_rate.json]

On the loci of tests/manual/gpu_plan_genotype_rate.py (the `catalogue` workload, 1-3 samples, random labels and HP tags), after
the plan has been executed once, 2 warm-up + --reps timed calls of each, alternating:
  parent   ltr_plan_genotype(want_read_ll = 1) + one ltr_vcf_record per locus on the first --sub loci, scaled to all of them;
           `in_c_ms` is the time inside the C calls alone, without the interpreter's loop around ltr_vcf_record
  new      ltr_plan_genotype_fields(want_posteriors = 0, want_read_ll = 0) + ltr_genotype_result_vcf_records, all loci;
           the two calls are also given apart (fields_ms / records_ms: arithmetic + transfers against the formatter)
  genotype ltr_plan_genotype(want_read_ll = 0) alone, as profiles/plan_genotype_rate.json has it
--kernels-only runs five new calls per H bucket (2, 3, 4, 5-8, 9-12) on plans of their own for
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/manual/gpu_plan_vcf_rate.py --kernels-only
and --parse-trace CSV (no GPU) adds the device time of ltr_genotype_fields_kernel per bucket, in dispatch order, to --out."""
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

BUCKETS = ((2, 2), (3, 3), (4, 4), (5, 8), (9, 12))


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=len(ts))


def parse_trace(path, out_path):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "ltr_genotype_fields_kernel" in r["Kernel_Name"]]
    per = len(us) // len(BUCKETS)                                # the same number of launches per bucket, in dispatch order
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["fields_kernel_device_us"] = {f"{lo}-{hi}": dict(median_us_per_launch=float(np.median(us[k * per:(k + 1) * per])), launches=per)
                                      for k, (lo, hi) in enumerate(BUCKETS)} if per else {}
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out["fields_kernel_device_us"], indent=1))


def describe(c, g_blocks, rng_seq):
    s0 = g_blocks[1]["start"]
    S = c["S"]
    none = np.zeros(0)
    return dict(chrom="chr1", region_start=s0 + 5, region_stop=g_blocks[1]["end"] - 5, name="", motif="N", period_str="1", chrom_seq=rng_seq,
                chrom_seq_start=s0 - 300, blocks=g_blocks, block=1, log_aln_probs=none, log_p1=c["p1"], log_p2=c["p2"], sample_label=c["lab"],
                alns=None, log_sample_posteriors=none, sample_total_ll=none, best_haplotypes=np.zeros(0, dtype=np.int32),
                sample_names=["S%d" % s for s in range(S)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--sub", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--parse-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_vcf_rate.json"))
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
    ctx = _lib.Context(0)
    ctx.set_host_threads(16)
    lib = _lib.lib()
    if a.kernels_only:
        H = np.asarray([len(c["haps"]) for c in cases])
        for lo, hi in BUCKETS:
            sel = [c for c, h in zip(cases, H) if lo <= h <= hi]
            b2, a2 = gt.pack(sel)
            p2 = ctx.plan(b2)
            p2.execute()
            p2.wait()
            pk = p2.pack_genotype([c["blocks"] for c in sel], prune=True, want_read_ll=False, **a2)
            for _ in range(5):
                p2.genotype_fields(packed=pk).close()
            p2.close()
        ctx.close()
        return
    batch, args = gt.pack(cases)
    plan = ctx.plan(batch)
    plan.execute()
    plan.wait()
    n = len(cases)
    blocks = [c["blocks"] for c in cases]
    pk_parent = plan.pack_genotype(blocks, prune=True, want_read_ll=True, **args)
    pk_new = plan.pack_genotype(blocks, prune=True, want_read_ll=False, **args)
    seq = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=600))
    # the locus descriptions around the final block lists (built once, outside the timed calls, for both paths)
    final = plan.genotype_packed(pk_parent)
    sub = min(a.sub, n)
    pv_new = [_abi.PackedVcfLocus(describe(c, g["blocks"], seq)) for c, g in zip(cases, final)]
    pv_old = [_abi.PackedVcfLocus(dict(describe(c, g["blocks"], seq), log_aln_probs=g["read_ll"], log_sample_posteriors=g["post"],
                                      sample_total_ll=g["sample_total_ll"], best_haplotypes=g["gts"])) for c, g in zip(cases[:sub], final[:sub])]
    del final
    arr = (_abi.VcfLocus * n)(*[p.struct for p in pv_new])
    buf, pos = C.create_string_buffer(1 << 20), C.c_int32(0)
    off, rpos = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)

    def parent():
        t0 = time.perf_counter()
        plan.genotype_packed(pk_parent, decode=False)
        t1 = time.perf_counter()
        in_c = 0.0
        for p in pv_old:
            ref = C.byref(p.struct)
            c0 = time.perf_counter()
            k = lib.ltr_vcf_record(ref, None, buf, len(buf), C.byref(pos))
            in_c += time.perf_counter() - c0
            assert k > 0
        t2 = time.perf_counter()
        scale = n / float(sub)
        return dict(genotype_ms=(t1 - t0) * 1e3, in_c_ms=(t1 - t0 + in_c * scale) * 1e3, with_loop_ms=(t1 - t0 + (t2 - t1) * scale) * 1e3,
                    records_in_c_ms=in_c * scale * 1e3)

    def new():
        t0 = time.perf_counter()
        res = plan.genotype_fields(packed=pk_new)
        t1 = time.perf_counter()
        text = C.c_void_p()
        ctx._check(lib.ltr_genotype_result_vcf_records(res._h, arr, None, C.byref(text), _lib._p(off), _lib._p(rpos)))
        t2 = time.perf_counter()
        lib.ltr_vcf_text_free(text)
        res.close()
        return dict(fields_ms=(t1 - t0) * 1e3, records_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)

    def genotype():
        t0 = time.perf_counter()
        plan.genotype_packed(pk_new, decode=False)
        return dict(total_ms=(time.perf_counter() - t0) * 1e3)

    runs = dict(parent=[], new=[], genotype=[])
    for k in range(2 + a.reps):                                  # alternating; the first two rounds warm up
        for name, fn in (("parent", parent), ("new", new), ("genotype", genotype)):
            r = fn()
            if k >= 2:
                runs[name].append(r)
    out = dict(workload=desc, loci=n, reads=int(len(args["pool_index"])), units=int(args["n_samples"].sum()), device=ctx.device_info(),
               host_threads=ctx.host_threads(), subsample=sub,
               results={name: {key: stats([r[key] for r in rs]) for key in rs[0]} for name, rs in runs.items()})
    p, q = out["results"]["parent"]["in_c_ms"], out["results"]["new"]["total_ms"]
    spread = max(p["max_ms"] - p["min_ms"], q["max_ms"] - q["min_ms"])
    out["new_below_parent_in_c_by_more_than_the_spread"] = bool(q["median_ms"] < p["median_ms"] - spread)
    out["spread_ms"] = spread
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
