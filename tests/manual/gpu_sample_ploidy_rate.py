"""ltr_ll_genotype with a ploidy per (locus, sample) against the uniform call, timed (MI355X).

    python tests/manual/gpu_sample_ploidy_rate.py [--loci 100000] [--reps 9] [--every 3] [--out profiles/sample_ploidy_rate.json]

The loci, matrices and calls of tests/manual/gpu_ll_genotype_rate.py (the `catalogue` workload, 1-3 samples, random labels and HP tags,
16 host threads; fields, want_posteriors = 0, want_read_ll = 0, then ltr_genotype_result_vcf_records), 2 warm-up + --reps timed calls of
each, alternating in one process:
  uniform  ltr_ll_genotype (every sample diploid)
  zeros    ltr_ll_genotype_sample_ploidy with an all-zero array: the same work through the new entry point
  mixed    ltr_ll_genotype_sample_ploidy with every --every-th unit haploid (unit order), so most loci of two or three samples are mixed"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "manual"))
from longtr_amd import _abi, _lib, synth  # noqa: E402
from gpu_plan_vcf_rate import describe, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--every", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_ploidy_rate.json"))
    a = ap.parse_args()
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
    batch, args = gt.pack(cases)
    plan = ctx.plan(batch)
    plan.execute()
    ll, seeds = plan.fetch()
    n = len(cases)
    blocks = [c["blocks"] for c in cases]
    mats, rseeds = [], []
    for l, c in enumerate(cases):
        r0 = int(batch.locus_read_off[l])
        M, s = _lib.scatter_pool_probs(batch.locus_matrix(ll, l), seeds[r0:r0 + len(c["pools"])], c["pool_index"], len(c["haps"]))
        mats.append(M)
        rseeds.append(s)
    largs = {k: v for k, v in args.items() if k != "pool_index"}
    pk = ctx.pack_ll_genotype(mats, rseeds, blocks, prune=True, want_read_ll=False, **largs)
    seq = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=600))
    nu = int(args["n_samples"].sum())
    flags = dict(zeros=np.zeros(nu + 1, dtype=np.uint8), mixed=(np.arange(nu + 1) % a.every == a.every - 1).astype(np.uint8))
    fr = _abi.FieldsRequest()
    off, rpos = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)

    def call(name):
        h = C.c_void_p()
        if name == "uniform":
            ctx._check(lib.ltr_ll_genotype(ctx._h, C.byref(pk["lb"]), C.byref(pk["gb"]), C.byref(fr), C.byref(h)))
        else:
            ctx._check(lib.ltr_ll_genotype_sample_ploidy(ctx._h, C.byref(pk["lb"]), C.byref(pk["gb"]), C.byref(fr), _lib._p(flags[name]), C.byref(h)))
        return _lib.GenotypeResult(ctx, h, pk)

    arrs = {}
    for name in ("uniform", "mixed"):                            # the final block lists differ with the calls: one description of the loci each
        with call(name) as res:
            pv = [_abi.PackedVcfLocus(describe(c, res.locus(l)["blocks"], seq)) for l, c in enumerate(cases)]
            n_mixed = sum(1 for l in range(n) if 0 < res.sample_haploid(l).sum() < cases[l]["S"])
        arrs[name] = ((_abi.VcfLocus * n)(*[p.struct for p in pv]), pv, n_mixed)
    arrs["zeros"] = arrs["uniform"]

    def run(name):
        t0 = time.perf_counter()
        res = call(name)
        t1 = time.perf_counter()
        text = C.c_void_p()
        ctx._check(lib.ltr_genotype_result_vcf_records(res._h, arrs[name][0], None, C.byref(text), _lib._p(off), _lib._p(rpos)))
        t2 = time.perf_counter()
        lib.ltr_vcf_text_free(text)
        res.close()
        return dict(fields_ms=(t1 - t0) * 1e3, records_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)

    runs = dict(uniform=[], zeros=[], mixed=[])
    for k in range(2 + a.reps):
        for name in runs:
            r = run(name)
            if k >= 2:
                runs[name].append(r)
    out = dict(workload=desc, loci=n, units=nu, mixed_loci=arrs["mixed"][2], every=a.every, device=ctx.device_info(), host_threads=ctx.host_threads(),
               source_id=_lib.source_id(), results={name: {key: stats([r[key] for r in rs]) for key in rs[0]} for name, rs in runs.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
