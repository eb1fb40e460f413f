"""ltr_ll_genotype on per-read matrices against the plan path and against the per-locus composition it replaces, timed (MI355X).

    python tests/manual/gpu_ll_genotype_rate.py [--loci 100000] [--sub 5000] [--reps 9] [--out profiles/ll_genotype_rate.json]

On the loci of tests/manual/gpu_plan_vcf_rate.py (the `catalogue` workload, 1-3 samples, random labels and HP tags, 16 host
threads), after the plan has been executed once and its scores scattered to per-read matrices (ltr_scatter_pool_probs), 2 warm-up
+ --reps timed calls of each, alternating in one process:
  ll           (a) ltr_ll_genotype(fields, want_posteriors = 0, want_read_ll = 0) + ltr_genotype_result_vcf_records
  plan         (b) ltr_plan_genotype_fields + ltr_genotype_result_vcf_records on the same scores
  composition  (c) what a caller without a plan had: per locus ltr_posteriors, the prune decision on the host
               (ltr_unused_alleles, ltr_remap_haplotypes, ltr_remap_aln_probs), ltr_posteriors again where an allele went, and
               ltr_vcf_record -- on the first --sub loci, time inside the C calls, scaled to all loci
After the timed rounds one more ltr_ll_genotype runs with the library's `trace` switch on (stderr is parsed): the bytes of the
per-read block and the time of the upload phase, which is what (a) is expected to cost above (b)."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "manual"))
from longtr_amd import _abi, _lib, synth  # noqa: E402
from gpu_plan_vcf_rate import describe, stats  # noqa: E402


def traced_upload(fn):
    """Run fn() with stderr in a file; (bytes, ms) of the upload phase from the trace lines."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    t = {k: float(m.group(1)) for k in ("begins", "done") for m in [re.search(r"\[ltr\s+([0-9.]+) ms\] ll_genotype: upload of \d+ bytes.*" + k, text)] if m}
    b = re.search(r"ll_genotype: upload of (\d+) bytes", text)
    return (int(b.group(1)) if b else None), (t["done"] - t["begins"] if len(t) == 2 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--sub", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ll_genotype_rate.json"))
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
    pk_plan = plan.pack_genotype(blocks, prune=True, want_read_ll=False, **args)
    pk_ll = ctx.pack_ll_genotype(mats, rseeds, blocks, prune=True, want_read_ll=False, **largs)
    seq = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=600))
    final = plan.genotype_packed(plan.pack_genotype(blocks, prune=True, want_read_ll=False, **args))
    pv = [_abi.PackedVcfLocus(describe(c, g["blocks"], seq)) for c, g in zip(cases, final)]
    del final
    arr = (_abi.VcfLocus * n)(*[p.struct for p in pv])
    off, rpos = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    sub = min(a.sub, n)
    buf, pos = C.create_string_buffer(1 << 20), C.c_int32(0)

    def records(res, t0):
        t1 = time.perf_counter()
        text = C.c_void_p()
        ctx._check(lib.ltr_genotype_result_vcf_records(res._h, arr, None, C.byref(text), _lib._p(off), _lib._p(rpos)))
        t2 = time.perf_counter()
        lib.ltr_vcf_text_free(text)
        res.close()
        return dict(fields_ms=(t1 - t0) * 1e3, records_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)

    def run_ll():
        t0 = time.perf_counter()
        return records(ctx.genotype_ll(packed=pk_ll, fields={}), t0)

    def run_plan():
        t0 = time.perf_counter()
        return records(plan.genotype_fields(packed=pk_plan), t0)

    def composition():
        in_c = 0.0
        for c, M in zip(cases[:sub], mats[:sub]):
            c0 = time.perf_counter()
            g = gt.chain(dict(c, seeds=None), M, lambda *x: ctx.posteriors(x[0], x[1], x[2], x[3], x[4], haploid=x[5]), _lib.unused_alleles,
                         _lib.haps_to_alleles, _lib.remap_haplotypes, _lib.remap_aln_probs, False)
            in_c += time.perf_counter() - c0                     # (the chain's own Python is in this figure: an upper bound of the C time)
            p = _abi.PackedVcfLocus(dict(describe(c, g["blocks"], seq), log_aln_probs=g["read_ll"], log_sample_posteriors=g["post"],
                                         sample_total_ll=g["sample_total_ll"], best_haplotypes=g["gts"]))
            ref = C.byref(p.struct)
            c0 = time.perf_counter()
            k = lib.ltr_vcf_record(ref, None, buf, len(buf), C.byref(pos))
            in_c += time.perf_counter() - c0
            assert k > 0
        return dict(total_ms=in_c * (n / float(sub)) * 1e3)

    runs = dict(ll=[], plan=[], composition=[])
    for k in range(2 + a.reps):                                  # alternating; the first two rounds warm up
        for name, fn in (("ll", run_ll), ("plan", run_plan), ("composition", composition)):
            r = fn()
            if k >= 2:
                runs[name].append(r)
    ctx.set_debug("trace", 1)
    up_bytes, up_ms = traced_upload(lambda: ctx.genotype_ll(packed=pk_ll, fields={}).close())
    ctx.set_debug("trace", 0)
    out = dict(workload=desc, loci=n, reads=int(len(args["pool_index"])), units=int(args["n_samples"].sum()), device=ctx.device_info(),
               host_threads=ctx.host_threads(), subsample=sub, ll_block_bytes=up_bytes, upload_phase_ms=up_ms,
               results={name: {key: stats([r[key] for r in rs]) for key in rs[0]} for name, rs in runs.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
