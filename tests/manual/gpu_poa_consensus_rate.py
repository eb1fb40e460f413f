"""Rate of ltr_poa_consensus (ltr_poa.hip) on two workloads -- 2 000 groups of 12 x 300 bases, 64 groups of 30 x 5 000 bases (BASELINE config
5's lengths), unique noisy copies at 5 % -- and of ltr_build_haplotypes_consensus against ltr_build_haplotypes_clustered (the medoid path, the
behaviour before the consensus existed) on 300 noisy loci in the same session.  Warm-up calls, then at least 5 timed calls, medians with
min - max, 16 host threads.  Writes profiles/poa_consensus_rate.json.  The times are whole calls (host packing, upload, kernel, download):
the library has no timer inside this call, so the kernel alone is NOT separated here.  DP cells = sum over the alignments of nodes x
columns, counted by the restatement (tests/poa_util.Graph.cells) on a sample of the groups and scaled to the workload.  There is no host POA to
compare with.

    python tests/manual/gpu_poa_consensus_rate.py [--small]      (--small: a tenth of the work, for a quick look; writes nothing)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cluster_util as cu  # noqa: E402
import poa_util as pu  # noqa: E402
from longtr_amd import _lib  # noqa: E402
from gpu_edit_distance_rate import noisy  # noqa: E402
from test_gpu_cluster_haplotypes import noisy_locus  # noqa: E402


def workload(rng, n_groups, members, length):
    groups = []
    for _ in range(n_groups):
        base = cu.BASES[rng.integers(0, 4, size=length)]
        g = set()
        while len(g) < members:
            g.add(noisy(rng, base, 0.05))
        groups.append(sorted(g, key=cu._order))
    return groups


def timed(fn, warm, reps):
    times = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
        print(f"  call {k}: {times[-1] * 1e3:.1f} ms", flush=True)
    times = sorted(times[warm:])
    return out, dict(median=times[len(times) // 2] * 1e3, min=times[0] * 1e3, max=times[-1] * 1e3)


def main():
    small = "--small" in sys.argv
    ctx = _lib.Context(0)
    ctx.set_host_threads(16)
    out = dict(device=ctx.device_info(), source_id=_lib.source_id(), workloads=[])
    rng = np.random.default_rng(2026)
    for name, n_groups, members, length, sample, warm in (("2000 x 12 x 300", 200 if small else 2000, 12, 300, 8, 2),
                                                         ("64 x 30 x 5000", 6 if small else 64, 30, 5000 if not small else 1000, 1, 1)):
        groups = workload(rng, n_groups, members, length)
        packed = _lib.pack_seq_groups(groups)
        print(name, flush=True)
        (got, status), ms = timed(lambda: _lib.poa_consensus(ctx, None, packed=packed, with_status=True), warm, 5)
        assert status == [0] * n_groups
        t0 = time.perf_counter()
        graphs = [pu.poa_graph(g) for g in groups[:sample]]
        cells = float(np.mean([g.cells for g in graphs])) * n_groups
        assert got[:sample] == [g.consensus() for g in graphs]
        print(f"  restatement of {sample} group(s): {time.perf_counter() - t0:.1f} s", flush=True)
        med = ms["median"] / 1e3
        out["workloads"].append(dict(name=name, groups=n_groups, cells=cells, cells_counted_on=f"{sample} group(s) by the restatement, scaled", call_ms=ms,
                                     groups_per_s=n_groups / med, cells_per_s=cells / med, kernel_alone="not separated: the call has no timer inside"))
        print(json.dumps(out["workloads"][-1]), flush=True)
    # 300 noisy loci: the consensus composition against the medoid composition
    n_loci = 30 if small else 300
    args, keep = [], []
    t0 = time.perf_counter()
    for k in range(n_loci):
        d = noisy_locus(seed=1000 + k, ref_len=330, alleles=(300, 360), n_reads=30, err=(0.03, 0.05, 0.08)[k % 3])
        rs0, re0 = d["region"]
        rs = _lib.ReadSet(d["raw"], d["n_samples"], rs0, re0, d["chrom"], d["chrom_start"])
        keep.append((d, rs))
        args.append(dict(rs=rs, region_start=rs0, region_stop=re0, period=d["period"], chrom_seq_start=d["chrom_start"], chrom_len=d["chrom_len"]))
    print(f"{n_loci} loci prepared in {time.perf_counter() - t0:.1f} s", flush=True)
    medoid, ms_medoid = timed(lambda: ctx.build_haplotypes_clustered(args), 1, 5)
    cons, ms_cons = timed(lambda: ctx.build_haplotypes_consensus(args), 1, 5)
    rounds = [r["consensus_rounds"][0] for r in cons]
    out["composition"] = dict(loci=n_loci, reads_per_locus=30, alleles=[300, 360], error=[0.03, 0.05, 0.08],
                              clustered_medoid_call_ms=ms_medoid, consensus_call_ms=ms_cons,
                              consensus_rounds=dict(total=int(sum(rounds)), max=int(max(rounds)), mean=float(np.mean(rounds))),
                              medoid_kept=int(sum(r["medoid_kept"][0] for r in cons)),
                              new_alleles=dict(medoid=int(sum(sum(r["inexact"]) for r in medoid)), consensus=int(sum(sum(r["inexact"]) for r in cons))))
    print(json.dumps(out["composition"]), flush=True)
    if not small:
        json.dump(out, open(os.path.join(ROOT, "profiles", "poa_consensus_rate.json"), "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
