"""Measurement (recorded, not gated): longtr_amd.call.genotype_regions on the bundled trio, five runs after a warm-up, with the
producer thread on and off in the same session.  Writes the per-stage seconds of every run and both medians with min - max, with
the tree's source_id.  Forty loci are too few for a stable ratio and there is no earlier number for this path: no threshold is set.

    python tests/manual/gpu_call_trio.py [out.json]          (default profiles/call_trio.json)
"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from longtr_amd import _lib, call  # noqa: E402
import test_gpu_call as T  # noqa: E402

RUNS = 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "call_trio.json")
    d = tempfile.mkdtemp(prefix="call_trio_")
    bed = os.path.join(d, "regions.bed")
    T.rt.convert_bed(os.path.join(T.DATA, "test_regions_hg38.bed"), bed)
    regions, _ = _lib.read_regions(bed, order=True)
    ref = T.ReadsReference(regions)
    ctx = _lib.Context(0)
    result = dict(what="longtr_amd.call.genotype_regions, bundled trio, chunk_loci=8 (5 chunks, so that the producer has something to overlap)",
                  source_id=_lib.source_id(), device=ctx.device_info(), loci=len(regions), runs=RUNS, modes={})
    go = lambda overlap: call.genotype_regions(ctx, T.BAMS, ref, bed, os.path.join(d, "out.vcf"), chunk_loci=8, overlap=overlap)
    r = go(True)                                                 # warm-up (code objects, pools)
    assert r["error"] is None, r["error"]
    result["genotyped"] = r["counters"]["genotype_success"]
    walls = {True: [], False: []}
    stages = {True: [], False: []}
    for _ in range(RUNS):
        for overlap in (True, False):                            # interleaved: both modes see the same drift
            r = go(overlap)
            assert r["error"] is None, r["error"]
            walls[overlap].append(r["timing"]["wall_seconds"])
            stages[overlap].append(r["timing"]["stage_seconds"])
    for overlap in (True, False):
        w = walls[overlap]
        result["modes"]["overlap_on" if overlap else "overlap_off"] = dict(
            wall_seconds=w, median=statistics.median(w), min=min(w), max=max(w), stage_seconds=stages[overlap],
            stage_median={k: statistics.median(s[k] for s in stages[overlap]) for k in call.STAGES})
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["median"], v["min"], v["max"]) for k, v in result["modes"].items()}))


if __name__ == "__main__":
    main()
