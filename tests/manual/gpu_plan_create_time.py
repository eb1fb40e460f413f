"""Manual GPU check (not a pytest file): wall time of ltr_plan_create -- describe_batch, class statistics, the schedule, layout and
upload -- on config 3 and the catalogue, one timing loop for any build (LTR_GPU_LIB).  Prints one JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from longtr_amd import _lib, synth

REPS, WARM = 9, 2
ctx = _lib.Context(0)
out = {}
for name, n in (("config3", 10000), ("catalogue", 100000)):
    loci, _ = synth.config_loci(name, n_loci=n)
    batch, _ = synth.pack_loci(loci)
    ms = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        plan = ctx.plan(batch)
        dt = (time.perf_counter() - t0) * 1e3
        plan.close()
        if i >= WARM:
            ms.append(dt)
    ms.sort()
    out[name] = dict(loci=n, pairs=int(batch.ll_size), plan_create_ms_median=ms[len(ms) // 2], plan_create_ms_min=ms[0], plan_create_ms_max=ms[-1])
print(json.dumps(out))
