"""CPU model of a family launch run along spines (csrc/ltr_dp_family.hpp, spine_walk): every `stride`-th locus of BASELINE config 3
through the library's own forming (ltr_debug_plan_families) and spine choice (ltr_debug_plan_family_forks, by rule on a one-CU
device so that the sample forms what the whole plan forms), modelled work = wavefront steps x (W + 1.5) (ltrp::kStepOverhead).

The work of the plain families splits into stem / tail rows and their fill/drain (L - 1 steps per stream); with a spine the rows
between p and each member's fork row on the spine and one fill/drain fall away.  The fork rows of the hook are the uncapped ones
(max(p, min(lcp(spine, member), n - 1))), so the model is evaluated here for any number of park slots: the best subset of the
distinct fork rows, as the library chooses it.  Writes profiles/family_spine_model.json.  No GPU.

    python tests/manual/family_spine_model.py [stride=10]"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from longtr_amd import _lib, synth      # noqa: E402

OVERHEAD = 1.5


def best_saved(p, forks, keep):
    """Most rows the members' tails lose with at most `keep` park rows beyond p (None: all of them)."""
    beyond = sorted({f for f in forks if f > p})
    if keep is None or keep >= len(beyond):
        return sum(f - p for f in forks)
    return max(sum(max([p] + [v for v in kept if v <= f]) - p for f in forks) for kept in itertools.combinations(beyond, keep))


def main():
    stride = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    hdr = synth.config_headers("config3")
    ids = list(range(0, len(hdr), stride))
    loci, _ = synth.config_loci("config3", ids=ids)
    batch, _ = synth.pack_loci(loci)
    base = _lib.debug_plan_families(batch, n_cu=1)
    forks = _lib.debug_plan_family_forks(batch, n_cu=1, family_spine=1)
    assert len(base["families"]) == len(forks["families"])
    caps = {"1": 1, "2": 2, "4": 4, "7": 7, "uncapped": None}
    parts = dict(stem_rows=0.0, stem_fill=0.0, tail_rows=0.0, tail_fill=0.0)
    work = {k: {"all": 0.0, "narrow": 0.0, "wide": 0.0} for k in list(caps) + ["plain", "library"]}
    tails, H, lanes, with_fork, distinct = [], [], [], 0, []
    for b, f in zip(base["families"], forks["families"]):
        assert b["out_idx"] == f["out_idx"]
        W, p, n = b["W"], b["p"], b["n"]
        m = min(n) - b["dd_min"]
        L = -(-(m - 1) // W)
        c = W + OVERHEAD
        band = "narrow" if W <= 10 else "wide"
        parts["stem_rows"] += (p - 1) * c; parts["stem_fill"] += (L - 1) * c
        parts["tail_rows"] += sum(x - p for x in n) * c; parts["tail_fill"] += len(n) * (L - 1) * c
        plain = (p - 1) + (L - 1) + sum(x - p + L - 1 for x in n)
        for key, v in (("plain", plain), ("library", f["steps"])):
            work[key]["all"] += v * c; work[key][band] += v * c
        tails += [x - p for x in n]; H.append(len(n)); lanes.append(L)
        others = [f["fork"][k] for k in range(len(n)) if k != f["spine"]] if f["spine"] >= 0 else []
        with_fork += f["spine"] >= 0
        distinct.append(len({x for x in others if x > p}))
        for key, keep in caps.items():
            v = plain if f["spine"] < 0 else plain - (L - 1) - best_saved(p, others, keep)
            work[key]["all"] += v * c; work[key][band] += v * c
    total = work["plain"]["all"]
    out = {
        "what": "every %dth locus of config 3 (seed %d): %d families formed by rule, pooled reads of 321 .. 1280 columns; work = steps x (W + 1.5)" % (stride, synth.CONFIG_SEED, len(H)),
        "families": len(H), "mean_H": float(np.mean(H)), "mean_lanes": float(np.mean(lanes)),
        "tail_rows_per_member": {"median": float(np.median(tails)), "mean": float(np.mean(tails))},
        "plain_work_split": {k: v / total for k, v in parts.items()},
        "families_with_a_fork_beyond_p": with_fork / len(H), "most_distinct_fork_rows_beyond_p": int(max(distinct)),
        "work_relative_to_plain": {"park_rows_beyond_p_" + k: {band: work[k][band] / work["plain"][band] for band in ("all", "narrow", "wide")} for k in caps},
        "library_as_built": {"park_slots": forks["park_slots"], "work_relative_to_plain": work["library"]["all"] / total,
                             "families_with_a_spine": forks["with_spine"], "steps_saved": forks["steps_saved"]},
    }
    path = os.path.join(ROOT, "profiles", "family_spine_model.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
