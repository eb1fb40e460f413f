"""Rate of ltr_edit_distances (ltr_editdist.hip) on two workloads -- 2 000 groups of 40 x 300 bases, 64 groups of 40 x 5 000 bases, noisy
copies at 5 % -- against the plain cell-by-cell loop of the reference's needleman_wunsch (HaplotypeGenerator.cpp:201-234, written out
here in a few lines of C++ and compiled by this script) on one host thread.  2 warm-up + 9 timed calls, medians with min - max, 16 host
threads.  Writes profiles/edit_distance_rate.json.  The times are whole calls (host packing, upload, kernel, download, scatter): the
library has no timer inside this call, so the kernel alone is NOT separated here.

    python tests/manual/gpu_edit_distance_rate.py [--small]      (--small: a tenth of the groups, for a quick look)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cluster_util as cu  # noqa: E402
import isa_util  # noqa: E402
from longtr_amd import _lib  # noqa: E402

SCALAR = r"""
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>
extern "C" long long scalar_nw(const unsigned char* a, int n, const unsigned char* b, int m) {
  std::vector<int32_t> dp((size_t)(n + 1) * (m + 1));
  for (int i = 0; i <= n; ++i) dp[(size_t)i * (m + 1)] = i;
  for (int j = 0; j <= m; ++j) dp[j] = j;
  for (int i = 1; i <= n; ++i) {
    int row_min = 1000;
    for (int j = 1; j <= m; ++j) {
      const int s = a[i - 1] == b[j - 1] ? 0 : 1;
      const int v = std::min(dp[(size_t)(i - 1) * (m + 1) + j] + 1, std::min(dp[(size_t)i * (m + 1) + j - 1] + 1, dp[(size_t)(i - 1) * (m + 1) + j - 1] + s));
      dp[(size_t)i * (m + 1) + j] = v;
      row_min = std::min(row_min, v + std::abs((n - m) - (i - j)));
    }
    if (row_min > 100000) return -1;
  }
  return dp[(size_t)n * (m + 1) + m];
}
"""


def step_loop_valu():
    """Vector instructions of one step of the kernel's column loop (one 64-row block x one column per lane), from the gfx950 assembly."""
    f = isa_util.analyse("ltr_editdist.hip")
    k = [v for n, v in f.items() if "ltr_editdist_kernel" in n][0]
    asm = isa_util.assembly("ltr_editdist.hip").splitlines()
    start = [i for i, l in enumerate(asm) if re.match(r"^\s*\.type\s+\S*ltr_editdist_kernel\S*,@function", l)][0]
    best = None
    for L in k["loops"]:
        seg = asm[start + L["first"]:start + L["last"] + 1]
        if any("row_shr" in x or "wave_shr" in x or "dpp" in x for x in seg) and (best is None or L["instructions"] < best[0]):
            best = (L["instructions"], sum(1 for x in seg if re.match(r"^\s+v_", x)), sum(1 for x in seg if re.match(r"^\s+ds_", x)))
    return dict(instructions=best[0], valu=best[1], lds=best[2]) if best else None


def workload(rng, n_groups, length):
    groups = []
    for _ in range(n_groups):
        base = cu.BASES[rng.integers(0, 4, size=length)]
        groups.append([noisy(rng, base, 0.05) for _ in range(40)])
    return groups


def noisy(rng, base, err):
    """cluster_util.noisy_copy without the per-base loop: deletions, substitutions, 1-base insertions, err in total."""
    r = rng.random(len(base))
    out = base.copy()
    sub = (r >= err / 3) & (r < 2 * err / 3)
    out[sub] = cu.BASES[rng.integers(0, 4, size=int(sub.sum()))]
    ins = np.flatnonzero(r >= 1.0 - err / 3)
    out = np.insert(out, ins + 1, cu.BASES[rng.integers(0, 4, size=len(ins))])
    keep = np.insert(r >= err / 3, ins + 1, True)
    return out[keep].tobytes()


def main():
    small = "--small" in sys.argv
    ctx = _lib.Context(0)
    ctx.set_host_threads(16)
    with tempfile.TemporaryDirectory() as tmp:
        src, so = os.path.join(tmp, "scalar.cpp"), os.path.join(tmp, "scalar.so")
        open(src, "w").write(SCALAR)
        subprocess.run(["g++", "-O3", "-shared", "-fPIC", src, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.scalar_nw.restype = C.c_longlong
        lib.scalar_nw.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        out = dict(device=ctx.device_info(), source_id=_lib.source_id(), step_loop=step_loop_valu(), workloads=[])
        rng = np.random.default_rng(2025)
        for name, n_groups, length in (("2000 x 40 x 300", 200 if small else 2000, 300), ("64 x 40 x 5000", 6 if small else 64, 5000)):
            groups = workload(rng, n_groups, length)
            packed = _lib.pack_seq_groups(groups)
            pairs = sum(len(g) * (len(g) - 1) // 2 for g in groups)
            cells = float(sum(len(g[i]) * len(g[j]) for g in groups for i in range(len(g)) for j in range(i + 1, len(g))))
            dist = np.zeros(int(packed["dist_off"][-1]), dtype=np.int32)
            times = []
            for k in range(11):
                t0 = time.perf_counter()
                got = _lib.edit_distances(ctx, None, 701, dist=dist, packed=packed)
                times.append(time.perf_counter() - t0)
            times = sorted(times[2:])
            g0 = groups[0]
            t0 = time.perf_counter()
            want = [lib.scalar_nw(g0[0], len(g0[0]), g0[j], len(g0[j])) for j in range(1, 9)]
            host = (time.perf_counter() - t0) / sum(len(g0[0]) * len(g0[j]) for j in range(1, 9))
            assert [int(got[0][0, j]) for j in range(1, 9)] == [min(int(w), 701) for w in want]
            med = times[len(times) // 2]
            out["workloads"].append(dict(name=name, pairs=pairs, cells=cells, call_ms=dict(median=med * 1e3, min=times[0] * 1e3, max=times[-1] * 1e3),
                                         pairs_per_s=pairs / med, cells_per_s=cells / med, host_scalar_cells_per_s=1.0 / host,
                                         kernel_alone="not separated: the call has no timer inside"))
            print(json.dumps(out["workloads"][-1]))
    path = os.path.join(ROOT, "profiles", "edit_distance_rate.json")
    if not small:
        json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out["step_loop"]))
    ctx.close()


if __name__ == "__main__":
    main()
