"""CPU A/B of the planning units (csrc/ltr_plan_*.cpp) between two builds of the library: every ltr_debug_* hook of ltr_plan.h over
grids and batches that reach every class boundary and every schedule, dumped once per library in a child process (LTR_GPU_LIB) and
compared byte for byte.

    python tests/manual/plan_units_ab.py BEFORE.so AFTER.so [--out profiles/plan_units_ab.json] [--fold-literals]

--fold-literals prints, from the FIRST library, the class sizes the fold-walk cases of tests/test_plan_units.py expect."""
import argparse
import ctypes as C
import json
import os
import pickle
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ASYM = (-1.2, -0.3, -0.9, -0.5, -0.0001, -5.0, -4.0)
SCHEDULES = {"plan kernel": dict(), "multi-width": dict(plan_kernel=1, no_multi=-1), "per class": dict(plan_kernel=1, no_multi=1)}   # tests/test_gpu_plan_schedule.py
N_CUS = (1, 4, 256)
FOLD_N_CU = 256


def blob(x):
    """Canonical bytes of a hook's result."""
    if isinstance(x, np.ndarray):
        return b"A" + str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, dict):
        return b"D" + b"".join(blob(k) + blob(v) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return b"L" + struct.pack("<q", len(x)) + b"".join(blob(v) for v in x)
    if isinstance(x, (bool, np.bool_)):
        return b"B" + (b"1" if x else b"0")
    if isinstance(x, (int, np.integer)):
        return b"I" + struct.pack("<q", int(x))
    if isinstance(x, (float, np.floating)):
        return b"F" + struct.pack("<d", float(x))
    if isinstance(x, str):
        return b"S" + x.encode()
    if x is None:
        return b"N"
    raise TypeError(type(x))


def fold_cases(class_of):
    """name -> list of (class, pairs): the hand-made class counts of tests/test_plan_units.py for the fold walk of each family."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_plan_units import FOLD_CASES
    return {name: [(class_of(*c), n) for c, n in case] for name, case in FOLD_CASES.items()}


def fold_arrays(case):
    cls = np.concatenate([np.full(n, k, dtype=np.int16) for k, n in case])
    return cls, (np.arange(len(cls)) % 500 + 1).astype(np.int16)


def random_batches():
    from longtr_amd import _abi
    rng = np.random.default_rng(20261019)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    lengths = (40, 41, 100, 257, 322, 500, 641, 642, 700, 1000, 1281, 1282, 1400, 2600, 3586, 3700, 4900, 5122, 8000, 10242, 11000)

    def locus(m, n_reads, n_haps, shared=0.5):
        core = seq(m)
        cut = int(m * shared)
        haps = [seq(30) + core + seq(30)] + [seq(30) + core[:cut] + seq(5 + 40 * h) + core[cut:] + seq(30) for h in range(n_haps - 1)]
        reads = []
        for _ in range(n_reads):
            r = bytearray(core)
            for p in rng.choice(m, size=min(3, m), replace=False):
                r[p] = ord("A") if r[p] != ord("A") else ord("C")
            reads.append(bytes(r[:max(2, m + int(rng.integers(-20, 1)))]))
        if rng.random() < 0.15:
            reads[0] = reads[0][:1] + b"N" + reads[0][2:]
        if rng.random() < 0.15:
            haps.append(b"ACGT" * 10)
        if rng.random() < 0.1:
            reads.append(seq(m + 700))
        return reads, haps

    out = {}
    out["mixed"] = _abi.PackedBatch([locus(int(rng.choice(lengths)), int(rng.integers(1, 9)), int(rng.integers(1, 7)), float(rng.uniform(0.05, 0.95))) for _ in range(160)])
    out["short"] = _abi.PackedBatch([locus(int(rng.integers(40, 700)), int(rng.integers(4, 30)), int(rng.integers(2, 9))) for _ in range(300)])
    out["families"] = _abi.PackedBatch([locus(int(rng.integers(322, 1282)), 4, int(rng.integers(2, 5)), 0.7) for _ in range(120)] +
                                       [locus(41, 20, 14) for _ in range(30)])
    out["long"] = _abi.PackedBatch([locus(int(rng.choice((3700, 4300, 4900, 5200, 8000, 11000))), int(rng.integers(1, 5)), int(rng.integers(1, 4))) for _ in range(60)])
    return out


def synth_batches():
    from longtr_amd import synth
    out = {}
    for name, n in (("config2", 1), ("config3", 700), ("config3skew", 300), ("config5", 8), ("config5hifi", 64), ("catalogue", 3000)):
        loci, _ = synth.config_loci(name, n_loci=n, workers=1)
        out[f"{name}/{n}"] = synth.pack_loci(loci)[0]
    return out


def dump(path, want_fold_literals):
    from longtr_amd import _abi, _lib
    L = _lib.lib()
    NK = L.ltr_debug_num_classes()
    res = {}

    info = []
    for k in range(NK):
        v = [C.c_int(0) for _ in range(4)]
        assert L.ltr_debug_class_info(k, *[C.byref(x) for x in v]) == 0
        info.append(tuple(x.value for x in v))
    res["class_info"] = blob(info)
    class_of = lambda family, W, lanes: next(k for k in range(NK) if info[k][0] == family and info[k][1] == W and info[k][3] == lanes)

    # ---- ltr_debug_classify / ltr_debug_pair_costs: every class boundary (lanes x strip width, the column blocks, the exact lists' and the
    # workgroup families' limits), length differences at the shortcut and at the risky_dd thresholds of both models
    cols = {1, 2, 3, 60, 61, 1280, 2560, 2561, 3584, 3585, 5120, 5121, 10240, 10241, 10999}
    for lanes in (2, 4, 8, 16, 32, 64, 128, 256, 512):
        for W in range(1, 21):
            cols.update((lanes * W - 1, lanes * W, lanes * W + 1))
    cols = sorted(c for c in cols if 1 <= c <= 11000)
    dds = (-601, -600, -574, -573, -511, -510, -430, -429, -1, 0, 1, 429, 430, 510, 511, 573, 574, 600, 601)
    grid = [(max(m + dd, 2), m, max(m + dd, 2) + 60, g) for m in (c + 1 for c in cols) for dd in dds for g in (0, 1) if m + dd >= 2]
    grid += [(0, c + 1, hl, 0) for c in cols[::7] for hl in (40, 60)]                       # hap_full_len <= 60: the constant-score shortcut
    win, rl, hfl = (np.asarray([g[i] for g in grid], dtype=np.int32) for i in range(3))
    n_grid = 0
    for pname, prm in (("sym", _abi.default_params()), ("asym", _abi.make_params(ASYM))):
        for mode in range(-1, 9):
            for n_cu in (N_CUS if mode == -1 else (256,)):
                for pairs, long_pairs in ((1 << 21, 1 << 20), (1 << 21, 100), (3000, 0), (40 * n_cu, 3)):
                    out = np.zeros((len(grid), 3), dtype=np.int32)
                    cls, key, xl = C.c_int(-1), C.c_int(-1), C.c_int(-1)
                    for i, (n, m, hl, g) in enumerate(grid):
                        assert L.ltr_debug_classify(C.byref(prm), mode, n_cu, pairs, long_pairs, n, m, hl, g, C.byref(cls), C.byref(key), C.byref(xl)) == 0
                        out[i] = (cls.value, key.value, xl.value)
                    cost = np.zeros(len(grid))
                    assert L.ltr_debug_pair_costs(C.byref(prm), mode, n_cu, pairs, long_pairs, len(grid), win.ctypes.data, rl.ctypes.data, hfl.ctypes.data, cost.ctypes.data) == 0
                    res[f"classify {pname} mode {mode} n_cu {n_cu} pairs {pairs}/{long_pairs}"] = blob(out)
                    res[f"pair_costs {pname} mode {mode} n_cu {n_cu} pairs {pairs}/{long_pairs}"] = blob(cost)
                    n_grid += len(grid)

    # ---- ltr_debug_threshold_table: bounds inside and beyond the table (600 / 1023 = 0.5865), no bound at all
    for c in (-1.0, -0.25, -0.9, -3.7, -0.5864, -0.5865, -0.5866, -0.59, -0.6, -1e-3, -5e-7, -700.0):
        tab = np.zeros(4096)
        n = L.ltr_debug_threshold_table(C.c_float(c), tab.ctypes.data, len(tab))
        res[f"threshold_table {c}"] = blob([n, tab[:max(n, 0)]])

    # ---- ltr_debug_sort_by_class
    def sort(cls, key, fold, n_cu):
        order = np.zeros(len(cls), dtype=np.int32); first = np.zeros(NK + 1, dtype=np.int32)
        assert L.ltr_debug_sort_by_class(cls.ctypes.data, key.ctypes.data, len(cls), fold, n_cu, order.ctypes.data, first.ctypes.data) == 0
        return order, first
    rng = np.random.default_rng(5)
    for n in (0, 1, 5000, 300000):
        cls = rng.integers(0, NK, size=n).astype(np.int16)
        key = rng.integers(0, 512, size=n).astype(np.int16)
        for fold in range(4):
            for n_cu in N_CUS:
                res[f"sort random {n} fold {fold} n_cu {n_cu}"] = blob(list(sort(cls, key, fold, n_cu)))
    literals = {}
    for name, case in fold_cases(class_of).items():
        cls, key = fold_arrays(case)
        for fold in range(4):
            order, first = sort(cls, key, fold, FOLD_N_CU)
            res[f"sort fold case {name} fold {fold}"] = blob([order, first])
            literals[(name, fold)] = {int(k): int(first[k + 1] - first[k]) for k in range(NK) if first[k + 1] > first[k]}
    if want_fold_literals:
        print("FOLD_EXPECTED = {")
        for (name, fold), sizes in literals.items():
            if fold:
                print(f"    ({name!r}, {fold}): {sizes},")
        print("}")

    # ---- describe_batch, the schedule, the families
    def call(f, *a, **kw):
        try:
            return f(*a, **kw)
        except _lib.LtrError as e:
            return ("error", e.code, str(e))
    batches = dict(random_batches(), **synth_batches())
    n_desc = 0
    for bname, batch in batches.items():
        for pname, prm in (("sym", _abi.default_params()), ("asym", _abi.make_params(ASYM))):
            for mode in range(-1, 9):
                for n_cu in N_CUS:
                    what = f"{bname} {pname} mode {mode} n_cu {n_cu}"
                    res[f"describe {what}"] = blob(call(_lib.debug_describe_batch, batch, params=prm, mode=mode, n_cu=n_cu))
                    grids = np.full(NK + 3, 8 * n_cu, dtype=np.int32)
                    for sname, knobs in SCHEDULES.items():
                        for chain in (0, 1):
                            res[f"schedule {what} {sname} chain {chain}"] = blob(call(_lib.debug_plan_schedule, batch, grids, params=prm, mode=mode, n_cu=n_cu, chain=chain, **knobs))
                    for fam in (-1, 0, 1, 2):
                        res[f"families {what} families {fam}"] = blob(call(_lib.debug_plan_families, batch, params=prm, mode=mode, n_cu=n_cu, families=fam))
                    n_desc += 1
    meta = dict(lib=_lib.LIB_PATH, classify_points=n_grid, batches={k: int(b.ll_size) for k, b in batches.items()}, settings_per_batch=n_desc // max(len(batches), 1))
    with open(path, "wb") as f:
        pickle.dump((meta, res), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--out")
    ap.add_argument("--labels", nargs=2, default=["before", "after"], help="what the two libraries are called in the result")
    ap.add_argument("--fold-literals", action="store_true")
    ap.add_argument("--dump")
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump, a.fold_literals)
    assert len(a.libs) == 2, "two library paths"
    dumps = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(a.libs):
            out = os.path.join(tmp, f"{i}.pkl")
            cmd = [sys.executable, os.path.abspath(__file__), "--dump", out] + (["--fold-literals"] if a.fold_literals and i == 0 else [])
            subprocess.run(cmd, check=True, env=dict(os.environ, LTR_GPU_LIB=os.path.abspath(lib)), cwd=ROOT)
            dumps.append(pickle.load(open(out, "rb")))
    (meta_a, A), (meta_b, B) = dumps
    assert meta_a["lib"] != meta_b["lib"] or a.libs[0] == a.libs[1]
    bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    by_hook = {}
    for k in A:
        by_hook[k.split()[0]] = by_hook.get(k.split()[0], 0) + 1
    result = dict(before=a.labels[0], after=a.labels[1], cases=len(A), cases_by_hook=by_hook, classify_points=meta_a["classify_points"],
                  batches=meta_a["batches"], settings_per_batch=meta_a["settings_per_batch"], mismatches=len(bad), mismatched=bad[:50])
    print(json.dumps(result, indent=1))
    if a.out:
        prev = json.load(open(a.out)) if os.path.exists(a.out) else {}
        prev["cpu_hooks"] = result
        json.dump(prev, open(a.out, "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
