"""The debug_* test hooks: the host half of planning on made-up numbers, no GPU."""
import ctypes as C

import numpy as np

from . import _abi
from ._loader import LtrError, _p, lib


def debug_describe_batch(batch, params=None, mode=-1, n_cu=256):
    """Test hook ltr_debug_describe_batch (csrc/ltr_plan.h): the host half of ltr_plan_create on a _abi.PackedBatch, no GPU.  dict(n_pairs,
    ll_size, max_len, cells, input_bytes, class_first, and per SORTED pair n, m, out_idx, key) or LtrError with the library's text."""
    L = lib()
    prm = params or _abi.default_params()
    cap = int(np.sum(np.diff(batch.locus_read_off) * np.diff(batch.locus_hap_off))) if batch.n_loci > 0 else 0
    cap = max(cap, 1)
    i64, f64 = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.float64)
    first = np.zeros(L.ltr_debug_num_classes() + 1, dtype=np.int32)
    n, m, key = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int16)
    out_idx = np.zeros(cap, dtype=np.int64)
    err = C.create_string_buffer(512)
    rc = L.ltr_debug_describe_batch(C.byref(prm), int(mode), int(n_cu), C.byref(batch.struct), _p(i64), _p(f64), _p(first), cap, _p(n), _p(m), _p(out_idx), _p(key), err, len(err))
    if rc != 0:
        raise LtrError(rc, err.value.decode())
    k = int(i64[0])
    return dict(n_pairs=k, ll_size=int(i64[1]), max_len=int(i64[2]), cells=float(f64[0]), input_bytes=float(f64[1]), class_first=first,
                n=n[:k], m=m[:k], out_idx=out_idx[:k], key=key[:k])


def debug_threshold_groups(class_first, merge=True, keep_waves=False):
    """Test hook ltr_debug_threshold_groups (ltrp::threshold_groups): per class (waves, strip width, pairs of the launch it leads)."""
    L = lib()
    first = np.ascontiguousarray(class_first, dtype=np.int32)
    nk = L.ltr_debug_num_classes()
    assert first.size == nk + 1
    nw, w, npairs = (np.zeros(nk, dtype=np.int32) for _ in range(3))
    rc = L.ltr_debug_threshold_groups(_p(first), int(bool(merge)), int(bool(keep_waves)), _p(nw), _p(w), _p(npairs))
    if rc != 0:
        raise LtrError(rc, "ltr_debug_threshold_groups")
    return nw, w, npairs


LAUNCH_KINDS = ("one-wave", "packed", "multi", "packed-multi", "plan", "workgroup", "family")      # ltrp::LaunchKind


def debug_plan_schedule(batch, grids, params=None, mode=-1, n_cu=256, plan_kernel=0, no_multi=0, chain=0, chain_min_w=0, chain_max_w=0,
                        plan_share=0, cap=0, grid_cap=0):
    """Test hook ltr_debug_plan_schedule (csrc/ltr_plan.h): describe_batch, class statistics and ltrp::build_schedule on a
    _abi.PackedBatch, no GPU.  grids: made-up occupancy grids, one per class (certificate, then exact), then of the multi-width
    one-wave launch, the multi-width packed launch and the plan kernel.  dict(launches, by_class: lists of dict(kind, cls, W,
    grid, small, cmax, pairs, cells, members); entries: list of dict(kind, W, first, pairs, queue_class, first_wave); n_tabs,
    use_plan, max_grid, max_grid_wide, max_len, xcand, class_first, x_grid).  cap: Schedule::cap_grids (the scratch strips' cap);
    grid_cap: the ltr_ctx_set_debug switch of that name (Schedule::cap_every_grid); one of the two at a time."""
    L = lib()
    nk = L.ltr_debug_num_classes()
    g = np.ascontiguousarray(grids, dtype=np.int32)
    assert g.size == nk + 3
    assert cap >= 0 and grid_cap >= 0 and not (cap and grid_cap)      # (one knob: the sign picks the cap)
    knobs = np.asarray([plan_kernel, no_multi, chain, chain_min_w, chain_max_w, plan_share, -grid_cap if grid_cap else cap], dtype=np.int32)
    prm = params or _abi.default_params()
    n_exact = nk - sum(1 for k in range(nk) if L.ltr_kernel_family(k) != 3)
    out, x_grid = np.zeros(8 + n_exact + nk + 1, dtype=np.int64), np.zeros(n_exact, dtype=np.int32)
    lcap, mcap, ecap = 2 * nk, 2 * nk + 128, 256
    launch, cells, members, entry = np.zeros((lcap, 8), np.int32), np.zeros(lcap), np.zeros(mcap, np.int32), np.zeros((ecap, 6), np.int32)
    rc = L.ltr_debug_plan_schedule(C.byref(prm), int(mode), int(n_cu), C.byref(batch.struct), _p(g), _p(knobs), _p(out), _p(x_grid),
                                   lcap, _p(launch), _p(cells), mcap, _p(members), ecap, _p(entry))
    if rc != 0:
        raise LtrError(rc, "ltr_debug_plan_schedule")
    rows, at = [], 0
    for i in range(int(out[0] + out[1])):
        kind, cls, w, grid, small, cmax, pairs, nm = (int(v) for v in launch[i])
        rows.append(dict(kind=LAUNCH_KINDS[kind], cls=cls, W=w, grid=grid, small=bool(small), cmax=cmax, pairs=pairs, cells=float(cells[i]),
                         members=[int(m) for m in members[at:at + nm]]))
        at += nm
    ents = [dict(zip(("kind", "W", "first", "pairs", "queue_class", "first_wave"), (int(v) for v in entry[i]))) for i in range(int(out[2]))]
    return dict(launches=rows[:int(out[0])], by_class=rows[int(out[0]):], entries=ents, n_tabs=int(out[3]), use_plan=bool(out[4]),
                max_grid=int(out[5]), max_grid_wide=int(out[6]), max_len=int(out[7]), xcand=out[8:8 + n_exact].copy(), class_first=out[8 + n_exact:].copy(), x_grid=x_grid)


def debug_plan_families(batch, params=None, mode=-1, n_cu=256, families=0, family_min_rows=0):
    """Test hook ltr_debug_plan_families (csrc/ltr_plan.h): describe_batch on a _abi.PackedBatch, no GPU; families / family_min_rows
    are the ltr_ctx_set_debug knobs of the same names.  dict(families: list of dict(first, count, p, W, dd_min, dd_max, U, n: window
    lengths of the members, out_idx: their LL indices), members, n_pairs)."""
    L = lib()
    prm = params or _abi.default_params()
    knobs = np.asarray([families, family_min_rows], dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    cap = max(int(batch.ll_size), 1)
    fam, U = np.zeros((cap, 6), np.int32), np.zeros(cap)
    mem_n, mem_out = np.zeros(cap, np.int32), np.zeros(cap, np.int64)
    rc = L.ltr_debug_plan_families(C.byref(prm), int(mode), int(n_cu), C.byref(batch.struct), _p(knobs), _p(out), cap, _p(fam), _p(U), cap, _p(mem_n), _p(mem_out))
    if rc != 0:
        raise LtrError(rc, "ltr_debug_plan_families")
    rows = []
    for i in range(int(out[0])):
        d = dict(zip(("first", "count", "p", "W", "dd_min", "dd_max"), (int(v) for v in fam[i])))
        a = d["first"] - int(out[2])
        d.update(U=float(U[i]), n=[int(v) for v in mem_n[a:a + d["count"]]], out_idx=[int(v) for v in mem_out[a:a + d["count"]]])
        rows.append(d)
    return dict(families=rows, members=int(out[1]), n_pairs=int(out[3]))


def debug_plan_family_forks(batch, params=None, mode=-1, n_cu=256, families=0, family_min_rows=0, family_spine=0):
    """Test hook ltr_debug_plan_family_forks (csrc/ltr_plan.h): describe_batch on a _abi.PackedBatch, no GPU, for the spines of its
    families; family_spine is the ltr_ctx_set_debug knob of that name.  dict(families: list of dict(spine: member or -1, slots, steps,
    slot_rows, first, count, p, W, dd_min, dd_max, fork: per member, slot: per member, out_idx: per member), members, with_spine,
    steps_saved, park_slots)."""
    L = lib()
    prm = params or _abi.default_params()
    knobs = np.asarray([families, family_min_rows, family_spine], dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    cap = max(int(batch.ll_size), 1)
    fam, slot_row = np.zeros((cap, 10), np.int32), np.zeros(cap * 16, np.int32)
    fork, slot, mem_out = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
    rc = L.ltr_debug_plan_family_forks(C.byref(prm), int(mode), int(n_cu), C.byref(batch.struct), _p(knobs), _p(out), cap, _p(fam), _p(slot_row),
                                       cap, _p(fork), _p(slot), _p(mem_out))
    if rc != 0:
        raise LtrError(rc, "ltr_debug_plan_family_forks")
    n_slots = int(fam[0, 3]) if out[0] else 0
    assert n_slots <= 16
    rows, at = [], 0
    for i in range(int(out[0])):
        d = dict(zip(("spine", "slots", "steps", "park_slots", "first", "count", "p", "W", "dd_min", "dd_max"), (int(v) for v in fam[i])))
        d.update(slot_rows=[int(v) for v in slot_row[i * n_slots:i * n_slots + d["slots"]]], fork=[int(v) for v in fork[at:at + d["count"]]],
                 slot=[int(v) for v in slot[at:at + d["count"]]], out_idx=[int(v) for v in mem_out[at:at + d["count"]]])
        at += d["count"]
        rows.append(d)
    return dict(families=rows, members=int(out[1]), with_spine=int(out[2]), steps_saved=int(out[3]), park_slots=n_slots)


# ltrp::LaunchKind, then the kinds of the launches formed at execute time (csrc/ltr_plan.h, kNote*)
LAUNCH_NOTE_KINDS = LAUNCH_KINDS + ("threshold", "exact", "exact-wide", "exact-narrow8", "nw-wave", "nw-workgroup")


def debug_last_launches(plan=None, ctx=None):
    """Test hook ltr_debug_last_launches (csrc/ltr_plan.h): every kernel launch of the last execute of a Plan, or (plan None) of the
    last haplotype_align_to_ref of a Context, as it was made.  List of dict(kind: one of LAUNCH_NOTE_KINDS, cls, grid, takers: per
    workgroup, wavefronts (or the workgroup itself) that take items independently, items: what the launch was given, -1 where only
    the device knows)."""
    L = lib()
    hp, hc = (plan._h if plan is not None else None), (ctx._h if ctx is not None else None)
    out = np.zeros((64, 5), dtype=np.int64)
    n = L.ltr_debug_last_launches(hp, hc, out.shape[0], _p(out))
    if n > out.shape[0]:
        out = np.zeros((n, 5), dtype=np.int64)
        n = L.ltr_debug_last_launches(hp, hc, out.shape[0], _p(out))
    if n < 0:
        raise LtrError(n, "ltr_debug_last_launches")
    return [dict(kind=LAUNCH_NOTE_KINDS[int(r[0])], cls=int(r[1]), grid=int(r[2]), takers=int(r[3]), items=int(r[4])) for r in out[:n]]


def debug_chunk_plan(n_loci, est_cells=0.0, budget=0, chunks=0, chunk_streams=0, chunk_growth=None, prep_ahead=0):
    """Test hook ltr_debug_chunk_plan (csrc/ltr_internal.h): the chunk rule of ltr_calc_hap_aln_probs on made-up numbers, no GPU.
    The keywords are the ltr_ctx_set_debug knobs of the same names (chunk_growth=None: not set); budget 0 = the process's.
    dict(bounds, n_streams, prep_ahead, ahead_threads)."""
    L = lib()
    knobs = np.asarray([chunks, chunk_streams, chunk_growth or 0.0, chunk_growth is not None, prep_ahead], dtype=np.float64)
    cap = max(int(chunks), 8) + 2
    bounds, out = np.zeros(cap, dtype=np.int64), np.zeros(4, dtype=np.int32)
    rc = L.ltr_debug_chunk_plan(int(n_loci), float(est_cells), _p(knobs), int(budget), _p(bounds), cap, _p(out))
    if rc != 0:
        raise LtrError(rc, "ltr_debug_chunk_plan")
    return dict(bounds=[int(b) for b in bounds[:int(out[0]) + 1]], n_streams=int(out[1]), prep_ahead=bool(out[2]), ahead_threads=int(out[3]))

