"""What hipcc made of the family kernel (csrc/ltr_dp_family.hpp), read off the gfx950 assembly (tests/isa_util.py; no GPU): the ten
strip widths of family_walk_call at three waves per SIMD, no scratch access and no atomic inside a wavefront step."""
import os
import re

import pytest

import isa_util

CACHE = os.path.join(isa_util.CSRC, "build", "isa")


@pytest.fixture(scope="module")
def funcs():
    return isa_util.analyse("ltr_k_family.hip", cache_dir=CACHE)


def _walks(funcs):
    return {int(re.search(r"<(\d+)>", n).group(1)): v for n, v in funcs.items() if re.search(r"\bfamily_walk_call<", n)}


def test_ten_strip_widths_at_three_waves_per_simd(funcs):
    walks = _walks(funcs)
    assert sorted(walks) == list(range(11, 21))
    for w, v in walks.items():
        assert v["vgprs"] <= 168, (w, v["vgprs"])
    (kernel,) = [v for n, v in funcs.items() if n.startswith("ltr_dp_family_kernel")]
    assert kernel["vgprs"] <= 168 and kernel["group_segment_fixed_size"] <= 160 * 1024 // 3      # three workgroups per CU
    # the exact bodies it calls for the members it cannot accept (ltr_dp_redo.hpp), under the same budget
    for base in ("redo_thr_call", "redo_generic_call"):
        sel = [v for n, v in funcs.items() if re.search(r"\b%s<" % base, n)]
        assert sel and all(v["vgprs"] <= 168 for v in sel), base


def test_no_scratch_and_no_atomic_inside_a_wavefront_step(funcs):
    """The stem's and the tails' step loops: 11 FP64 operations per column and nothing else that waits.  The member loop around the
    tail holds the peeled last step (12 operations per column: the result capture) behind the member's set-up: no scratch access
    between the first and the last FP64 operation of that loop -- what the wide bodies reload (one pointer) is reloaded at its head."""
    asm = isa_util.assembly("ltr_k_family.hip", cache_dir=CACHE).splitlines()
    checked = 0
    for w, v in _walks(funcs).items():
        steps = [L for L in v["step_loops"] if 11 * w <= L["fp64"] < 12 * w]
        assert len(steps) == 2, (w, v["step_loops"])              # the stem, the tail
        for L in steps:
            assert L["scratch"] == 0 and L["atomics"] == 0 and L["lane_moves"] == 0, (w, L)
            checked += 1
        start = next(i for i, l in enumerate(asm) if re.match(r"^\s*\.type\s+%s,@function" % re.escape(v["mangled"]), l))
        last = [L for L in v["step_loops"] if L["fp64"] >= 12 * w]
        assert len(last) == 1, (w, v["step_loops"])
        for L in last:
            seg = asm[start + L["first"]:start + L["last"] + 1]
            fp = [i for i, x in enumerate(seg) if isa_util._FP64.match(x)]
            inside = [x.strip() for i, x in enumerate(seg) if fp[0] <= i <= fp[-1] and (isa_util._SCRATCH.match(x) or isa_util._ATOMIC.match(x))]
            assert inside == [] and L["scratch"] <= 1 and L["atomics"] == 0, (w, L, inside)
            checked += 1
        # its counters: plain adds nobody waits for (no return value) -- nothing here pops a queue
        assert all(not p["returns"] for p in isa_util.pop_sites("\n".join(asm), v["mangled"])), w
    assert checked == 30
