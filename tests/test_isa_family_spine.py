"""What hipcc made of the family kernel's spine bodies (csrc/ltr_dp_family.hpp, spine_narrow_call<6 .. 10> and spine_wide_call<11 ..
20>: families run along a spine), read off the gfx950 assembly (tests/isa_util.py; no GPU): every strip width within the kernel's
three waves per SIMD, and no scratch access and no atomic inside a wavefront step -- the stream's loop, which also holds the parking
stores, and the tails' loops."""
import os
import re

import pytest

import isa_util

CACHE = os.path.join(isa_util.CSRC, "build", "isa")


@pytest.fixture(scope="module")
def funcs():
    return isa_util.analyse("ltr_k_family.hip", cache_dir=CACHE)


def _spine(funcs):
    return {int(re.search(r"<(\d+)>", n).group(1)): v for n, v in funcs.items() if re.search(r"\bspine_(narrow|wide)_call<", n)}


def test_fifteen_strip_widths_within_the_kernels_budget(funcs):
    walks = _spine(funcs)
    assert sorted(walks) == list(range(6, 21))
    assert sorted(int(re.search(r"<(\d+)>", n).group(1)) for n in funcs if re.search(r"\bspine_narrow_call<", n)) == [6, 7, 8, 9, 10]
    for w, v in sorted(walks.items()):
        print("spine call<%d>: %d VGPRs, %d bytes of scratch" % (w, v["vgprs"], v.get("scratch", 0)))
        assert v["vgprs"] <= 168, (w, v["vgprs"])
    (kernel,) = [v for n, v in funcs.items() if n.startswith("ltr_dp_family_kernel")]
    assert kernel["vgprs"] <= 168 and kernel["group_segment_fixed_size"] <= 160 * 1024 // 3      # three workgroups per CU


def test_no_scratch_and_no_atomic_inside_a_wavefront_step(funcs):
    """Three loops hold wavefront steps: the stream (11 FP64 operations per column, and the stores of a park row behind a branch),
    a tail's steps (11 per column) and the loop over the members around a tail's peeled last step (12 per column)."""
    checked = 0
    for w, v in _spine(funcs).items():
        steps = [L for L in v["step_loops"] if L["fp64"] >= 11 * w]
        assert len(steps) == 3 and len(steps) == len(v["step_loops"]), (w, v["step_loops"])
        for L in steps:
            assert L["scratch"] == 0 and L["atomics"] == 0, (w, L)
            checked += 1
    assert checked == 45
