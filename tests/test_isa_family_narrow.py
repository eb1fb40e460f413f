"""What hipcc made of the family kernel's narrow bodies (csrc/ltr_dp_family.hpp, family_narrow_call<6 .. 10>: reads of 321 .. 640
columns), read off the gfx950 assembly (tests/isa_util.py; no GPU): five strip widths within the kernel's three waves per SIMD, no
scratch access, no atomic and no lane move inside a wavefront step."""
import os
import re

import pytest

import isa_util

CACHE = os.path.join(isa_util.CSRC, "build", "isa")


@pytest.fixture(scope="module")
def funcs():
    return isa_util.analyse("ltr_k_family.hip", cache_dir=CACHE)


def _narrow(funcs):
    return {int(re.search(r"<(\d+)>", n).group(1)): v for n, v in funcs.items() if re.search(r"\bfamily_narrow_call<", n)}


def test_five_narrow_strip_widths_within_the_kernels_budget(funcs):
    walks = _narrow(funcs)
    assert sorted(walks) == [6, 7, 8, 9, 10]
    for w, v in walks.items():
        print("family_narrow_call<%d>: %d VGPRs, %d bytes of scratch" % (w, v["vgprs"], v.get("scratch", 0)))
        assert v["vgprs"] <= 168, (w, v["vgprs"])
    (kernel,) = [v for n, v in funcs.items() if n.startswith("ltr_dp_family_kernel")]
    assert kernel["vgprs"] <= 168 and kernel["group_segment_fixed_size"] <= 160 * 1024 // 3      # three workgroups per CU


def test_no_scratch_no_atomic_and_no_lane_move_inside_a_wavefront_step(funcs):
    """The stem's and the tail's step loops hold 11 FP64 operations per column (the peeled last step of a tail, which captures the
    result, holds 12 and is not one of them)."""
    checked = 0
    for w, v in _narrow(funcs).items():
        steps = [L for L in v["step_loops"] if 11 * w <= L["fp64"] < 12 * w]
        assert len(steps) == 2, (w, v["step_loops"])              # the stem, the tail
        for L in steps:
            assert L["scratch"] == 0 and L["atomics"] == 0 and L["lane_moves"] == 0, (w, L)
            checked += 1
    assert checked == 10
