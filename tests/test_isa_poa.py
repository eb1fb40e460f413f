"""ltr_poa_kernel (longtr_amd/csrc/ltr_poa.hip) as hipcc builds it for gfx950: the kernel exists, and the loop that computes a row of scores --
the one with the max-scan across the lanes -- makes no scratch access, nor does any other loop.  Whole-kernel registers, scratch and
occupancy are recorded in DESIGN section 3 (K6), not asserted."""
import re

import isa_util


def test_poa_kernel_exists_and_its_row_loop_uses_no_scratch(tmp_path):
    asm = isa_util.assembly("ltr_poa.hip", cache_dir=str(tmp_path))
    f = isa_util.parse(asm)
    kernels = {n: v for n, v in f.items() if "ltr_poa_kernel" in n}
    assert len(kernels) == 1, list(f)
    (name, v), = kernels.items()
    meta = {k: m for k, m in isa_util.kernel_spills(asm).items() if "ltr_poa_kernel" in k}
    print(name, {k: v.get(k) for k in ("vgprs", "sgprs", "scratch", "scratch_accesses")}, meta)
    assert ".amdgcn_target" in asm and "gfx950" in asm
    # the function's own lines, as isa_util.parse cuts them
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^\s*\.type\s+%s,@function" % re.escape(v["mangled"]), l))
    body = lines[start:]
    scan = re.compile(r"^\s*(ds_bpermute_b32|v_\w+_dpp|v_mov_b32_dpp)")
    row_loops = []
    for loop in v["loops"]:
        seg = body[loop["first"]:loop["last"] + 1]
        assert loop["scratch"] == 0, (loop["first"], loop["last"])
        if sum(1 for l in seg if scan.match(l)) >= 6 and any(re.match(r"^\s*v_max_i32", l) for l in seg):
            row_loops.append(loop)
    assert row_loops, "no loop with the six-step max-scan: the row loop was not found"
    assert all(loop["scratch"] == 0 for loop in row_loops)
