"""ltr_editdist_kernel (longtr_amd/csrc/ltr_editdist.hip) as hipcc builds it for gfx950: the kernel exists and touches no scratch memory
(no private arrays, no spills).  Registers and occupancy are recorded in DESIGN section 3."""
import isa_util


def test_editdist_kernel_uses_no_scratch(tmp_path):
    f = isa_util.analyse("ltr_editdist.hip", cache_dir=str(tmp_path))
    kernels = {n: v for n, v in f.items() if "ltr_editdist_kernel" in n}
    assert len(kernels) == 1, list(f)
    for n, v in kernels.items():
        print(n, {k: v.get(k) for k in ("vgprs", "sgprs", "scratch", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")})
        assert v["scratch"] == 0 and v["scratch_accesses"] == 0, (n, v["scratch"])
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, n
