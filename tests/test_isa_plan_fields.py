"""ltr_genotype_fields_kernel (longtr_amd/csrc/ltr_plan_fields.hip) as hipcc builds it for gfx950: both workgroup sizes exist and
neither touches scratch memory (no private arrays, no spills).  Registers and occupancy are recorded in DESIGN section 3."""
import isa_util


def test_fields_kernel_uses_no_scratch(tmp_path):
    f = isa_util.analyse("ltr_plan_fields.hip", cache_dir=str(tmp_path))
    kernels = {n: v for n, v in f.items() if "ltr_genotype_fields_kernel" in n}
    assert sorted(n[n.index("<"):n.index(">") + 1] for n in kernels) == ["<256>", "<64>"], list(f)
    for n, v in kernels.items():
        print(n, {k: v.get(k) for k in ("vgprs", "sgprs", "scratch", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")})
        assert v["scratch"] == 0 and v["scratch_accesses"] == 0, (n, v["scratch"])
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, n
