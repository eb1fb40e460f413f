"""The signature table of longtr_amd/_abi.py against include/ltr_gpu.h, and the surface of the longtr_amd._lib facade.  No GPU."""
import ctypes as C
import os
import re
import types

from longtr_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


def header_declarations():
    """[(return type, name, [parameter, ...])] of every `return-type ltr_name(params);` in the header, comments stripped."""
    src = open(os.path.join(ROOT, "include", "ltr_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = []
    for m in re.finditer(r"([A-Za-z_][\w \t\n\*]*?)\b(ltr_\w+)\s*\(([^()]*)\)\s*;", src):
        ret = " ".join(m.group(1).split())
        if ret.startswith("define LTR_ABI_VERSION"):             # (the match that begins inside the #define line above ltr_abi_version)
            assert m.group(2) == "ltr_abi_version"
            ret = ret.split()[-1]
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        out.append((ret, m.group(2), [] if params == ["void"] else params))
    return out


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def check_type(c_type, ct, where):
    """c_type: the declared C type (names of parameters removed); ct: the table's ctypes type."""
    c_type = c_type.replace("const", " ").replace("struct", " ")
    if "*" in c_type or "[" in c_type:
        assert is_pointer(ct), (where, c_type, ct)
    else:
        base = c_type.split()
        assert len(base) == 1 and base[0] in SCALARS, (where, c_type)
        assert ct is SCALARS[base[0]], (where, c_type, ct)


def test_table_matches_the_header():
    decls = header_declarations()
    assert len(decls) == 179 and len({d[1] for d in decls}) == 179
    assert [d for d in decls if d[1] == "ltr_abi_version"] == [("int", "ltr_abi_version", [])]
    assert {d[1] for d in decls} == set(_abi.SIGNATURES) and not set(_abi.SIGNATURES) & set(_abi.HOOK_SIGNATURES)
    for ret, name, params in decls:
        restype, argtypes = _abi.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        check_type(ret, restype, name)
        for i, (p, ct) in enumerate(zip(params, argtypes)):
            assert "(" not in p, (name, p)                       # no function-pointer parameter
            m = re.match(r"(.*?)(\w+)\s*(\[\d*\])?$", p)          # type, parameter name, array suffix
            check_type(m.group(1) + (m.group(3) or ""), ct, (name, i))


def test_exports_are_the_table_in_order():
    assert _lib.EXPORTS == list(_abi.SIGNATURES)


def test_lib_applies_the_table_to_every_function():
    L = _lib.lib()
    for table in (_abi.SIGNATURES, _abi.HOOK_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            assert fn.restype is restype, name
            assert list(fn.argtypes) == list(argtypes), name


# sorted(n for n, v in vars(_lib).items() if not n.startswith("__") and not isinstance(v, types.ModuleType)) on the commit before the split
SURFACE = ['Bam', 'BamRecord', 'CSRC', 'Context', 'EXPORTS', 'FAMILIES', 'Fasta', 'GenotypeResult', 'HERE', 'HIPCC_FLAGS', 'KERNEL_TUS',
           'LAUNCH_KINDS', 'LIB_PATH', 'LINK_LIBS', 'LtrError', 'OBJ_DIR', 'PLAN_UNITS', 'Plan', 'ReadSet', 'SOURCES', 'VcfPanel', 'VcfWriter',
           '_bind_genotype', '_hap_result', '_lib', '_locus_haploid', '_p', 'build', 'cluster_sequences', 'debug_chunk_plan',
           'debug_describe_batch', 'debug_plan_families', 'debug_plan_family_forks', 'debug_plan_schedule', 'debug_threshold_groups',
           'edit_distances', 'extract_genotypes', 'get_alleles', 'haplotype_seqs', 'haps_to_alleles', 'lib', 'pack_seq_groups', 'phasing_priors',
           'poa_consensus', 'pool_reads', 'prune_hap_blocks', 'read_regions', 'remap_aln_probs', 'remap_haplotypes', 'scatter_pool_probs',
           'source_id', 'tbi_parse', 'trim_alignment', 'unused_alleles', 'vcf_fields', 'vcf_header', 'vcf_index', 'vcf_record',
           'vcf_record_from_fields']


def test_facade_keeps_the_surface():
    missing = [n for n in SURFACE if n != "_bind_genotype" and not hasattr(_lib, n)]
    assert missing == []
    assert not hasattr(_lib, "_bind_genotype")
    for n in SURFACE:
        if n != "_bind_genotype":
            assert not isinstance(getattr(_lib, n), types.ModuleType), n


def test_facade_defines_nothing_itself():
    src = open(os.path.join(ROOT, "longtr_amd", "_lib.py")).read()
    assert not re.search(r"^\s*(def|class)\s", src, flags=re.M)
