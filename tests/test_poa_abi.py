"""The C-ABI of the consensus entry points (include/ltr_gpu.h: ltr_poa_consensus, ltr_poa_consensus_capacity,
ltr_build_haplotypes_consensus and the two accessors) as far as it can be seen without a device: the symbols and their documented
signatures, and the statuses of calls that never reach one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from longtr_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ltr_gpu.h")).read(), flags=re.S)
HEADER = re.sub(r"\s+", " ", HEADER)


def test_symbols_and_documented_signatures():
    L = _lib.lib()
    for sym in ("ltr_poa_consensus", "ltr_poa_consensus_capacity", "ltr_build_haplotypes_consensus", "ltr_hap_result_consensus_rounds",
                "ltr_hap_result_medoid_kept"):
        assert hasattr(L, sym) and sym in _lib.EXPORTS, sym
    for decl in ("int ltr_poa_consensus(ltr_ctx* ctx, const ltr_seq_groups* sg, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off , uint8_t* status );",
                 "int64_t ltr_poa_consensus_capacity(const ltr_seq_groups* sg);",
                 "int ltr_build_haplotypes_consensus(ltr_ctx* ctx, const ltr_hap_build_locus* loci, int64_t n_loci, int32_t indel_flank_len, ltr_hap_result** out );",
                 "int32_t ltr_hap_result_consensus_rounds(const ltr_hap_result* r, int32_t sample);",
                 "int32_t ltr_hap_result_medoid_kept(const ltr_hap_result* r, int32_t sample);"):
        assert decl in HEADER, decl
    assert "#define LTR_ABI_VERSION 6" in HEADER                   # no existing struct changed
    assert L.ltr_abi_version() == 6


def _outputs(n_groups, cap):
    return dict(bytes=np.full(max(cap, 1), 0x5A, dtype=np.uint8), off=np.full(n_groups + 1, -7, dtype=np.int64),
                status=np.full(max(n_groups, 1), 9, dtype=np.uint8), cap=cap)


def _untouched(out):
    return bool((out["bytes"] == 0x5A).all() and (out["off"] == -7).all() and (out["status"] == 9).all())


def test_without_a_context_is_an_error_not_a_fallback():
    groups = [[b"ACGT", b"ACGT", b"AGGT"], [b"AC"]]
    out = _outputs(2, 64)
    with pytest.raises(_lib.LtrError) as e:
        _lib.poa_consensus(None, groups, out=out)
    assert e.value.code == _abi.LTR_ERR_NO_DEVICE and _untouched(out)
    out = _outputs(2, 3)                                            # a too small out_cap: still "no device", nothing written
    with pytest.raises(_lib.LtrError) as e:
        _lib.poa_consensus(None, groups, out=out)
    assert e.value.code == _abi.LTR_ERR_NO_DEVICE and _untouched(out)


def test_capacity_and_malformed_groups():
    L = _lib.lib()
    groups = [[b"ACGT", b"", b"AGGTT"], [], [b"AC"]]
    pk = _lib.pack_seq_groups(groups)
    assert L.ltr_poa_consensus_capacity(C.byref(pk["sg"])) == 11    # the bytes of all groups
    assert L.ltr_poa_consensus_capacity(None) == _abi.LTR_ERR_INVALID
    raw, seq_off, gso = pk["keep"]
    for spoil in ("group range", "sequence offsets", "negative count"):
        bad = _lib.pack_seq_groups(groups)
        _, so, go = bad["keep"]
        if spoil == "group range":
            go[2] = 9                                               # past the last sequence
        elif spoil == "sequence offsets":
            so[2] = 1                                               # descending
        else:
            bad["sg"].n_groups = -1
        assert L.ltr_poa_consensus_capacity(C.byref(bad["sg"])) == _abi.LTR_ERR_INVALID, spoil
        out = _outputs(3, 64)
        with pytest.raises(_lib.LtrError) as e:                     # without a context the status is "no device" whatever the groups are
            _lib.poa_consensus(None, None, packed=bad, out=out)
        assert e.value.code == _abi.LTR_ERR_NO_DEVICE and _untouched(out), spoil


def test_build_haplotypes_consensus_without_a_context():
    L = _lib.lib()
    arr = (_abi.HapBuildLocus * 2)()
    out = (C.c_void_p * 2)(1, 1)
    assert L.ltr_build_haplotypes_consensus(None, arr, 2, 5, out) == _abi.LTR_ERR_NO_DEVICE
    assert out[0] is None and out[1] is None                        # every out[l] NULL on an error status
    assert L.ltr_build_haplotypes_consensus(None, arr, -1, 5, out) == _abi.LTR_ERR_INVALID
    assert L.ltr_build_haplotypes_consensus(None, arr, 2, -1, out) == _abi.LTR_ERR_INVALID
    assert L.ltr_build_haplotypes_consensus(None, arr, 2, 5, None) == _abi.LTR_ERR_INVALID
    assert L.ltr_hap_result_consensus_rounds(None, 0) == 0 and L.ltr_hap_result_medoid_kept(None, 0) == 0
