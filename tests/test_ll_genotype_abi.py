"""CPU: ltr_ll_genotype is exported, struct ltr_ll_batch in longtr_amd/_abi.py has the layout the C compiler gives the header's
struct (a tiny probe compiled against include/ltr_gpu.h prints sizeof / offsetof), and NULL arguments are refused before
anything touches a device."""
import ctypes as C
import os
import shutil
import subprocess

from longtr_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ltr_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(ltr_ll_batch), offsetof(ltr_ll_batch, log_aln_probs), offsetof(ltr_ll_batch, seed_positions),
         offsetof(ltr_ll_batch, n_haps));
  return 0;
}
"""


def test_symbol_is_exported_and_declared():
    L = _lib.lib()
    assert hasattr(L, "ltr_ll_genotype") and "ltr_ll_genotype" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ltr_gpu.h")).read()
    assert "int ltr_ll_genotype(ltr_ctx* ctx, const ltr_ll_batch* lb, const ltr_genotype_batch* gb," in hdr


def test_struct_layout_matches_the_header(tmp_path):
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/llvm/bin/clang")
               if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c))), None)
    assert cc, "no C compiler"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o_ll, o_seed, o_h = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    B = _abi.LlBatch
    assert (C.sizeof(B), B.log_aln_probs.offset, B.seed_positions.offset, B.n_haps.offset) == (size, o_ll, o_seed, o_h)
    assert [f[0] for f in B._fields_] == ["log_aln_probs", "seed_positions", "n_haps"]


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    lb, gb, pb = _abi.LlBatch(), _abi.GenotypeBatch(), _abi.PosteriorBatch()
    gb.pb = C.pointer(pb)
    fake = C.c_void_p(0x1000)                                    # never dereferenced: the NULL argument is found first
    for ctx, plb, pgb, with_out in ((None, lb, gb, True), (fake, None, gb, True), (fake, lb, None, True), (fake, lb, gb, False)):
        h = C.c_void_p(0x1234)
        rc = L.ltr_ll_genotype(ctx, None if plb is None else C.byref(plb), None if pgb is None else C.byref(pgb), None,
                               C.byref(h) if with_out else None)
        assert rc == _abi.LTR_ERR_INVALID
        assert not with_out or not h.value                       # *out is cleared whenever it can be
    nopb = _abi.GenotypeBatch()                                  # gb->pb NULL
    h = C.c_void_p(0x1234)
    assert L.ltr_ll_genotype(fake, C.byref(lb), C.byref(nopb), None, C.byref(h)) == _abi.LTR_ERR_INVALID and not h.value
