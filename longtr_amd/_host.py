"""Host-only helpers of the C-ABI (no GPU needed): trimming, pooling, genotype extraction, allele pruning and remapping, phasing priors."""
import ctypes as C

import numpy as np

from . import _abi
from ._haplotypes import _hap_result
from ._loader import LtrError, _p, lib


def trim_alignment(aln_dict, repeat_start, repeat_end, indel_flank_len):
    pa = _abi.PackedAlignments([aln_dict])
    lt, rt = C.c_int32(0), C.c_int32(0)
    rc = lib().ltr_trim_alignment(pa.array, repeat_start, repeat_end, indel_flank_len, C.byref(lt), C.byref(rt))
    return rc, lt.value, rt.value


def haplotype_seqs(blocks):
    ph = _abi.PackedHaplotype(blocks)
    n = lib().ltr_haplotype_num_combs(C.byref(ph.struct))
    cap = int(sum(max(len(a) for a in b["alleles"]) for b in blocks)) + 1
    out = []
    buf = np.zeros(cap, dtype=np.uint8)
    for k in range(n):
        ln = lib().ltr_haplotype_seq(C.byref(ph.struct), k, _p(buf), cap)
        if ln < 0:
            raise LtrError(ln, "ltr_haplotype_seq")
        out.append(buf[:ln].tobytes())
    return out


def pool_reads(reads):
    keep = [np.frombuffer(r, dtype=np.uint8).copy() if len(r) else np.zeros(1, dtype=np.uint8) for r in reads]
    ptrs = (C.c_void_p * max(len(reads), 1))(*[k.ctypes.data for k in keep])
    lens = np.asarray([len(r) for r in reads], dtype=np.int32)
    idx = np.zeros(max(len(reads), 1), dtype=np.int32)
    n = lib().ltr_pool_reads(ptrs, _p(lens), len(reads), _p(idx))
    return n, idx[:len(reads)]


def scatter_pool_probs(pool_probs, pool_seeds, pool_index, n_alleles, realign_to_hap=None, copy_read=None,
                       second_mate=None, log_aln_probs=None, seed_positions=None):
    pool_probs = np.ascontiguousarray(pool_probs, dtype=np.float64)
    pool_seeds = np.ascontiguousarray(pool_seeds, dtype=np.int32)
    pool_index = np.ascontiguousarray(pool_index, dtype=np.int32)
    R = len(pool_index)
    out = np.full(R * n_alleles, np.nan, dtype=np.float64) if log_aln_probs is None else log_aln_probs
    seeds = np.full(R, -1, dtype=np.int32) if seed_positions is None else seed_positions
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    rh, cr, sm = u8(realign_to_hap), u8(copy_read), u8(second_mate)
    rc = lib().ltr_scatter_pool_probs(_p(pool_probs), _p(pool_seeds), _p(pool_index), R, n_alleles, _p(rh), _p(cr),
                                      _p(sm), _p(out), _p(seeds))
    if rc != 0:
        raise LtrError(rc, "ltr_scatter_pool_probs")
    return out.reshape(R, n_alleles), seeds


def extract_genotypes(log_sample_posteriors, sample_total_ll, best_haplotypes, hap_to_allele, n_variants, haploid=False,
                      want=("gls", "gl_diffs", "pls", "phased_gls")):
    """Genotyper::extract_genotypes_and_likelihoods (genotyper.cpp:132-256) through ltr_extract_genotypes.

    log_sample_posteriors [S, H, H], sample_total_ll [S], best_haplotypes [S, 2] (ltr_posteriors' gts),
    hap_to_allele [H].  Returns a dict of numpy arrays (best_gts, log_*_posteriors, gls, gl_diffs, pls, phased_gls)."""
    post = np.ascontiguousarray(log_sample_posteriors, dtype=np.float64)
    S, H = post.shape[0], post.shape[1]
    stl = np.ascontiguousarray(sample_total_ll, dtype=np.float64)
    bh = np.ascontiguousarray(best_haplotypes, dtype=np.int32)
    h2a = np.ascontiguousarray(hap_to_allele, dtype=np.int32)
    if post.shape != (S, H, H) or stl.shape != (S,) or bh.shape != (S, 2) or h2a.shape != (H,):
        raise LtrError(-1, "extract_genotypes: shape mismatch")
    f, arrs = _abi.genotype_field_buffers(S, n_variants, haploid, want)
    rc = lib().ltr_extract_genotypes(S, H, n_variants, _p(h2a), 1 if haploid else 0, _p(post), _p(stl), _p(bh), C.byref(f))
    if rc != 0:
        raise LtrError(rc, "ltr_extract_genotypes")
    return arrs


# ---- the genotyper's last steps (host): allele pruning and remapping ---------------------------
def haps_to_alleles(blocks, block):
    ph = _abi.PackedHaplotype(blocks)
    out = np.zeros(ph.num_combs, dtype=np.int32)
    rc = lib().ltr_haps_to_alleles(C.byref(ph.struct), block, _p(out))
    if rc != 0:
        raise LtrError(rc, "ltr_haps_to_alleles")
    return out


def unused_alleles(best_haplotypes, hap_to_allele, n_block_alleles, sample_has_aligned_read=None, sample_filtered=None):
    bh = np.ascontiguousarray(best_haplotypes, dtype=np.int32)
    h2a = np.ascontiguousarray(hap_to_allele, dtype=np.int32)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    ar, fl = u8(sample_has_aligned_read), u8(sample_filtered)
    out = np.zeros(max(n_block_alleles, 1), dtype=np.int32)
    n = lib().ltr_unused_alleles(len(bh), _p(bh), _p(ar), _p(fl), len(h2a), _p(h2a), n_block_alleles, _p(out))
    if n < 0:
        raise LtrError(n, "ltr_unused_alleles")
    return out[:n].tolist()


def remap_haplotypes(old_blocks, new_blocks):
    po, pn = _abi.PackedHaplotype(old_blocks), _abi.PackedHaplotype(new_blocks)
    mapping = np.zeros(po.num_combs, dtype=np.int32)
    realign = np.zeros(pn.num_combs, dtype=np.uint8)
    rc = lib().ltr_remap_haplotypes(C.byref(po.struct), C.byref(pn.struct), _p(mapping), _p(realign))
    if rc != 0:
        raise LtrError(rc, "ltr_remap_haplotypes")
    return mapping, realign


def remap_aln_probs(old_ll, mapping, h_new):
    old = np.ascontiguousarray(old_ll, dtype=np.float64)
    R, Ho = old.shape
    m = np.ascontiguousarray(mapping, dtype=np.int32)
    new = np.zeros((R, h_new), dtype=np.float64)
    rc = lib().ltr_remap_aln_probs(_p(old), R, Ho, _p(m), h_new, _p(new))
    if rc != 0:
        raise LtrError(rc, "ltr_remap_aln_probs")
    return new


def prune_hap_blocks(blocks, block, unused):
    """ltr_prune_hap_blocks (HapBlock::remove_alleles for one block of a list): the new list of block dicts."""
    ph = _abi.PackedHaplotype(blocks)
    un = np.ascontiguousarray(unused, dtype=np.int32)
    h = C.c_void_p()
    rc = lib().ltr_prune_hap_blocks(C.byref(ph.struct), int(block), _p(un) if len(un) else None, len(un), C.byref(h))
    if rc != 0:
        raise LtrError(rc, "ltr_prune_hap_blocks")
    return _hap_result(h)["blocks"]


def phasing_priors(sample_of_read, haplotype, n_samples):
    """ltr_phasing_priors (SNPBamProcessor::process_phased_reads for unpaired reads): (log_p1, log_p2, phased reads)."""
    so = np.ascontiguousarray(sample_of_read, dtype=np.int32)
    hp = np.ascontiguousarray(haplotype, dtype=np.int32)
    p1, p2 = np.zeros(len(so)), np.zeros(len(so))
    n = C.c_int32(0)
    rc = lib().ltr_phasing_priors(len(so), _p(so), _p(hp), int(n_samples), _p(p1), _p(p2), C.byref(n))
    if rc != 0:
        raise LtrError(rc, "ltr_phasing_priors")
    return p1, p2, n.value
