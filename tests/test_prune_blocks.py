"""CPU: ltr_prune_hap_blocks (HapBlock::remove_alleles for a block list) and the haplotype order of the pruned list --
against the C restatement's re-mapping (oracle/ltr_oracle_vcf.c) and a Python restatement of Haplotype::next()
(genotype_util.gray_counts).  Parity with the reference itself is unpinned for these functions, as for the rest of the
genotyper's last steps (seq_stutter_genotyper.cpp needs htslib)."""
import numpy as np
import pytest

import genotype_util as gt
import oracle_lib as ol
from longtr_amd import _abi, _lib, synth


def _random_blocks(rng, n_multi):
    """[flank][repeat][flank] with n_multi of the three blocks multi-allelic (distinct sequences per block)."""
    L = synth.synth_locus(rng, int(rng.integers(9, 50)), 3, int(rng.integers(3, 7)), 2)
    blocks = L.blocks()
    for b in ([], [2], [0, 2])[n_multi - 1]:
        base = blocks[b]["alleles"][0]
        alts = []
        for k in range(int(rng.integers(1, 4))):
            f = bytearray(base)
            f[3 + 2 * k] = ord("A") if f[3 + 2 * k] != ord("A") else ord("C")
            alts.append(bytes(f))
        blocks[b]["alleles"] = [base] + alts
    return blocks


def test_prune_hap_blocks_remap_and_gray_order():
    rng = np.random.default_rng(81)
    reordered = 0
    for trial in range(90):
        blocks = _random_blocks(rng, 1 + trial % 3)
        removed = []
        for b in blocks:                                         # any subset of the alternates, allele 0 never
            n = len(b["alleles"])
            removed.append(sorted(int(a) for a in rng.choice(np.arange(1, n), size=int(rng.integers(0, n)), replace=False)) if n > 1 else [])
        new = blocks
        for b, rm in enumerate(removed):                         # one block per call, like a caller of ltr_unused_alleles
            new = _lib.prune_hap_blocks(new, b, rm)
        want = gt.remove_alleles(blocks, removed)
        assert [b["alleles"] for b in new] == [b["alleles"] for b in want]
        for k in ("start", "end", "is_repeat", "period"):
            assert [b[k] for b in new] == [b[k] for b in blocks]
        m, realign = _lib.remap_haplotypes(blocks, new)
        mo, ro = ol.oracle_remap_haplotypes(blocks, new)
        assert np.array_equal(m, mo) and np.array_equal(realign, ro) and not realign.any()
        old_seqs, new_seqs = _lib.haplotype_seqs(blocks), _lib.haplotype_seqs(new)
        assert old_seqs == gt.gray_seqs(blocks) and new_seqs == gt.gray_seqs(new)      # Haplotype::next() order of each list
        kept = [j for j in range(len(old_seqs)) if m[j] >= 0]
        assert sorted(m[j] for j in kept) == list(range(len(new_seqs)))
        assert all(new_seqs[m[j]] == old_seqs[j] for j in kept)
        if [int(m[j]) for j in kept] != list(range(len(kept))):
            reordered += 1                                       # the new order is NOT the old order with gaps
    assert reordered >= 5, reordered


def test_gray_order_changes_when_an_inner_allele_goes():
    """Hand-checked on two blocks of three options each (block 0 moves fastest and turns round at either end): which old
    haplotype every new one is depends on the walk of the NEW list -- removing an allele of the second block reverses a sweep
    of the first, so the survivors do not keep their old order."""
    A = [b"AAAA", b"CCCC", b"GGGG"]
    B = [b"TT", b"TA", b"AT"]
    blocks = [dict(start=0, end=4, is_repeat=False, period=0, alleles=A), dict(start=4, end=6, is_repeat=True, period=1, alleles=B)]
    assert gt.gray_counts([3, 3]) == [(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (0, 1), (0, 2), (1, 2), (2, 2)]
    new = _lib.prune_hap_blocks(blocks, 0, [2])
    assert gt.gray_counts([2, 3]) == [(0, 0), (1, 0), (1, 1), (0, 1), (0, 2), (1, 2)]
    m, _ = _lib.remap_haplotypes(blocks, new)
    assert list(m) == [0, 1, -1, -1, 2, 3, 4, 5, -1]
    new = _lib.prune_hap_blocks(blocks, 0, [1])
    m, _ = _lib.remap_haplotypes(blocks, new)
    # new walk over A0 / A2: 00 20 21 01 02 22 -> old indices 0, 2, 3, 5, 6, 8: here the old order with gaps
    assert list(m) == [0, -1, 1, 2, -1, 3, 4, -1, 5]
    new = _lib.prune_hap_blocks(blocks, 1, [1])
    m, _ = _lib.remap_haplotypes(blocks, new)
    # new walk over B0 / B2: 00 10 20 22 12 02 -> old 0, 1, 2, 8, 7, 6: the second sweep runs the other way round
    assert list(m) == [0, 1, 2, -1, -1, -1, 5, 4, 3]
    assert _lib.haplotype_seqs(new) == [b"AAAATT", b"CCCCTT", b"GGGGTT", b"GGGGAT", b"CCCCAT", b"AAAAAT"]


def test_prune_hap_blocks_rejects_the_reference_allele_and_bad_indices():
    blocks = _random_blocks(np.random.default_rng(82), 1)
    n = len(blocks[1]["alleles"])
    for block, unused in ((1, [0]), (1, [n]), (1, [-1]), (3, [1]), (-1, [1]), (0, [1])):
        with pytest.raises(_lib.LtrError) as e:
            _lib.prune_hap_blocks(blocks, block, unused)
        assert e.value.code == _abi.LTR_ERR_INVALID
    assert [b["alleles"] for b in _lib.prune_hap_blocks(blocks, 1, [])] == [b["alleles"] for b in blocks]
    assert [b["alleles"] for b in _lib.prune_hap_blocks(blocks, 1, [1, 1])][1] == [a for i, a in enumerate(blocks[1]["alleles"]) if i != 1]
