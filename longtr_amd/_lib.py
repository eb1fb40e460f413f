"""Loader + thin Python binding of libltr_gpu.so (the C-ABI of include/ltr_gpu.h).

The product path is the HIP library.  There is no Python/numpy/torch compute
fallback here: a missing library raises at import-of-use time, a missing GPU
makes every compute call raise LtrError(LTR_ERR_NO_DEVICE).

This module is the facade: every name is defined in one of the modules below, by subject.
  _build       the sources and flags of the .so, build(), source_id()
  _abi         the struct layouts and SIGNATURES, the C signature of every function (EXPORTS = its names)
  _loader      lib() (loads at first use, applies SIGNATURES once), LtrError
  _context     Context
  _genotype    Plan, GenotypeResult, the VCF record of a locus
  _filter      the reference's read filter for one region (libltr_filter.so, include/ltr_filter.h)
  _snp         phasing priors of reads from a phased SNP VCF (libltr_snp.so, include/ltr_snp.h)
  _formats     region files, FASTA, VCF writer / panel / index, BAM
  _host        host-only helpers: trimming, pooling, pruning, remapping, phasing priors
  _haplotypes  ReadSet, edit distances, clustering, consensus
  _debug       the debug_* test hooks
"""
from ._abi import BamRecord, SIGNATURES
from ._build import CSRC, HERE, HIPCC_FLAGS, KERNEL_TUS, LIB_PATH, LINK_LIBS, OBJ_DIR, PLAN_UNITS, SOURCES, build, source_id
from ._context import Context
from ._debug import (LAUNCH_KINDS, LAUNCH_NOTE_KINDS, debug_chunk_plan, debug_describe_batch, debug_last_launches, debug_plan_families,
                     debug_plan_family_forks, debug_plan_schedule, debug_threshold_groups)
from ._filter import filter_options, filter_reads
from ._formats import Bam, Fasta, VcfPanel, VcfWriter, read_regions, tbi_parse, vcf_header, vcf_index
from ._genotype import FAMILIES, GenotypeResult, Plan, _locus_haploid, get_alleles, vcf_fields, vcf_record, vcf_record_from_fields
from ._haplotypes import ReadSet, _hap_result, cluster_sequences, edit_distances, pack_seq_groups, poa_consensus
from ._host import (extract_genotypes, haplotype_seqs, haps_to_alleles, phasing_priors, pool_reads, prune_hap_blocks, remap_aln_probs,
                    remap_haplotypes, scatter_pool_probs, trim_alignment, unused_alleles)
from ._loader import LtrError, _lib, _p, lib      # (_lib: the loader's cache as it was at import; _loader._lib is the live one)
from ._snp import PhasedSnps, SnpSet

EXPORTS = list(SIGNATURES)                        # every symbol include/ltr_gpu.h declares
