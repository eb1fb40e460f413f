"""-m gpu: the --ref-vcf chain on REAL reads (examples/real_reads_trio.py with ref_vcf=...): the trio's discovery-mode VCF,
indexed by ltr_vcf_index, read back as the panel of candidate alleles.  Checked: every locus genotyped in discovery mode is
genotyped with the panel; the output records keep the panel's POS / REF / ALT; the called allele lengths are those of
discovery mode; the LL matrix of every panel locus bit for bit against the CPU oracle; and, with five records edited (one
allele a motif unit longer than any other added, the ALT order reversed), the edited alleles are scored in the panel's order
and none is pruned.

The VCF record orders its ALTs as write_vcf_record does in the reference -- reorder_alleles (seq_stutter_genotyper.cpp:1074)
sorts them by length, then sequence, whatever the candidates' order -- so an output record equals the panel record when the
panel's ALTs are in that order (as every panel written by the genotyper is), and holds the same ALTs otherwise."""
import gzip, importlib.util, os

import numpy as np
import pytest

from longtr_amd import _abi, _lib
from test_gpu_host_path import _expected_calc_hap_aln_probs, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("real_reads_trio", os.path.join(ROOT, "examples", "real_reads_trio.py"))
rt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rt)


def _records(path):
    """Data lines of a BGZF VCF keyed by (chrom, INFO START, INFO END), and the header text."""
    text = gzip.decompress(open(path, "rb").read()).decode()
    head = "".join(t + "\n" for t in text.splitlines() if t.startswith("#"))
    recs = {}
    for t in text.splitlines():
        if t.startswith("#"):
            continue
        c = t.split("\t")
        info = dict(kv.split("=", 1) for kv in c[7].split(";") if "=" in kv)
        recs[(c[0], int(info["START"]), int(info["END"]))] = c
    return recs, head


def _key(l):
    r = l["region"]
    return (r["chrom"], r["start"] + 1, r["stop"])


def _rel_gt_lens(l):
    """Called allele lengths relative to the REF allele (a panel block is the VCF allele, a discovery block the trimmed one)."""
    alleles = l["blocks"][1]["alleles"]
    return [tuple(sorted(len(alleles[int(g)]) - len(alleles[0]) for g in gt)) for gt in l["gts"]]


def _check_oracle(loci):
    prm, sp = _abi.default_params(), _abi.default_stutter_params()
    for l in loci:
        want, ws = _expected_calc_hap_aln_probs(prm, sp, l["blocks"], l["alns"], None)
        assert np.array_equal(bits(l["ll"]), bits(want)) and np.array_equal(l["seeds"], ws), l["region"]["name"]


@pytest.fixture(scope="module")
def discovery(gpu_ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("panel")
    vcf = str(d / "discovery.vcf.gz")
    loci = rt.run(gpu_ctx, vcf, tmp_dir=str(d))
    _lib.vcf_index(vcf)
    return d, vcf, loci


@pytest.mark.gpu
def test_trio_panel_round_trip(gpu_ctx, discovery):
    d, vcf, disc = discovery
    panel_recs, _ = _records(vcf)
    out = str(d / "panel_out.vcf.gz")
    loci = rt.run(gpu_ctx, out, tmp_dir=str(d), ref_vcf=vcf)
    by_key = {_key(l): l for l in loci}
    ok_disc = [l for l in disc if l["status"] == "ok"]
    assert len(ok_disc) >= 35
    for l in ok_disc:
        p = by_key[_key(l)]
        assert p["status"] == "ok", (l["region"]["name"], p["status"])
        c = p["vcf_line"].split("\t")
        assert c[1] == panel_recs[_key(l)][1] and c[3] == panel_recs[_key(l)][3] and c[4] == panel_recs[_key(l)][4], l["region"]["name"]
        if l["region"]["period"] >= 2:
            assert _rel_gt_lens(p) == _rel_gt_lens(l), l["region"]["name"]
    for l in disc:                                                  # a locus without a call has no record: it stops where it stopped, or there
        if l["status"] != "ok":
            assert by_key[_key(l)]["status"] in (l["status"], "no panel record"), l["region"]["name"]
    ok = [l for l in loci if l["status"] == "ok"]
    assert len(ok) == len(panel_recs)
    _check_oracle(ok)
    written, _ = _records(out)
    assert sorted(written) == sorted(panel_recs)


@pytest.mark.gpu
def test_trio_edited_panel(gpu_ctx, discovery):
    d, vcf, disc = discovery
    recs, head = _records(vcf)
    ok = {_key(l): l for l in disc if l["status"] == "ok"}
    poly = [k for k in sorted(recs) if k in ok and recs[k][4] != "." and ok[k]["region"]["period"] >= 2][:5]
    assert len(poly) == 5
    edited = {}
    for k in poly:
        c = list(recs[k])
        alts = c[4].split(",")
        motif = ok[k]["region"]["motif"].split(",")[0].upper()
        longest = max([c[3]] + alts, key=len)
        i = max(longest.find(motif), 1)
        longer = longest[:i] + motif + longest[i:]                  # one motif unit longer than any allele of the record
        c[4] = ",".join(list(reversed(alts + [longer])))
        recs[k] = c
        edited[k] = [c[3]] + c[4].split(",")
    path = str(d / "edited.vcf.gz")
    w = _lib.VcfWriter(path)
    w.header(head)
    for k in sorted(recs, key=lambda k: (k[0], int(recs[k][1]))):
        w.add_record(k[0], int(recs[k][1]), "\t".join(recs[k]))
    w.close()
    _lib.vcf_index(path)
    loci = {_key(l): l for l in rt.run(gpu_ctx, str(d / "edited_out.vcf.gz"), tmp_dir=str(d), ref_vcf=path)}
    for k, alleles in edited.items():
        l = loci[k]
        assert l["status"] == "ok", l["status"]
        # scored in the panel's order, nothing pruned ("<DEL>": the block allele with no bases)
        assert l["blocks"][1]["alleles"] == [b"" if a == "<DEL>" else a.upper().encode() for a in alleles]
        alt_out = l["vcf_line"].split("\t")[4].split(",")
        assert sorted(alt_out) == sorted(alleles[1:])                                       # every panel ALT in the record, the added one too
        dels = [a for a in alleles[1:] if a == "<DEL>"]                                     # write_vcf_record's order (get_alleles, reorder_alleles)
        assert alt_out == dels + sorted((a for a in alleles[1:] if a != "<DEL>"), key=lambda a: (len(a), a))
        assert _rel_gt_lens(l) == _rel_gt_lens(ok[k]), l["region"]["name"]
    _check_oracle([loci[k] for k in edited])
