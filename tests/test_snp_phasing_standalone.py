"""longtr_amd/snp/ltr_snp.cpp under AddressSanitizer + UBSan: a stand-alone program (tests/host_sanitize/snp_main.cpp) runs the hand-made
cases of tests/snp_phasing_util.py.  CPU only, nothing preloaded; what the program prints must be what the restatement gives."""
import os
import shutil
import subprocess

import pytest

import snp_phasing_util as U
from longtr_amd import _snp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def set_lines(name, header, lines, skip, padding=15):
    yield "\t".join(["SET", name, str(padding), ",".join(f"{a}:{b}" for a, b in skip) or "-", str(len(lines))])
    yield header
    yield from lines


def reads_lines(column, reads):
    yield "\t".join(["READS", str(column), str(len(reads))])
    for r in reads:
        yield "\t".join([str(r["pos"]), str(r["end_pos"]), r["bases"].hex() or "*", r["quals"].hex() or "*", "".join(f"{n}{op}" for op, n in r["cigar"]) or "*"])


def expected_set(name, header, lines, skip):
    try:
        ref = U.build_set(header, lines, skip)
    except U.SnpDie as e:
        return ["SET", name, str(e.code)]
    return ["SET", name, "0", str(len(ref["samples"])), str(ref["n_valid"]), ";".join(",".join(f"{p}:{a}:{b}" for p, a, b in v) for v in ref["snps"]),
            ",".join(str(ref["index"][s]) for s in ref["samples"])]


def expected_reads(ref, column, reads, tables):
    try:
        p1, p2, n = U.priors(ref, column, reads, tables)
    except U.SnpDie as e:
        return ["READS", str(e.code)]
    return ["READS", "0", ",".join(f"{int(b):016x}" for b in U.bits(p1)), ",".join(f"{int(b):016x}" for b in U.bits(p2)), ",".join(str(k) for k in n)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_snp_priors_under_address_and_undefined_sanitizers(tmp_path):
    exe, tables = str(tmp_path / "snp_main"), _snp.quality_tables()
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host_sanitize", "snp_main.cpp"), os.path.join(ROOT, "longtr_amd", "snp", "ltr_snp.cpp"),
                    "-o", exe], check=True)
    text, want = [], []
    for name, header, lines, skip, _ in U.record_cases():
        text += set_lines(name, header, lines, skip)
        want.append(expected_set(name, header, lines, skip))
    for name, snps, reads, _ in U.read_cases():
        header, lines = U.HEADER + "\tS", U.snp_lines(snps)
        text += set_lines(name, header, lines, [])
        want.append(expected_set(name, header, lines, []))
        for column in (0, -1):
            text += reads_lines(column, reads)
            want.append(expected_reads(U.build_set(header, lines), column, reads, tables))
    path = tmp_path / "cases.txt"
    path.write_text("".join(t + "\n" for t in text))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    got = r.stdout.split("\n")
    n_sets = sum(1 for w in want if w[0] == "SET")
    assert got[len(want)] == f"snp sets run: {n_sets}, read blocks run: {len(want) - n_sets}"
    for g, w in zip(got, want):
        f = g.split("\t")
        if w[2 if w[0] == "SET" else 1] != "0":                  # an error: the status, and some text after it
            assert f[:len(w)] == w and len(f) == len(w) + 1 and f[-1], g
        else:
            assert f == w, g
    assert sum(1 for w in want if w[0] == "READS" and w[1] == "-5") == 2 and sum(1 for w in want if w[0] == "READS" and w[1] == "-1") == 2
