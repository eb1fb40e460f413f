"""longtr_amd/filter/ltr_filter.cpp under AddressSanitizer + UBSan: a stand-alone program (tests/host_sanitize/filter_main.cpp) runs the
hand-made cases of tests/read_filter_util.py.  CPU only, nothing preloaded; what the program prints must be what the restatement gives."""
import os
import shutil
import subprocess

import pytest

import read_filter_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_lines(name, recs, options, tables):
    o = dict(U.DEFAULTS, **options)
    yield "\t".join(["CASE", name, str(o["min_mapq"]), repr(float(o["min_mean_qual"])), str(o["require_spanning"]), str(o["min_flank"]),
                     str(o["max_total_reads"]), str(ord(o["base_qual_trim"])), str(int("read_groups" in tables)), str(U.START), str(U.STOP)])
    for g in tables.get("read_groups", []):
        yield "\t".join(["RG", g["id"], g["sample"], str(g["file"])])
    for s in tables.get("file_samples", []):
        yield "\t".join(["FS", s])
    for r in recs:
        yield "\t".join(["REC", r["name"], str(r["file"]), str(r["pos"]), str(r["end_pos"]), str(r["mapq"]), str(r["flag"]), r["seq"] or "*",
                         r["qual"] or "*", "".join(t for t, _ in r["cigar"]) or "*", r.get("RG", "*"), str(int("XA" in r))])
    yield "END"


def expected_line(name, recs, options, tables):
    try:
        ref = U.filter_reads(recs, U.START, U.STOP, **tables, **options)
    except U.FilterDie as e:
        return "\t".join([name, "-1", "", "", "", "", "", str(e)])
    return "\t".join([name, "0", ",".join(ref["verdicts"]), ",".join(f"{i}:{s}:{int(pf)}" for i, s, pf in ref["passing"]), ",".join(ref["samples"]),
                      ",".join(str(ref["counters"][k]) for k in U.COUNTERS), str(int(ref["too_many_reads"])), ""])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_filter_under_address_and_undefined_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "filter_main"), U.hand_made_cases()
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host_sanitize", "filter_main.cpp"), os.path.join(ROOT, "longtr_amd", "filter", "ltr_filter.cpp"),
                    "-o", exe], check=True)
    path = tmp_path / "cases.tsv"
    path.write_text("".join(line + "\n" for c in cases for line in case_lines(*c[:4])))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == f"filter cases run: {len(cases)}"
    assert lines[:len(cases)] == [expected_line(*c[:4]) for c in cases]
