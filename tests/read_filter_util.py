"""A second restatement of the reference's read filter for reads without mates, written from BamProcessor::read_and_filter_reads
(src/bam_processor.cpp:188-487) and the lines it calls; it does not call the library.  Records are the dicts of Bam.fetch(...,
tags=("RG", "XA")).  The one place where it follows include/ltr_filter.h rather than the reference is named there too: the
max_total_reads stop counts the reads held (the reference counts paired reads, which reads without mates never are), and a record
flagged paired is dropped."""
import functools

DEFAULTS = dict(min_mapq=20, min_mean_qual=30.0, require_spanning=1, min_flank=5, max_total_reads=1000000, base_qual_trim="5")
COUNTERS = ("overlapped", "hard_clipped", "has_n", "low_mapq", "low_qual", "not_spanning", "not_unique", "passed", "paired_unsupported")


class FilterDie(Exception):
    """Where the reference calls printErrorAndDie."""


def trim_alignment_name(name):                                   # :163-170
    return name[:-2] if len(name) > 2 and name[-2] == "/" else name


@functools.lru_cache(maxsize=None)                               # (the tests filter the same records under several option sets)
def mean_quality(qual):                                          # base_quality.h:77-84
    return sum(float(ord(c) - ord("!")) for c in qual) / len(qual)


def spans(rec, start, stop):                                     # :175-186 for one region
    if rec["pos"] > stop or rec["end_pos"] < start:
        return False
    return not (rec["pos"] > start) and not (rec["end_pos"] < stop)


def read_group_sample(rec, read_groups, file_samples):           # :153-161, :458
    if file_samples is not None:
        return file_samples[rec["file"]]
    if "RG" not in rec:
        raise FilterDie("Failed to retrieve BAM alignment's RG tag")
    for g in read_groups:
        if g["file"] == rec["file"] and g["id"] == str(rec["RG"]):
            return g["sample"]
    raise FilterDie("No sample found for read group " + str(rec["RG"]) + " in BAM file headers")


def filter_reads(records, start, stop, read_groups=None, file_samples=None, **options):
    o = dict(DEFAULTS, **options)
    n = dict.fromkeys(COUNTERS, 0)
    verdicts = ["NOT_SCANNED"] * len(records)
    potential_strs, potential_mates = {}, set()                  # key -> (record index, PF)
    too_many, prev_file, file_index, label = False, None, 0, "0_"
    for i, r in enumerate(records):
        if r["pos"] > stop or r["end_pos"] < start:              # :208-215
            verdicts[i] = "OUTSIDE"
            continue
        if r["flag"] & 0x1:
            verdicts[i] = "PAIRED_UNSUPPORTED"
            n["paired_unsupported"] += 1
            continue
        if len(potential_strs) > o["max_total_reads"]:           # :217-220
            too_many = True
            break
        if (r["flag"] & 0x4) or r["pos"] == 0 or not r["cigar"] or not r["seq"]:   # :222
            verdicts[i] = "SKIPPED"
            continue
        overlaps = r["pos"] < stop and r["end_pos"] >= start
        if overlaps and o["base_qual_trim"] > " " and (r["cigar"][0][0] == "H" or r["cigar"][-1][0] == "H"):    # :227-235
            n["overlapped"] += 1
            n["hard_clipped"] += 1
            verdicts[i] = "HARD_CLIPPED"
            continue
        if prev_file != r["file"]:                               # :247-254
            prev_file = r["file"]
            potential_mates.clear()
            file_index += 1
            label = f"{file_index}_"
        key = (label + trim_alignment_name(r["name"])).encode("latin-1")     # bytes compare like std::string
        if not overlaps:                                         # :385-417
            verdicts[i] = "OUTSIDE"
            if key not in potential_strs:
                potential_mates.add(key)
            continue
        n["overlapped"] += 1
        if "N" in r["seq"]:                                      # :265-284
            v = "HAS_N_BASES"; n["has_n"] += 1
        elif mean_quality(r["qual"]) < o["min_mean_qual"]:
            v = "LOW_BASE_QUALS"; n["low_qual"] += 1
        elif r["mapq"] < o["min_mapq"]:
            v = "LOW_MAPQ"; n["low_mapq"] += 1
        elif o["require_spanning"] == 1 and not spans(r, start, stop):
            v = "NOT_SPANNING"; n["not_spanning"] += 1
        else:
            v = "PASS"
        if v != "PASS":                                          # :379-383
            verdicts[i] = v
            potential_mates.add(key)
            continue
        pf = not (o["min_flank"] > 0 and (r["pos"] > start - o["min_flank"] or r["end_pos"] < stop + o["min_flank"]))    # :290
        potential_mates.discard(key)                             # :324-329
        if key in potential_strs:                                # std::map::insert keeps the first (:328, :376)
            verdicts[i] = "DUPLICATE_NAME"
        else:
            potential_strs[key] = (i, pf)
            verdicts[i] = "PASS"
    unpaired = []                                                # :420-437
    for key in sorted(potential_strs):
        i, pf = potential_strs[key]
        if "XA" in records[i]:
            n["not_unique"] += 1
            verdicts[i] = "NO_UNIQUE_MAPPING"
        else:
            unpaired.append((i, pf))
    n["passed"] = len(unpaired)
    samples, by_sample = [], []                                  # :452-483
    while unpaired:
        i, pf = unpaired.pop()
        s = read_group_sample(records[i], read_groups, file_samples)
        if s not in samples:
            samples.append(s)
            by_sample.append([])
        by_sample[samples.index(s)].append((i, pf))
    passing = [(i, k, pf) for k, group in enumerate(by_sample) for i, pf in group]
    return dict(verdicts=verdicts, passing=passing, samples=samples, counters=n, too_many_reads=too_many)


# ---- the hand-made edge cases (tests/test_read_filter.py (b), tests/test_read_filter_standalone.py) -----------------------------
START, STOP = 1000, 1020                                         # the region of every hand-made case
RGS = [dict(id="rg0", sample="S0", library="", file=0)]


def rec(name, pos, end_pos, file=0, mapq=60, flag=0, seq=None, qual=None, cigar=None, rg="rg0", xa=False):
    n = max(end_pos - pos, 1)
    seq = "A" * n if seq is None else seq
    d = dict(name=name, file=file, pos=pos, end_pos=end_pos, mapq=mapq, flag=flag, seq=seq, qual="I" * len(seq) if qual is None else qual,
             cigar=[("=", n)] if cigar is None else cigar)
    if rg is not None:
        d["RG"] = rg
    if xa:
        d["XA"] = "chr2,+5,10M,0;"
    return d


def hand_made_cases():
    """[(name, records, options, sample tables, what must come out)]: expected = dict(verdicts=..., passing=[(record, PF)...] or None,
    too_many_reads=..., error=text or None)."""
    good = lambda name, **kw: rec(name, 900, 1100, **kw)
    rg = dict(read_groups=RGS)
    cases = [
        ("pos_eq_stop_is_outside", [rec("a", STOP, STOP + 50)], {}, rg, dict(verdicts=["OUTSIDE"], passing=[])),
        ("end_eq_start_is_inside", [rec("a", 900, START)], {}, rg, dict(verdicts=["NOT_SPANNING"], passing=[])),
        ("pos_zero", [rec("a", 0, 1100)], {}, rg, dict(verdicts=["SKIPPED"], passing=[])),
        ("hard_clip_left", [good("a", cigar=[("H", 5), ("=", 200)])], {}, rg, dict(verdicts=["HARD_CLIPPED"], passing=[])),
        ("hard_clip_right", [good("a", cigar=[("=", 200), ("H", 5)])], {}, rg, dict(verdicts=["HARD_CLIPPED"], passing=[])),
        ("hard_clip_without_trim", [good("a", cigar=[("H", 5), ("=", 200)])], dict(base_qual_trim=" "), rg, dict(verdicts=["PASS"], passing=[(0, True)])),
        ("n_base", [good("a", seq="A" * 100 + "N" + "A" * 99)], {}, rg, dict(verdicts=["HAS_N_BASES"], passing=[])),
        ("mean_qual_30_and_mapq_20_pass", [good("a", qual="?" * 200, mapq=20)], {}, rg, dict(verdicts=["PASS"], passing=[(0, True)])),
        ("mean_qual_below_30", [good("a", qual="?" * 199 + ">")], {}, rg, dict(verdicts=["LOW_BASE_QUALS"], passing=[])),
        ("mapq_19", [good("a", mapq=19)], {}, rg, dict(verdicts=["LOW_MAPQ"], passing=[])),
        ("n_before_quality_before_mapq", [good("a", seq="N" * 200, qual="!" * 200, mapq=0)], {}, rg, dict(verdicts=["HAS_N_BASES"], passing=[])),
        ("pos_eq_start_end_eq_stop_spans", [rec("a", START, STOP)], {}, rg, dict(verdicts=["PASS"], passing=[(0, False)])),
        ("one_base_short_of_spanning", [rec("a", START + 1, 1100), rec("b", 900, STOP - 1)], {}, rg, dict(verdicts=["NOT_SPANNING"] * 2, passing=[])),
        ("not_spanning_allowed", [rec("a", START + 1, 1100)], dict(require_spanning=0), rg, dict(verdicts=["PASS"], passing=[(0, False)])),
        ("min_flank_boundaries", [rec("a", START - 5, STOP + 5), rec("b", START - 4, STOP + 5), rec("c", START - 5, STOP + 4)], {}, rg,
         dict(verdicts=["PASS"] * 3, passing=[(2, False), (1, False), (0, True)])),
        ("min_flank_zero", [rec("a", START, STOP)], dict(min_flank=0), rg, dict(verdicts=["PASS"], passing=[(0, True)])),
        ("xa_tag", [good("a", xa=True), good("b")], {}, rg, dict(verdicts=["NO_UNIQUE_MAPPING", "PASS"], passing=[(1, True)])),
        ("flag_paired", [good("a", flag=0x1), good("b")], {}, rg, dict(verdicts=["PAIRED_UNSUPPORTED", "PASS"], passing=[(1, True)])),
        ("unmapped_flag", [good("a", flag=0x4)], {}, rg, dict(verdicts=["SKIPPED"], passing=[])),
        ("two_passing_one_name", [good("a", mapq=50), good("a", mapq=40)], {}, rg, dict(verdicts=["PASS", "DUPLICATE_NAME"], passing=[(0, True)])),
        ("name_suffix_is_cut", [good("a/1"), good("a/2")], {}, rg, dict(verdicts=["PASS", "DUPLICATE_NAME"], passing=[(0, True)])),
        ("failing_then_passing_one_name", [good("a", mapq=3), good("a")], {}, rg, dict(verdicts=["LOW_MAPQ", "PASS"], passing=[(1, True)])),
        ("eleven_files_key_order", [good("r", file=k, rg=None) for k in range(11)], {}, dict(file_samples=[f"F{k}" for k in range(11)]),
         dict(verdicts=["PASS"] * 11, passing=[(k, True) for k in (8, 7, 6, 5, 4, 3, 2, 1, 0, 10, 9)])),
        ("skipped_record_keeps_the_file_label", [rec("x", 0, 1100, file=0, rg=None), good("r", file=1, rg=None), good("r", file=2, rg=None)], {},
         dict(file_samples=["F0", "F1", "F2"]), dict(verdicts=["SKIPPED", "PASS", "PASS"], passing=[(2, True), (1, True)])),
        ("samples_in_order_of_the_walk", [good("a", file=0, rg=None), good("b", file=0, rg=None), good("c", file=1, rg=None)], {},
         dict(file_samples=["F0", "F1"]), dict(verdicts=["PASS"] * 3, passing=[(2, True), (1, True), (0, True)])),
        ("two_files_one_sample", [good("a", file=0, rg=None), good("b", file=1, rg=None), good("c", file=2, rg=None)], {},
         dict(file_samples=["X", "Y", "X"]), dict(verdicts=["PASS"] * 3, passing=[(2, True), (0, True), (1, True)])),
        ("max_total_reads_2_of_4", [good("a"), good("b"), good("c"), good("d")], dict(max_total_reads=2), rg,
         dict(verdicts=["PASS", "PASS", "PASS", "NOT_SCANNED"], passing=[(2, True), (1, True), (0, True)], too_many_reads=True)),
        ("no_rg_under_rg_mapping", [good("a", rg=None)], {}, rg, dict(error="Failed to retrieve BAM alignment's RG tag")),
        ("unknown_rg", [good("a", rg="other")], {}, rg, dict(error="No sample found for read group other in BAM file headers")),
        ("failing_read_without_rg_is_no_error", [good("a", rg=None, mapq=0)], {}, rg, dict(verdicts=["LOW_MAPQ"], passing=[])),
    ]
    return cases
