"""Shared builders for the short (stutter) path tests."""
import numpy as np

from longtr_amd import synth

KA_LF = b"ACGTTGCAAGCTTAGGCTAACGTTAGCCATGGATC"
KA_RF = b"GGATCCTTAGCAATCGGATTACAGGCTTAACCGTA"


def known_answer_case():
    """The probe behind SURVEY.md 8c's short-path values (-7.8693081508, -4.3896419406): a 14-bp
    poly-A locus with two alleles and one read carrying the +1 allele, all qualities 'I'."""
    pl, pr, rep = b"TTGAC", b"CAGTT", b"A" * 14
    s0 = 1000
    blocks = [dict(start=s0, end=s0 + 35, is_repeat=False, period=0, alleles=[KA_LF]),
              dict(start=s0 + 35, end=s0 + 59, is_repeat=True, period=1, alleles=[pl + rep + pr, pl + rep + b"A" + pr]),
              dict(start=s0 + 59, end=s0 + 94, is_repeat=False, period=0, alleles=[KA_RF])]
    rs = KA_LF + pl + rep + b"A" + pr + KA_RF
    aln = dict(start=s0, stop=s0 + 93, seq=rs, cigar=[("=", 54), ("I", 1), ("=", 40)], qual=b"I" * len(rs))
    return blocks, [aln]


homopolymer_locus = synth.homopolymer_locus       # (the bench's neighbour measurement draws the same loci)


# ---- inputs for the pins of compute_aln_logprob / calc_seed_base / calc_best_seed_position (HapAligner.cpp:165-233, :467-542)
def lcg_matrix(seed, n):
    """n doubles in (-977.2, -0.5], every 17th residue class IMPOSSIBLE-like (-1e9): exact integer arithmetic + one
    correctly rounded division, so that a golden file can name a matrix by its seed."""
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) % np.uint64(1000003)
    v = -0.5 - k.astype(np.float64) / 1024.0
    v[k % np.uint64(17) == 0] = -1.0e9
    return v


def _rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(int(x) for x in rng.choice(list(alphabet), size=n))


def random_blocks(rng, n_repeats=None, start=None):
    """flank | repeat | flank [| repeat | flank ...]: contiguous coordinates, 1-3 alleles per repeat block."""
    nrep = int(rng.integers(1, 4)) if n_repeats is None else n_repeats
    pos = int(rng.integers(100, 5000)) if start is None else start
    blocks = []
    for b in range(2 * nrep + 1):
        if b % 2 == 0:
            seq = _rand_seq(rng, int(rng.integers(3, 40)))
            blocks.append(dict(start=pos, end=pos + len(seq), is_repeat=False, period=0, alleles=[seq]))
        else:
            period = int(rng.integers(1, 4))
            motif = _rand_seq(rng, period)
            units = int(rng.integers(1, 15))
            ref = motif * units
            alts = [motif * max(units + int(d), 0) for d in rng.choice([-2, -1, 1, 2, 3], size=int(rng.integers(0, 3)), replace=False)]
            alts = [a for a in alts if len(a) > 0]
            seq = ref
            blocks.append(dict(start=pos, end=pos + len(seq), is_repeat=True, period=period, alleles=[ref] + alts))
        pos += len(seq)
    return blocks


def seed_case(rng):
    """(blocks, alignment) for calc_seed_base: a random =/X/I/D CIGAR that starts before, at or inside the first block and
    may run past the last one."""
    blocks = random_blocks(rng)
    first, last = blocks[0]["start"], blocks[-1]["end"]
    start = first + int(rng.integers(-30, 12))
    cigar, pos, nbases = [], start, 0
    stop_at = last + int(rng.integers(-10, 30))
    while pos < stop_at:
        t = "=XID"[int(rng.choice(4, p=[0.55, 0.15, 0.15, 0.15]))]
        k = int(rng.integers(1, 30)) if t == "=" else int(rng.integers(1, 4))
        if cigar and cigar[-1][0] == t:
            continue
        cigar.append((t, k))
        if t in "=XD":
            pos += k
        if t in "=XI":
            nbases += k
    seq = _rand_seq(rng, max(nbases, 1))
    return blocks, dict(start=start, stop=pos - 1, seq=seq, cigar=cigar, qual=b"I" * len(seq))


def logprob_case(rng, mseed):
    """Arguments of compute_aln_logprob for a random haplotype (random allele per block) and seed position."""
    blocks = random_blocks(rng)
    counts = [int(rng.integers(0, len(b["alleles"]))) for b in blocks]
    hapsize = sum(len(b["alleles"][c]) for b, c in zip(blocks, counts))
    base_seq_len = int(rng.integers(3, 40))
    seed_base = int(rng.integers(1, base_seq_len - 1))
    lflank, rflank = seed_base, base_seq_len - seed_base - 1
    q = int(rng.integers(2, 42))
    err = 10.0 ** (-q / 10.0)
    return dict(blocks=blocks, counts=counts, base_seq_len=base_seq_len, seed_base=seed_base, seed_char=int(rng.choice(list(b"ACGT"))),
                log_seed_wrong=float(np.log(err / 3.0)), log_seed_correct=float(np.log1p(-err)), mseed=int(mseed),
                l_prob=-float(rng.random() * 30) - 0.5, r_prob=-float(rng.random() * 30) - 0.5, n_l=lflank * hapsize, n_r=rflank * hapsize)


def logprob_matrices(c):
    return lcg_matrix(c["mseed"], c["n_l"]), lcg_matrix(c["mseed"] + 7919, c["n_r"])


# ---- crafted loci and reads: the geometry rules of the seeded path (ltr_short.hip, short_geometry) -------------------
# homopolymer_locus fixes the shape of every read (35-base flanks, seed in their middle, sides of 180 .. 260 bases); these
# builders put the seed, the side lengths, the flank lengths and the repeat block where a test wants them.
MIN_SEED_DIST = 5                                 # HapAligner.cpp:17: a seed needs >= 9 matched flank bases around it


def crafted_locus(lf_len, repeat_alleles, rf_len, rng=None, start=1000):
    """[flank][repeat, period 1][flank] with the given repeat alleles (bytes; the first is the reference allele and may not be
    empty).  Flank bases are drawn from CGT: a flank never extends an A homopolymer."""
    rng = np.random.default_rng(lf_len * 1009 + rf_len) if rng is None else rng
    lf, rf = _rand_seq(rng, lf_len, b"CGT"), _rand_seq(rng, rf_len, b"CGT")
    ref = len(repeat_alleles[0])
    assert lf_len > 0 and rf_len > 0 and ref > 0 and len(set(repeat_alleles)) == len(repeat_alleles)
    return [dict(start=start, end=start + lf_len, is_repeat=False, period=0, alleles=[lf]),
            dict(start=start + lf_len, end=start + lf_len + ref, is_repeat=True, period=1, alleles=[bytes(a) for a in repeat_alleles]),
            dict(start=start + lf_len + ref, end=start + lf_len + ref + rf_len, is_repeat=False, period=0, alleles=[rf])]


def crafted_read(blocks, allele, left_pad, right_pad, seed_flank, rng, plant_quals=None, plant_bases=None):
    """left_pad random bases, the haplotype of repeat allele `allele` (an index), right_pad random bases; a negative pad cuts
    that many bases off the haplotype's end instead (the read starts or ends inside a flank, or inside the repeat).  The CIGAR
    has ONE '=' run -- over the flank `seed_flank` ("left" / "right") and the read's bases outside the haplotype on that side --
    and 'X' everywhere else, so calc_seed_base (HapAligner.cpp:494-542) seeds the middle of what the read holds of that flank:
    seed = left_pad + (lf_len - 1) // 2 for a whole left flank, mirrored on the right.  With fewer than 9 flank bases under the
    '=' run there is no seed (MIN_SEED_DIST): the builder promises no side length, callers read it back (sides()).
    plant_quals / plant_bases: {read position (negative: from the end): byte} written over the random qualities '#'..'J' /
    over the bases."""
    lf, rep, rf = blocks[0]["alleles"][0], blocks[1]["alleles"][allele], blocks[2]["alleles"][0]
    hap = lf + rep + rf
    assert -left_pad < len(hap) and -right_pad < len(hap) and max(-left_pad, 0) + max(-right_pad, 0) < len(hap)
    seq = _rand_seq(rng, max(left_pad, 0)) + hap[max(-left_pad, 0):len(hap) - max(-right_pad, 0)] + _rand_seq(rng, max(right_pad, 0))
    n = len(seq)
    if seed_flank == "left":
        n_eq = max(min(left_pad + len(lf), n), 0)
        cigar = [("=", n_eq), ("X", n - n_eq)]
        start = blocks[0]["start"] - left_pad                            # the '=' run ends where the left flank ends
    else:
        assert seed_flank == "right"
        n_eq = max(min(right_pad + len(rf), n), 0)
        cigar = [("X", n - n_eq), ("=", n_eq)]
        start = blocks[2]["end"] + right_pad - n                         # the '=' run starts where the right flank starts
    cigar = [(t, k) for t, k in cigar if k > 0]
    qual = rng.integers(ord("#"), ord("J") + 1, size=n).astype(np.uint8)
    for pos, q in (plant_quals or {}).items():
        qual[pos] = q if isinstance(q, int) else ord(q)
    seq = bytearray(seq)
    for pos, c in (plant_bases or {}).items():
        seq[pos] = c if isinstance(c, int) else ord(c)
    return dict(start=start, stop=start + n - 1, seq=bytes(seq), cigar=cigar, qual=qual.tobytes())


def left_pad_for(lf_len, side):
    """left_pad of a left-seeded read whose LEFT side (= its seed) is `side` bases; the smallest reachable is 4."""
    mid = (lf_len - 1) // 2
    return side - mid if side >= mid else 2 * side + 1 - lf_len


def right_pad_for(rf_len, side):
    """right_pad of a right-seeded read whose RIGHT side (len - seed - 1) is `side` bases; the smallest reachable is 4."""
    mid = rf_len // 2
    return side - mid if side >= mid else 2 * side + 1 - rf_len


def sides(alns, seeds):
    """(left, right) alignment side of every read from the seeds a scorer returned: (seed, len - seed - 1)."""
    return [(int(s), len(a["seq"]) - int(s) - 1) for a, s in zip(alns, seeds)]


# ---- short_geometry (ltr_short.hip) restated: S, the chunk capacity, the block kernel's LDS bytes, the kernel path
K_NUM_ART, K_MAX_DEL = 13, 6                      # artifact sizes -6 .. +6, MAX_STUTTER_REPEAT_DEL


def geometry(max_side, max_block, max_hap, n_pairs):
    S = max(max_side, max_block + 2, K_NUM_ART) + 2
    HS = max_hap + 4
    n_ilog = max_hap + max_block + 16
    lds = (4 * S + n_ilog) * 8 + (K_MAX_DEL * max_block + 8) * 4 + ((S + 7) & ~7) + HS + 64
    cap = max(1, min(n_pairs, (2 ** 30 - 64) // (2 * K_NUM_ART * 8 * S)))
    return dict(S=S, HS=HS, lds_bytes=lds, chunk_cap=cap, four_launch=max(max_side, 1) <= 512 and lds <= 64 * 1024)


def geometry_of(blocks, side_list, n_pairs):
    """geometry() of one process_reads call: side_list = sides() of the reads that are scored."""
    mb = max(len(a) for a in blocks[1]["alleles"])
    return geometry(max(max(s) for s in side_list), mb, len(blocks[0]["alleles"][0]) + mb + len(blocks[2]["alleles"][0]), n_pairs)


# ---- the cases of tests/test_gpu_short_geometry.py (GPU against the restatement) and tests/test_short_geometry_cases.py (the
# restatement alone): (blocks, alns) per case, built once per process
EDGE_SIDES = [4, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]       # 4: the smallest a seed allows
PAST_512 = [513, 700]
FLANK_SHAPES = [(1, 12), (12, 1), (2, 9), (9, 2), (31, 31), (32, 32), (33, 32), (70, 70), (200, 9)]
_cases = {}


def _cached(fn):
    def get(*args):
        key = (fn.__name__,) + args
        if key not in _cases:
            _cases[key] = fn(*args)
        return _cases[key]
    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


def _edge_reads(blocks, rng, side_list, n_alleles, special=False):
    """per wanted side: a left-seeded read with that LEFT side and a right-seeded read with that RIGHT side; the other side
    is short (the read ends a few bases into the far flank)."""
    lf_len, rf_len = len(blocks[0]["alleles"][0]), len(blocks[2]["alleles"][0])
    alns = []
    for k, s in enumerate(side_list):
        far = -int(rng.integers(max(rf_len - 8, 0), rf_len))             # 1 .. 8 bases of the far flank stay
        pq = pb = None
        if special and k % 4 == 1:                                       # extreme qualities, N and lower case on the short side
            pq, pb = {-2: " ", -5: "!", -9: "~", 1: "~", 2: "!"}, {-3: "N", -7: "a", -12: "t"}
        alns.append(crafted_read(blocks, k % n_alleles, left_pad_for(lf_len, s), far, "left", rng, pq, pb))
        far = -int(rng.integers(max(lf_len - 8, 0), lf_len))
        if special and k % 4 == 1:
            pq, pb = {1: " ", 4: "!", 8: "~", -2: "~", -3: "!"}, {2: "N", 6: "a", 11: "g"}
        alns.append(crafted_read(blocks, (k + 1) % n_alleles, far, right_pad_for(rf_len, s), "right", rng, pq, pb))
    return alns


@_cached
def case_a():
    """Side-length edges on the four-launch path: flanks 35/35, alleles A*14, A*15, A*12, every side of EDGE_SIDES on the left
    and on the right, maximum side 512."""
    rng = np.random.default_rng(7001)
    blocks = crafted_locus(35, [b"A" * 14, b"A" * 15, b"A" * 12], 35, rng)
    return blocks, _edge_reads(blocks, rng, EDGE_SIDES, 3, special=True)


@_cached
def case_b():
    """case A's reads plus sides of 513 and 700, left and right: the 512/513 rule sends the call to the lane-per-pair kernel."""
    blocks, alns = case_a()
    return blocks, list(alns) + _edge_reads(blocks, np.random.default_rng(7002), PAST_512, 3)


C_SIDES = [4, 40, 127, 128, 257, 300]             # under 128 and over 256 on either side


@_cached
def case_c(which):
    rng = np.random.default_rng(7100 + which)
    if which == 1:       # num_deletions 0 (empty block), 1, 2, 3, 5, 6
        alleles = [b"A" * n for n in (3, 0, 1, 2, 5, 6, 7, 13)]
    elif which == 2:     # interrupted runs: upstream-match tables with zeros
        alleles = [b"AAAAGAAAAAA", b"AAAAGAAAAAAA", b"AAAGAAAAAAA"]
    elif which == 3:     # the block is longer than the seeded side; sides 10 .. ~370
        alleles = [b"A" * 300, b"A" * 301, b"A" * 298]
    else:                # 4: case 3's locus, every read ends inside the repeat: S comes from the longest block + 2, not from a read
        blocks = case_c(3)[0]
        alns = [crafted_read(blocks, k % 3, left_pad_for(35, s), -(35 + 298 - keep), "left", rng)
                for k, (s, keep) in enumerate([(4, 3), (10, 100), (17, 200), (120, 150), (129, 60), (250, 40)])]
        alns += [crafted_read(blocks, k % 3, -(35 + 298 - keep), right_pad_for(35, s), "right", rng)
                 for k, (s, keep) in enumerate([(5, 250), (64, 200), (130, 100), (256, 30)])]
        return blocks, alns
    blocks = crafted_locus(35, alleles, 35, rng)
    if which == 3:
        alns = _edge_reads(blocks, rng, [10, 17, 100, 128, 200], 3)
        alns.append(crafted_read(blocks, 1, left_pad_for(35, 17), 17, "left", rng))       # a whole read: sides 17 and 370
        alns.append(crafted_read(blocks, 1, 17, right_pad_for(35, 17), "right", rng))
        alns.append(crafted_read(blocks, 2, left_pad_for(35, 300), -30, "left", rng))     # both sides over 256
    else:
        alns = _edge_reads(blocks, rng, C_SIDES, len(alleles), special=True)
    return blocks, alns


@_cached
def case_d(lf_len, rf_len):
    """Flank shapes: the final kernel's entry list has lf_len + rf_len entries.  Two alleles; reads are seeded in whichever
    flank holds a seed (>= 9 bases), with short and long sides."""
    rng = np.random.default_rng(7200 + 7 * lf_len + rf_len)
    blocks = crafted_locus(lf_len, [b"A" * 10, b"A" * 11], rf_len, rng)
    alns = []
    for k, s in enumerate([4, 30, 129, 260]):
        if lf_len >= 9:
            alns.append(crafted_read(blocks, k % 2, left_pad_for(lf_len, max(s, 4)), int(rng.integers(0, 6)) - min(rf_len - 1, 3), "left", rng))
        if rf_len >= 9:
            alns.append(crafted_read(blocks, (k + 1) % 2, int(rng.integers(0, 6)) - min(lf_len - 1, 3), right_pad_for(rf_len, s), "right", rng))
    return blocks, alns


E_DISTINCT, E_MASKED_READS, E_REALIGN_HAP = 48, (5, 29), (1, 0, 1)


@_cached
def case_e():
    """The chunk loop: 48 distinct reads on case A's locus -- two with a side of 512 (left, right), the others short -- for
    tiling past twice the chunk capacity.  Returns (blocks, distinct reads)."""
    blocks = case_a()[0]
    rng = np.random.default_rng(7300)
    alns = [crafted_read(blocks, 0, left_pad_for(35, 512), -30, "left", rng), crafted_read(blocks, 1, -30, right_pad_for(35, 512), "right", rng)]
    while len(alns) < E_DISTINCT:
        k = len(alns)
        if k % 2:
            alns.append(crafted_read(blocks, k % 3, left_pad_for(35, int(rng.integers(4, 40))), -int(rng.integers(20, 34)), "left", rng))
        else:
            alns.append(crafted_read(blocks, k % 3, -int(rng.integers(20, 34)), right_pad_for(35, int(rng.integers(4, 40))), "right", rng))
    assert len(set(a["seq"] for a in alns)) == len(alns)
    return blocks, alns


def case_e_tiling(n_distinct, chunk_cap):
    """(tiles, realign_read of one tile, realign_hap, pairs): the fewest whole tiles with pairs > 2 * chunk_cap."""
    rr = np.ones(n_distinct, dtype=np.uint8)
    rr[list(E_MASKED_READS)] = 0
    rh = np.array(E_REALIGN_HAP, dtype=np.uint8)
    per_tile = int(rr.sum()) * int(rh.sum())
    tiles = 2 * chunk_cap // per_tile + 1
    return tiles, rr, rh, tiles * per_tile


@_cached
def case_f(block_len):
    """The LDS rule: alleles A*block_len, A*(block_len + 1); every read ends inside the repeat, all sides under 512."""
    rng = np.random.default_rng(7400 + block_len)
    blocks = crafted_locus(35, [b"A" * block_len, b"A" * (block_len + 1)], 35, rng)
    alns = [crafted_read(blocks, k % 2, left_pad_for(35, s), -(35 + block_len - keep), "left", rng)
            for k, (s, keep) in enumerate([(4, 20), (17, 300), (130, 200), (300, 480)])]
    alns += [crafted_read(blocks, k % 2, -(35 + block_len - keep), right_pad_for(35, s), "right", rng)
             for k, (s, keep) in enumerate([(5, 470), (64, 100), (257, 250)])]
    return blocks, alns
