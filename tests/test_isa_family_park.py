"""How a family along a spine parks a row (csrc/ltr_dp_family.hpp, spine_walk's park_if), read off the gfx950 assembly of the fifteen
spine bodies (tests/isa_util.py; no GPU).  The stream's step loop is the one step loop with vector stores in it.  A parking step must
not wait for memory: the lane's chunk of a slot is 2W+2 consecutive doubles, so the loop holds exactly W+1 stores, all 128-bit; the
slot's row and range come from LDS, so the only vector-memory loads of the loop are the step's own two prefetches (the next haplotype
row code, the next column-0 record); and those are waited for before the park branch, so no wait on the vector-memory counter lies
between the first park store and the loop's back edge -- the counter is in order, and such a wait would drain the stores."""
import os
import re

import pytest

import isa_util

CACHE = os.path.join(isa_util.CSRC, "build", "isa")

_VSTORE = re.compile(r"^\s*(global|buffer|flat)_store_(\w+)")
_VLOAD = re.compile(r"^\s*(global|buffer|flat)_load_(\w+)")
_VATOMIC = re.compile(r"^\s*(global|buffer|flat)_atomic_")
_WAIT_VM = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")


@pytest.fixture(scope="module")
def bodies():
    """{W: (the function's info, its assembly lines)} of spine_narrow_call<6 .. 10> and spine_wide_call<11 .. 20>."""
    asm = isa_util.assembly("ltr_k_family.hip", cache_dir=CACHE)
    funcs = isa_util.parse(asm)
    lines = asm.splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^\s*\.type\s+\S+,@function", l)] + [len(lines)]
    out = {}
    for name, v in funcs.items():
        if not re.search(r"\bspine_(narrow|wide)_call<", name):
            continue
        (s,) = [i for i in starts[:-1] if re.match(r"^\s*\.type\s+%s,@function" % re.escape(v["mangled"]), lines[i])]
        out[int(re.search(r"<(\d+)>", name).group(1))] = (v, lines[s:starts[starts.index(s) + 1]])
    return out


def _stream_loop(w, v, body):
    with_stores = [L for L in v["step_loops"] if any(_VSTORE.match(x) for x in body[L["first"]:L["last"] + 1])]
    assert len(with_stores) == 1, (w, [(L["first"], L["last"]) for L in with_stores])
    (L,) = with_stores
    return body[L["first"]:L["last"] + 1]


def test_the_stream_parks_a_row_without_waiting_for_memory(bodies):
    assert sorted(bodies) == list(range(6, 21))
    for w, (v, body) in sorted(bodies.items()):
        seg = _stream_loop(w, v, body)
        stores = [(k, _VSTORE.match(x).group(2)) for k, x in enumerate(seg) if _VSTORE.match(x)]
        loads = [_VLOAD.match(x).group(0).strip() for x in seg if _VLOAD.match(x)]
        atomics = sum(1 for x in seg if _VATOMIC.match(x))
        first_store = stores[0][0]
        waits_behind = [x.strip() for x in seg[first_store:] if _WAIT_VM.match(x)]
        waits_before = [x.strip() for x in seg[:first_store] if _WAIT_VM.match(x)]
        print("spine call<%d>: stream loop of %d lines, %d vector stores (%s), vector loads %s, vmcnt waits before / behind the first store: %d / %d"
              % (w, len(seg), len(stores), ",".join(sorted({s for _, s in stores})), loads, len(waits_before), len(waits_behind)))
        # the lane's chunk: W+1 stores of 16 bytes, nothing narrower
        assert len(stores) == w + 1 and all(s == "dwordx4" for _, s in stores), (w, stores)
        # the step's own two prefetches and no other vector-memory load (the slot's row and range are LDS reads); no atomic
        assert sorted(loads) == ["buffer_load_dwordx4", "buffer_load_ushort"], (w, loads)
        assert atomics == 0, (w, atomics)
        # no wait on the vector-memory counter from the first park store to the back edge
        assert waits_behind == [], (w, waits_behind)
        # ... and none right behind the back edge either: a wait at the loop's head, before the step's own prefetches are all issued,
        # could only be for something older than them -- the stores of the step before (the loop is entered with no load pending)
        last_load = max(k for k, x in enumerate(seg) if _VLOAD.match(x))
        assert last_load < first_store and not any(_WAIT_VM.match(x) for x in seg[:last_load]), (w, waits_before)


def test_a_tail_reloads_its_chunk_with_as_many_wide_loads(bodies):
    """Outside the step loops: the tails' set-up reloads the lane's chunk, W+1 loads of 16 bytes, and no 8-byte global load of a
    parked double is left anywhere in the body."""
    for w, (v, body) in sorted(bodies.items()):
        in_loop = set()
        for L in v["step_loops"]:
            in_loop.update(range(L["first"], L["last"] + 1))
        wide = [x for k, x in enumerate(body) if k not in in_loop and re.match(r"^\s*global_load_dwordx4\b", x)]
        print("spine call<%d>: %d global 128-bit loads outside the step loops" % (w, len(wide)))
        assert len(wide) >= w + 1, (w, len(wide))
