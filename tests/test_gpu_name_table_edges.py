"""The read-name table where it can go wrong: names that share all 64 bits of their hash, names whose home slot is the
last of a part or of the table, a bucket of the LDS build that overflows, frames whose insert has a finding.

Random names never meet any of it: the tag compare followed by the compare of the bytes (insert_name, match_name,
k_build_parts), the probe that wraps at the end of the table, the keys k_build_parts spills and k_build_spill inserts,
the fallback from an abandoned build to k_names_pass.  tests/name_model.py writes such names down (twins, with_home) and
says what the serial loops of the reference make of them (table_model); every case runs through k_index_insert, through
k_names_pass from capture records and - in a table of 8192 slots, two parts - through the LDS build, and code, record,
n_entries, index_mem, the answers of probe_delete_np to a permuted second file and alive_np must be the model's.

Names with bytes >= 0x80 keep an image out of the streaming pass, so the 8-byte twins and the twins of 64 bytes go
through the line index only; the twins of 48 bytes (word 5, high half: all bytes below 0x80) and of 128 bytes (word 15)
go every way."""
import os
import re
import subprocess

import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import name_model as nm
from tests.test_gpu_name_keys import INSERT_WAYS, READ, Streamed, profiled
from tests.util import REPO

pytestmark = pytest.mark.gpu
A = fq.abi
FMT = nm.NAME_CASAVA18
TWINS8 = nm.twins(41)                                        # bytes >= 0x80: the line index only
TWINS48 = nm.twins(41, length=48, word=5, high=True)         # 7-bit: every way
TWINS64 = nm.twins(6, length=64, word=7)                     # equal name records (56 bytes), bytes >= 0x80
TWINS128 = nm.twins(6, length=128, word=15, high=True)       # equal name records, 7-bit, beyond what a capture record holds


def headers(names, mate=1):
    return [nm.header_for(x, "casava", True, mate) if x is not None else b"X" + nm.header_for(b"noat", "casava", True, mate)[1:]
            for x in names]


def pads(count, first=0):
    return nm.generated_names("casava", count, first)


TAIL = 32   # generated names behind every frame: more than a 4 KiB chunk of records


def tail(k):
    """The streaming pass does not speculate on the line types of an image's last chunk, so the headers that begin there
    are never captured: every image ends in a chunk of generated names, and the names a case is about lie in front."""
    return pads(TAIL, 9000 + 100 * k)


def run_case(way, expected, frames, asks, want_profile=(), not_profile=(), part_log=None, capacity=None, seven_bit=True):
    """frames: lists of names (None: a header without '@') inserted one after the other; asks: lists of names probed one
    after the other; each gets its tail() - an asking frame the tail of the inserted frame of the same number, or names
    nobody inserted.  Everything the index reports against the model."""
    ins_flags, build = INSERT_WAYS[way]
    frames = [names + tail(k) for k, names in enumerate(frames)]
    asks = [names + tail(k if k < len(frames) else 100 + k) for k, names in enumerate(asks)]
    capacity = capacity or max(1024, 2 * expected)
    model = nm.TableModel(capacity, part_log)
    with Streamed(build) as ctx:
        idx = ctx.name_index(expected)
        st, ran_all = None, set()
        for names in frames:
            img = nm.image(headers(names), seed=len(names), ln=READ)
            if st is None:
                st = A.probe_first_record(img, True)
                assert st.readname_format == FMT
            r = ctx.validate(img, None, st, flags=A.VALIDATE_NO_STATS | ins_flags)
            streamed = seven_bit and None not in names     # (a frame with a finding of its own may be framed another way)
            assert r["n_records"] == len(names) and (r["path"] == 3 if streamed else seven_bit or r["path"] != 3), r
            ir, ran = profiled(ctx, lambda: idx.insert_unique(st))
            ran_all |= ran
            want = model.insert(names)
            assert (ir["code"], ir["record"]) == want, (way, ir, want)
            assert (ir["n_entries"], ir["index_mem"]) == (model.n_entries, model.index_mem), (way, ir, model.n_entries, model.index_mem)
            if way != "index" and streamed:   # the names in front of the tail came from capture records (a chunk border
                hold = sum(1 for h in headers(names[:-TAIL]) if nm.holdable(h, FMT, True, False))   # can cost one each)
                assert idx.names_captured() >= hold - (len(img) + nm.CHUNK - 1) // nm.CHUNK, (idx.names_captured(), hold, len(img))
        assert set(want_profile) <= ran_all and not set(not_profile) & ran_all, (way, sorted(ran_all))
        st2 = None
        for names in asks:
            img = nm.image(headers(names, 2), seed=len(names) + 1, ln=READ)
            if st2 is None:
                st2 = A.probe_first_record(img, True)
                assert st2.readname_format == FMT
            ctx.validate(img, None, st2, flags=A.VALIDATE_NO_STATS | ins_flags)
            mr, ans = idx.probe_delete_np(st2, len(names))
            code, record, want = model.match_delete(names)
            bad = [(i, names[i], int(ans[i]), want[i]) for i in range(len(names)) if int(ans[i]) != want[i]]
            assert not bad, (way, bad[:5])
            assert (mr["code"], mr["record"], mr["n_entries"]) == (code, record, model.entries_left()), (way, mr, code, record)
        assert idx.alive_np(len(model.names)).tolist() == model.alive(), way
        idx.close()
    return model


def permuted(names, seed=1):
    rng = np.random.default_rng(seed)
    return [names[i] for i in rng.permutation(len(names))]


TWIN_SETS = {"8": (TWINS8, False), "48": (TWINS48, True)}


def ways_for(seven_bit, expected):
    """the ways a case can take: names with bytes >= 0x80 never reach the capture, a table of 1024 slots has no build"""
    if not seven_bit:
        return ["index"]
    return ["index", "pass", "build"] if expected >= 4096 else ["index", "pass"]


def twin_cases():
    out = []
    for which, (tw, seven) in TWIN_SETS.items():
        for k in (2, 3, 40):
            for expected in (0, 4096):
                for way in ways_for(seven, expected):
                    out.append(pytest.param(which, k, expected, way, id="%s-%d-%d-%s" % (which, k, expected, way)))
    return out


@pytest.mark.parametrize("which,k,expected,way", twin_cases())
def test_twins_neither_fake_nor_hide_a_repeat(which, k, expected, way):
    """k names of one 64-bit hash among other names: no duplicate; a second file that asks for each once, permuted, gets
    its own bytes' record; an asker that asks twice - the later one is the finding; an unknown twin is FQG_NO_MATCH"""
    tw, seven = TWIN_SETS[which]
    names = pads(30)
    for i in range(k):
        names.insert(3 + 2 * i if k < 40 else 5 + i, tw[i])
    model = nm.table_model(names, 1024)
    assert model.finding() == (0, 0) and len({nm.hash64(x) for x in tw[:k]}) == 1
    ask = permuted(names, k)
    ask.insert(len(ask) // 2, tw[40])            # an unknown twin
    ask.append(tw[0])                            # ... and one asked for a second time
    run_case(way, expected, [names], [ask], seven_bit=seven,
             want_profile={"index": ["k_index_insert"], "pass": ["k_names_insert"], "build": ["k_names_build_parts"]}[way])


@pytest.mark.parametrize("which,expected,way", [pytest.param(w, e, y, id="%s-%d-%s" % (w, e, y)) for w, (t, s) in TWIN_SETS.items()
                                                for e in (0, 4096) for y in ways_for(s, e)])
def test_a_true_repeat_among_twins(which, expected, way):
    """one twin twice and another three times: the finding is the second-smallest record of the earliest repeated name"""
    tw, seven = TWIN_SETS[which]
    names = pads(10) + tw[:8] + pads(10, 10) + [tw[5]] + tw[8:12] + [tw[2], tw[5], tw[5]] + pads(5, 20)
    model = nm.table_model(names, 1024)
    assert model.finding() == (nm.E_DUP_NAME, 28) and names[28] == tw[5]
    run_case(way, expected, [names], [permuted(names, 3)], seven_bit=seven)
    # ... and with the later-starting name repeated first in the file
    names = pads(10) + tw[:8] + [tw[7], tw[1]] + pads(5, 20) + [tw[1]]
    assert nm.table_model(names, 1024).finding() == (nm.E_DUP_NAME, 18)
    run_case(way, expected, [names], [], seven_bit=seven)


@pytest.mark.parametrize("which,expected,way", [pytest.param(w, e, y, id="%s-%d-%s" % (w, e, y))
                                                for w, s in (("64", False), ("128", True)) for e in (0, 4096) for y in ways_for(s, e)])
def test_twins_beyond_the_name_record(which, expected, way):
    """twins of 57 bytes and more that agree in their first 56: hash, tag AND name record are equal, so the bytes come
    through the images - a repeat among them, an asker for each, an asker whose name is in no image"""
    tw = TWINS64 if which == "64" else TWINS128
    assert len({x[:56] for x in tw}) == 1 and len({nm.hash64(x) for x in tw}) == 1
    names = pads(12) + tw[:4] + pads(6, 12) + [tw[1]]
    assert nm.table_model(names, 1024).finding() == (nm.E_DUP_NAME, 22)
    ask = [tw[3], tw[5], tw[0]] + permuted(names[:12], 4) + [tw[2], tw[1], tw[1]]
    run_case(way, expected, [names], [ask], seven_bit=which == "128")
    # in one order, where the asker first looks at the name record at its own place
    clean = pads(12) + tw[:4]
    run_case(way, expected, [clean], [clean[:13] + [tw[2], tw[1], tw[0], tw[3]]], seven_bit=which == "128")


HOMES = nm.with_home({4094, 4095, 8191}, 8191, 6)
HOMES_1K = nm.with_home({1022, 1023}, 1023, 5)


@pytest.mark.parametrize("way", ["index", "pass", "build"])
def test_homes_at_the_end_of_a_part_and_of_the_table(way):
    """names whose home is slot 4095 (all but one leave their part) and 8191 (all but one wrap to slot 0), 4094 and 4095
    mixed, a repeat whose copies both spill, a repeat with one copy placed and one spilled"""
    a, b, c = HOMES[4095], HOMES[8191], HOMES[4094]
    names = pads(40) + [a[0], b[0], a[1], c[0], a[2], b[1], c[1], a[3], b[2], b[3], c[2], a[4]] + pads(40, 40)
    model = nm.table_model(names, 8192, part_log=12)
    assert model.finding() == (0, 0)
    spilled = {names[r] for r in model.spilled}
    assert spilled >= {a[1], a[2], a[3], a[4], b[1], b[2], b[3]} and len(spilled & set(c)) >= 1
    assert all(model.slot_of(x)[0] < 8 for x in b[1:4])                 # wrapped past the end of the table
    ask = permuted(names, 5) + [HOMES[4095][5], HOMES[8191][5]]         # two names nobody inserted, same homes
    want = {"index": ["k_index_insert"], "pass": ["k_names_insert"], "build": ["k_names_build_parts", "k_names_build_spill"]}[way]
    run_case(way, 4096, [names], [ask], want_profile=want, part_log=12)
    # a[2] again: both copies spill.  a[0] again behind it: the first copy is (under the serial order) the one placed
    rep = names[:50] + [a[2]] + names[50:] + [a[0]]
    m = nm.table_model(rep, 8192, part_log=12)
    assert m.finding() == (nm.E_DUP_NAME, 50) and rep.index(a[2]) in m.spilled and rep.index(a[0]) not in m.spilled
    run_case(way, 4096, [rep], [permuted(rep, 6)], part_log=12)
    rep = names + [a[0]]
    run_case(way, 4096, [rep], [permuted(rep, 7)], part_log=12)


@pytest.mark.parametrize("way", ["index", "pass"])
def test_homes_at_the_end_of_a_table_of_1024_slots(way):
    a, b = HOMES_1K[1023], HOMES_1K[1022]
    names = pads(20) + [a[0], b[0], a[1], b[1], a[2], a[3], b[2]] + pads(20, 20) + [a[1]]
    model = nm.table_model(names, 1024)
    assert model.finding() == (nm.E_DUP_NAME, 47) and sum(1 for x in a[:4] + b[:3] if model.slot_of(x)[0] < 8) >= 5
    run_case(way, 0, [names], [permuted(names, 8) + [a[4]]])


@pytest.mark.parametrize("way", ["index", "pass", "build"])
def test_two_frames_into_one_index(way):
    """frame 1 spills a name into the next part, frame 2 (the build loads the parts as the table holds them) repeats it,
    adds names of the same home, and repeats a name of its own"""
    a, b = HOMES[4095], HOMES[8191]
    one = pads(60) + [a[0], a[1], b[0], b[1]] + pads(60, 60)
    two = pads(50, 200) + [a[2], b[2]] + pads(10, 300) + [a[1]] + pads(10, 400) + [a[2], b[1]]
    m = nm.TableModel(8192, 12)
    assert m.insert(one) == (0, 0) and m.insert(two) == (nm.E_DUP_NAME, 62)
    assert {a[1], b[1], a[2], b[2]} <= {m.names[r] for r in m.spilled}
    ask1, ask2 = permuted(one + two[:52], 9), permuted(two[52:], 10) + [a[0]]
    want = ["k_names_build_parts"] if way == "build" else []
    run_case(way, 4096, [one, two], [ask1, ask2], want_profile=want, part_log=12)


@pytest.mark.parametrize("way", ["index", "pass"])
def test_a_second_frame_that_makes_the_table_grow(way):
    """an index of 1024 slots and two frames of 400 names: the second makes it grow, and the first frame is inserted
    again through the line index with names = nullptr.  After it every name still answers - twins and names at the end
    of the smaller table among them - and a repeat across the two frames is still found"""
    a = HOMES_1K[1023]
    one = pads(380) + TWINS48[:10] + a[:4] + pads(6, 380)
    two = pads(380, 1000) + TWINS48[10:20] + [a[4]] + pads(8, 2000) + [TWINS48[3]]
    assert len(one) == len(two) == 400
    m = run_case(way, 0, [one, two], [permuted(one + two, 11)], capacity=2048, want_profile=["k_index_insert(regrow)"])
    assert m.findings == [(0, 0), (nm.E_DUP_NAME, 399)]


def build_plan(capacity, n_records, empty=True):
    """what names_build plans for this table: fqg_names_build_plan.h itself, compiled"""
    exe = os.path.join(build_plan.dir, "names_build_plan_print")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "cxx", "names_build_plan_print.cpp")], check=True)
    out = subprocess.run([exe, str(capacity), str(n_records), "1" if empty else "0"], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out)}


def test_a_bucket_that_overflows_abandons_the_build(tmp_path):
    """more names of one hash - one home, one part, one bucket - than the plan gives a bucket room for: the scatter raises
    the flag, k_build_parts leaves the table alone, and k_names_pass inserts the frame.  The smallest count that overflows:
    every probe of these names compares bytes."""
    build_plan.dir = str(tmp_path)
    p = build_plan(8192, 1000)
    assert p["applies"] and (p["part_log"], p["bits0"], p["bits1"]) == (12, 1, 0)     # two parts, one bucket each
    rec_bytes = len(nm.image(headers(TWINS48[:1]), ln=READ))
    others = pads(1) + pads(1, 1) + tail(0)           # the frame's other names: run_case adds the tail
    part = (nm.hash64(TWINS48[0]) & 8191) >> 12       # the twins' part, and so their bucket
    beside = sum(1 for x in others if (nm.hash64(x) & 8191) >> 12 == part)

    def first_that_overflows(lost_per_chunk, beside):
        """the smallest t for which t twins, less the headers that straddle a chunk and so reach the table through
        k_names_rest, are more than a bucket's room in a frame of t twins and the other names; found by bisection - the
        room grows half as fast as t"""
        lo, hi = 8, 4000
        while lo < hi:
            t = (lo + hi) // 2
            lost = lost_per_chunk * ((t + len(others)) * rec_bytes // nm.CHUNK + 1)
            if t + beside - lost > build_plan(8192, t + len(others))["cap0"]:
                hi = t
            else:
                lo = t + 1
        return lo

    t = first_that_overflows(1, 0)
    assert 200 < t < 600, t
    tw = nm.twins(t + 1, length=48, word=5, high=True)
    names = pads(1) + tw[:t] + pads(1, 1)
    ask = permuted(names, 12) + [tw[t]]
    run_case("build", 4096, [names], [ask], want_profile=["k_names_build_scatter0", "k_names_build_parts", "k_names_insert"])
    # the largest count that cannot overflow: the bucket holds, the build stands - some 300 keys of one home, inserted
    # in LDS with a compare of the bytes at every probe, most of them spilled
    t = first_that_overflows(0, beside) - 1
    names = pads(1) + tw[:t] + pads(1, 1)
    assert build_plan(8192, len(names) + TAIL)["cap0"] >= t + beside > 200
    run_case("build", 4096, [names], [permuted(names, 13)], want_profile=["k_names_build_parts"], not_profile=["k_names_insert"],
             part_log=12)


@pytest.mark.parametrize("way", ["index", "pass", "build"])
@pytest.mark.parametrize("what", ["repeat", "wrong_header"])
def test_a_frame_with_a_finding_then_a_second_file(what, way):
    """the caller may go on after an insert has reported a repeat or a header without '@': the table holds the repeated
    name once, at its first record, and the record of the second copy must not stand in for it when the second file - in
    the same order - asks at that place (n_positional is off)"""
    names = pads(100)
    if what == "repeat":
        names[50] = names[10]
        names[70] = TWINS48[0]
        names[80] = TWINS48[0]
    else:
        names[30] = None
        names[60] = names[20]
    model = nm.table_model(names, 8192)
    assert model.finding() == ((nm.E_DUP_NAME, 50) if what == "repeat" else (nm.E_WRONG_HEADER, 30))
    code, record, want = nm.table_model(names, 8192).match_delete(names)
    assert (code, record) == ((nm.E_UNPAIRED, 50) if what == "repeat" else (nm.E_WRONG_HEADER, 30))
    assert want[50 if what == "repeat" else 60] == nm.NO_MATCH
    run_case(way, 4096, [names], [names])
