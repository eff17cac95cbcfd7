"""tests/name_model.py against what does not depend on the code under test: the canonical name against the oracle's
restatements of fastq_get_readname over the whole ladder, the constructed names against their promises, the table model
against the serial loops of the oracle and against tables worked out by hand."""
import numpy as np
import pytest

from oracle import loader as orc
from oracle import pre_barcodes_oracle as pbo
from tests import name_model as nm


def oracle_readname(line, fmt):
    """fastq_get_readname with is_pe set, as fastq_pre_barcodes uses it"""
    f = pbo.MemFile("x.fastq", b"")
    f.fmt, f.space = fmt, 0
    e = pbo.Entry()
    e.hdr1, e.seq = line + b"\n", b"ACGT\n"
    return pbo.get_readname(pbo.Run(), f, e)


@pytest.mark.parametrize("style,is_pe", [m for m in nm.MODES if m[1]])
def test_canonical_is_the_oracles_readname_on_every_ladder_entry(style, is_pe):
    fmt = nm.FMT_OF[style]
    entries = nm.ladder(style, is_pe) + nm.degenerate(style)[:1]
    assert len(entries) > 40
    for line, note in entries:
        n, acct, at = nm.canonical(line, True, fmt, is_pe)
        assert at
        want = oracle_readname(line, fmt)
        assert nm.canonical_name(line, True, fmt, is_pe) == want and n == len(want), (style, note, line[:80])
        assert acct == (n if style == "casava" else max(len(line) - (1 if style == "slash" else 0), 0)), (note, acct)


@pytest.mark.parametrize("style,is_pe", [m for m in nm.MODES if m != ("slash", True)])
def test_canonical_is_the_name_fastq_info_reports_as_repeated(style, is_pe):
    """one file, not paired: the reference's is_pe is off (this is the only oracle for `slash` without is_pe).  An image
    of the format's lead record and a ladder header twice: the second copy is the finding, and the message names the
    canonical name."""
    fmt = nm.FMT_OF[style]
    for line, note in nm.ladder(style, False):
        name = nm.canonical_name(line, True, fmt, False)
        if b"\0" in name or name == nm.canonical_name(nm.lead_header(style), True, fmt, False):
            continue
        img = nm.image([nm.lead_header(style), line, line], ln=12)
        got = orc.fastq_info(img, "f.fastq")
        assert got["first"]["code"] == nm.E_DUP_NAME and got["first"]["record"] == 2, (style, note, got["first"], got["stderr"][-200:])
        assert ("duplicated sequence " + name.decode("latin-1") + "\n") in got["stderr"] + "\n", (style, note, got["stderr"][-300:])
        # ... and the name does not end earlier: the header with its last name byte changed is no repeat
        n = len(name)
        if n and name[-1:] != b"\n":
            other = line[:n] + (b"#" if line[n:n + 1] != b"#" else b"%") + line[n + 1:]
            got = orc.fastq_info(nm.image([nm.lead_header(style), line, other], ln=12), "f.fastq")
            assert got["first"]["code"] == 0, (style, note, got["first"])


def test_the_ladder_keeps_its_edges():
    """what the GPU tests rely on: every length and every blank place of the issue is there, under every mode"""
    for style, is_pe in nm.MODES:
        fmt = nm.FMT_OF[style]
        ent = nm.ladder(style, is_pe)
        lens = {nm.canonical(h, True, fmt, is_pe)[0] for h, _ in ent}
        lens |= {nm.canonical(h, True, fmt, is_pe)[0] for h, _ in nm.degenerate(style)[:1]}
        assert set(nm.NAME_LENGTHS) <= lens, (style, sorted(set(nm.NAME_LENGTHS) - lens))
        lines = {len(h) for h, _ in ent}
        assert set(nm.LINE_LENGTHS + nm.LONGEST_LINES) <= lines, (style, sorted(lines))
        assert max(lines) == nm.MAX_LABEL - 2
        if style == "casava":
            blanks = {h.find(b" ") for h, _ in ent}
            assert set(nm.BLANK_AT) | {-1} <= blanks
            slashes = {h.find(b" ") for h, _ in ent if h[h.find(b" ") - 2:h.find(b" ") - 1] == b"/" and h.find(b" ") >= 3}
            assert {p for p in nm.BLANK_AT if p >= 3} <= slashes
        kept = nm.distinct(ent, fmt, is_pe)
        assert len(kept) >= len(ent) - (14 if style == "casava" else 4), (style, len(kept), len(ent))


def test_hash_words_and_check_bits():
    # the seed carries the length, a word counts only when it holds a name byte, zero bytes behind the name
    assert nm.hash64(b"") == nm.name_fin(0x2545F4914F6CDD1D)
    assert nm.hash64(b"a") != nm.hash64(b"a\0")
    assert nm.name_mul(0) == 0x9E3779B97F4A7C15 and nm.name_mul(1) & 1
    assert nm.zero_half(0, False) == bytes.fromhex("EB83B580") and nm.zero_half(0, True) == bytes.fromhex("4786C861")
    assert nm.zero_half(5, True) == b"I\x13>I"
    # the second hash closes with the partial word - an empty one at a multiple of eight
    assert nm.hash2(b"abcdefgh") != nm.hash2(b"abcdefgh\0")
    assert nm.owner(0, 64) == 0 and nm.owner(nm.M64, 64) == 63 and nm.owner(1 << 63, 3) == 1
    assert nm.name_record(b"ab") == b"\x02" + b"\0" * 7 + b"ab" + b"\0" * 54
    assert nm.name_record(b"x" * 70, at_sign=False)[:8] == (70 | 1 << 63).to_bytes(8, "little")
    assert nm.travel_record(b"x" * 70) == b"x" * 56 + (70).to_bytes(8, "little")


@pytest.mark.parametrize("kw", [dict(), dict(high=True), dict(length=48, word=5, high=True), dict(length=64, word=7),
                                dict(length=64, word=7, high=True), dict(length=128, word=15, high=True), dict(length=19, word=1)],
                         ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()) or "default")
def test_twins_differ_in_bytes_and_agree_in_all_64_hash_bits(kw):
    t = nm.twins(40, **kw)
    assert len(set(t)) == 40 and {len(x) for x in t} == {kw.get("length", 8)}
    assert len({nm.hash64(x) for x in t}) == 1
    assert len({nm.check23(x) for x in t}) > 30
    if kw.get("word", 0) >= 7:
        assert len({x[:56] for x in t}) == 1     # the name records are equal: only the images tell them apart
    if kw.get("word") in (5, 15) and kw.get("high"):
        assert all(0 < b < 0x80 and b not in b" \n\r/" for x in t for b in x)   # these pass the streaming pass
    # a name that is no twin: the same bytes but one in the zeroing half
    x = bytearray(t[0])
    x[8 * kw.get("word", 0) + (4 if kw.get("high") else 0)] ^= 1
    assert nm.hash64(bytes(x)) != nm.hash64(t[0])


def test_with_home_returns_what_it_promises():
    for style in ("casava", "int"):
        got = nm.with_home({4094, 4095, 8191}, 8191, 4, style)
        assert set(got) == {4094, 4095, 8191}
        for slot, names in got.items():
            assert len(set(names)) == 4 and all(nm.hash64(x) & 8191 == slot for x in names)
            assert style != "int" or all(x.isdigit() for x in names)


@pytest.mark.parametrize("kw", [dict(), dict(high=True), dict(length=48, word=5, high=True), dict(length=64, word=7)])
def test_the_oracle_takes_twin_names_as_different_names(kw):
    """bytes >= 0x80 in a header are no obstacle to the reference; a true repeat among the twins is found, at the
    second-smallest record of the earliest repeated name"""
    t = nm.twins(40, **kw)
    for style, is_pe in (("casava", False), ("slash", False)):
        hdrs = [nm.lead_header(style)] + [nm.header_for(x, style, is_pe) for x in t]
        got = orc.fastq_info(nm.image(hdrs, ln=12), "f.fastq")
        assert got["first"]["code"] == 0 and got["summary"]["num_reads"] == 41, (style, got["first"], got["stderr"][-200:])
        rep = hdrs[:30] + [hdrs[7]] + hdrs[30:] + [hdrs[3], hdrs[7]]
        got = orc.fastq_info(nm.image(rep, ln=12), "f.fastq")
        assert (got["first"]["code"], got["first"]["record"]) == (nm.E_DUP_NAME, 30)
        names = [nm.canonical_name(h, True, nm.FMT_OF[style], is_pe) for h in rep]
        assert nm.table_model(names, 1024).finding() == (nm.E_DUP_NAME, 30)


def test_table_model_by_hand():
    """a table of 8 slots, names chosen by their home slot: probing, the wrap, the spill of a part of 4 slots"""
    home = nm.with_home({3, 7}, 7, 3)
    a, b, c = home[7]
    d, e, f = home[3]
    names = [a, d, b, e, c, a, None, f]
    m = nm.table_model(names, 8, part_log=2)
    rec = lambda s: None if s is None else s & ((1 << 40) - 1)  # noqa: E731
    # a -> 7; d -> 3; b: 7 taken, wraps to 0; e: 3 taken -> 4; c: 7, 0 taken -> 1; f: 3, 4 taken -> 5
    assert [rec(s) for s in m.slots] == [2, 4, None, 1, 3, 7, None, 0]
    assert all(m.slots[i] >> 40 == nm.hash64(names[rec(m.slots[i])]) >> 40 for i in (0, 1, 3, 4, 5, 7))
    assert m.spilled == [2, 3, 4, 7]          # parts are slots 0..3 and 4..7: whoever meets its part's end spills
    assert m.finding() == (nm.E_DUP_NAME, 5) and m.first_wrong == 6
    assert m.n_entries == 6 and m.index_mem == 8 + 6 * 41 + sum(len(x) for x in (a, b, c, d, e, f))
    assert m.slot_of(c) == (1, 2) and m.slot_of(b"nobody")[0] is None
    # askers: c, an unknown name, a header without '@', a, c again, then (a second frame) a again and f
    code, record, ans = m.match_delete([c, b"nobody", None, a, c])
    assert (code, record) == (nm.E_UNPAIRED, 1) and ans == [4, nm.NO_MATCH, nm.MATCH_WRONG_HEADER, 0, nm.NO_MATCH]
    code, record, ans = m.match_delete([a, f])
    assert (code, record) == (nm.E_UNPAIRED, 0) and ans == [nm.NO_MATCH, 7]
    assert m.alive() == [0, 1, 1, 1, 0, 0, 0, 0] and m.entries_left() == 3
    # without parts nothing spills; a header without '@' in front of the repeat is the finding
    assert nm.table_model([None, a, a], 8).finding() == (nm.E_WRONG_HEADER, 0)
    assert nm.table_model(names, 8).spilled == []


@pytest.mark.parametrize("case", ["clean", "repeat", "three_times", "asked_twice", "unknown", "short", "permuted"])
def test_table_model_follows_the_oracles_serial_loops(case):
    """fastq_info on two files (src/fastq_info.c:333-356) stops where the model's findings are"""
    rng = np.random.default_rng(3)
    names = nm.generated_names("casava", 60) + nm.twins(6)
    n = len(names)
    one, two = list(range(n)), list(rng.permutation(n)) if case == "permuted" else list(range(n))
    if case == "repeat":
        one = one[:40] + [12] + one[40:]
    if case == "three_times":
        one = one[:20] + [5] + one[20:50] + [3, 5] + one[50:]
    if case == "asked_twice":
        two = two[:30] + [63] + two[30:]
    if case == "short":
        two = two[:50]
    ask = [names[i] for i in two]
    if case == "unknown":
        ask[17] = nm.twins(7)[6]
    img1 = nm.image([nm.lead_header("casava", 1)] + [nm.header_for(names[i], "casava", True, 1) for i in one], ln=12)
    img2 = nm.image([nm.lead_header("casava", 2)] + [nm.header_for(x, "casava", True, 2) for x in ask], ln=12)
    lead = nm.canonical_name(nm.lead_header("casava"), True, nm.NAME_CASAVA18, True)
    m = nm.table_model([lead] + [names[i] for i in one], 1024)
    whole = orc.fastq_info(img1, "a.fastq", img2, "b.fastq", orc.ARG2_FILE)
    got = whole["first"]
    if m.finding()[0]:
        assert (got["code"], got["file"], got["record"]) == (m.finding()[0], 0, m.finding()[1]), (got, m.finding())
        return
    code, record, ans = m.match_delete([lead] + ask)
    if code:
        assert (got["code"], got["file"], got["record"]) == (code, 2, record), (got, code, record)
    elif m.entries_left():
        assert "found %d unpaired reads" % m.entries_left() in whole["stderr"], whole["stderr"][-300:]   # (nobody asked for them)
    else:
        assert got["code"] == 0, got
        assert sorted(ans) == list(range(n + 1))


def test_run_models_by_hand():
    F2, chk = nm.FP_FILE2, lambda c: c << 40  # noqa: E731
    fps = [50, 10, 10, 20, 30, 30, 40, 40, 40, 50, 60, 60]
    idx = [0 | chk(1), 1 | chk(3), F2 | 2 | chk(3), 3, F2 | 9, F2 | 4, 5, 6, F2 | 7, F2 | 8 | chk(2), 10, 11]
    s, ent = nm.pair_runs_model(fps, idx)
    # 10: a pair; 20: one holder left over; 30: two askers; 40: (2, 1) complex; 50: (1, 1) with other check bits; 60: (2, 0)
    assert s == {"matched": 1, "leftover": 3, "unpaired": 2, "first_unpaired": 4, "n_complex": 5}
    assert ent == sorted([(5, 5), (5, 6), (5, F2 | 7), (8, 0), (8, F2 | 8)])
    assert nm.candidates_model(fps, idx) == sorted([(1, F2 | 2), (F2 | 4, F2 | 9), (5, 6), (5, F2 | 7), (0, F2 | 8), (10, 11)])
    # with names: the pair of run 10 holds only when the records are the same bytes of a name that fits one
    rec = [nm.travel_record(b"n%d" % (f if f != 50 else i)) for i, f in enumerate(fps)]
    assert nm.pair_runs_model(fps, idx, rec)[0]["matched"] == 1
    rec[2] = nm.travel_record(b"other")
    s, ent = nm.pair_runs_model(fps, idx, rec)
    assert s["matched"] == 0 and s["n_complex"] == 7 and (0, 1) in ent and (0, F2 | 2) in ent
    rec[1] = rec[2] = nm.travel_record(b"L" * 57)
    assert nm.pair_runs_model(fps, idx, rec)[0]["n_complex"] == 7
