"""The line-type masks of the streaming pass as SPANS between a lane's newlines (fqg_type_spans.h, stream_pass1_body):
findings placed where a span that is off by one - or one that holds its newline - would show, images of very short reads
whose lanes hold three newlines (the span form's limit) and four or more (the chunk leaves its class tests to the redo
kernel), a wrong speculation, and the two name modes on such an image.

Every image is 2 - 4 MiB (the streaming path starts at 1 MiB) and is judged three ways: the result fields and the
accumulator of the streaming pass equal those of the two-pass path (FQG_VALIDATE_TWO_PASS, whose kernels know every
line's true rank), and both give what the oracle (`fastq_info -r`) gives.

The C-ABI has no counter of the chunks that went to the redo list (k_stream_redo is launched in every call, so its
profile entry says nothing): the tests with four-newline lanes assert the results only."""
import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import loader as orc

pytestmark = pytest.mark.gpu
A = fq.abi
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK, SLICE, LANE = 4096, 2048, 32
KEYS = ("code", "record", "aux0", "aux1", "n_records", "n_lines", "consumed", "tail_lines", "stopped")


@pytest.fixture(scope="module")
def ctx():
    c = fq.Context(0)
    yield c
    c.close()


def record(name, seq, qual):
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def records(seed, n, lo, hi, name_len=None):
    """n records (name, sequence, quality) with reads of lo..hi bases, qualities '#'..'I'; name_len(rng, i) -> bytes to
    pad the name with"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    total = int(lens.sum())
    seq = BASES[rng.integers(0, 4, total)]
    qual = (rng.integers(2, 41, total) + 33).astype(np.uint8)
    out, at = [], 0
    for i in range(n):
        L = int(lens[i])
        pad = name_len(rng, i) if name_len else 0
        out.append([b"R%d" % i + b"_" * pad, seq[at:at + L].tobytes(), qual[at:at + L].tobytes()])
        at += L
    return out


def join(recs):
    return b"".join(record(*r) for r in recs)


def run(ctx, img, flags=0):
    st = A.probe_first_record(img, False)
    acc = ctx.accumulator()
    try:
        r = ctx.validate(img, acc, st, flags=flags)
        return r, acc.read(), acc.median()
    finally:
        acc.close()


def check(ctx, img, want_path=3):
    """streaming pass == two-pass path == oracle; returns the streaming result"""
    assert (2 << 20) <= len(img) <= (4 << 20), len(img)
    r, s, med = run(ctx, img)
    assert r["path"] == want_path, r
    r2, s2, med2 = run(ctx, img, A.VALIDATE_TWO_PASS)
    assert r2["path"] == 2, r2
    assert {k: r[k] for k in KEYS} == {k: r2[k] for k in KEYS}, (r, r2)
    if r["code"] == 0:
        assert s == s2 and med == med2, (s, s2, med, med2)
    want = orc.fastq_info(img, "t.fastq", flags=orc.FLAG_R)
    first = want["first"]
    assert r["code"] == first["code"], (r, first)
    if r["code"]:
        assert r["record"] == first["record"] and r["aux0"] == first["aux0"], (r, first)
    else:
        w = want["summary"]
        assert (s["num_rds"], s["min_rl"], s["max_rl"], s["min_qual"], s["max_qual"], med) == (
            w["num_reads"], w["min_rl"], w["max_rl"], w["min_qual"], w["max_qual"], w["median_rl"]), (s, med, w)
    return r, s


def place(recs, k, delta, want):
    """pad the names of the records in front of record k so that the byte `delta` bytes behind record k's '@' lands at
    offset `want` of its 4 KiB chunk.  Returns (records, position of that byte in the image)."""
    recs = [list(r) for r in recs]
    start = sum(len(r[0]) + len(r[1]) + len(r[2]) + 6 for r in recs[:k])
    shift = (want - (start + delta)) % CHUNK
    i = k - 1
    while shift:
        step = min(shift, 40)
        recs[i][0] += b"x" * step
        shift -= step
        i -= 1
    assert i >= 0
    pos = sum(len(r[0]) + len(r[1]) + len(r[2]) + 6 for r in recs[:k]) + delta
    assert pos % CHUNK == want
    return recs, pos


def lane_newlines(img):
    """newlines in each aligned 32-byte piece of the image's whole chunks"""
    a = np.frombuffer(img, dtype=np.uint8)[:len(img) // CHUNK * CHUNK]
    return (a == 10).reshape(-1, LANE).sum(axis=1)


# ---- placed findings ------------------------------------------------------------------------------------------------
# (which byte of the line, slice, lane, bit of the lane's 32 bytes)
PLACES = [
    ("first", 0, 0, 0),    # behind a newline that is the last byte of the chunk in front
    ("first", 1, 0, 0),    # behind a newline that is the last byte of slice 0
    ("first", 0, 17, 0),   # behind a newline that is a lane's last byte
    ("first", 1, 40, 31),  # the newline in front at bit 30
    ("first", 0, 63, 1),   # the newline in front at bit 0
    ("last", 0, 63, 31),   # its newline is the first byte of slice 1
    ("last", 1, 63, 31),   # its newline is the first byte of the next chunk
    ("last", 1, 63, 30),   # its newline is the chunk's last byte
    ("last", 0, 5, 0),     # its newline at bit 1
    ("last", 1, 0, 30),    # its newline at bit 31
    ("mid", 0, 0, 31),
    ("mid", 0, 63, 0),
    ("mid", 1, 0, 0),
    ("mid", 1, 63, 31),
]
_BASE = {}


def base_records(L):
    if L not in _BASE:
        n = (3 << 20) // (2 * L + 40)
        _BASE[L] = records(100 + L, n, L, L, name_len=lambda rng, i: int(rng.integers(0, 24)))
    return _BASE[L]


@pytest.mark.parametrize("what", ["bad_base", "qual_below", "qual_above"])
@pytest.mark.parametrize("L", [150, 100, 36])
def test_placed_findings(ctx, L, what):
    recs0 = base_records(L)
    k = len(recs0) // 2 + 7
    for which, sl, lane, bit in PLACES:
        in_line = {"first": 0, "last": L - 1, "mid": L // 2}[which]
        name = recs0[k][0]
        line = 1 if what == "bad_base" else 3
        delta = (len(name) + 2 if line == 1 else len(name) + 2 + L + 3) + in_line
        recs, pos = place(recs0, k, delta, sl * SLICE + lane * LANE + bit)
        byte = {"bad_base": b"X", "qual_below": b"!", "qual_above": b"~"}[what]
        field = bytearray(recs[k][1 if line == 1 else 2])
        field[in_line] = byte[0]
        recs[k][1 if line == 1 else 2] = bytes(field)
        img = join(recs)
        assert img[pos:pos + 1] == byte and (img[pos - 1] == 10) == (which == "first") and (img[pos + 1] == 10) == (which == "last")
        r, s = check(ctx, img)
        where = (L, what, which, sl, lane, bit)
        if what == "bad_base":
            assert r["code"] == 6 and r["record"] == k, (where, r)
        elif what == "qual_below":
            assert r["code"] == 0 and s["min_qual"] == ord("!") and s["max_qual"] == 73, (where, r, s)
        else:
            assert r["code"] == 0 and s["min_qual"] == 35 and s["max_qual"] == ord("~"), (where, r, s)


# ---- three newlines in a lane, and four or more ---------------------------------------------------------------------
def short_records(kind):
    """very short reads.  A third of the names are a few bytes long - with a read of a few bases the whole record fits
    a lane's 32 bytes -, the others long enough to keep every chunk below the 256 newlines the staging area holds."""
    def name_len(rng, i):
        return 0 if rng.random() < 0.33 else int(rng.integers(90, 130))
    if kind == "1_28":
        return records(7, 26000, 1, 28, name_len)
    recs = records(8, 14000, 1, 150, name_len)
    tiny = records(9, 14000, 1, 28, name_len)
    return [tiny[i] if i % 2 else recs[i] for i in range(len(recs))]


def byte_tables(img):
    """per byte of the image: type of its line (index mod 4), newlines of its lane, most newlines in a lane of its chunk"""
    a = np.frombuffer(img, dtype=np.uint8)
    nl = a == 10
    ltype = ((np.cumsum(nl) - nl) & 3).astype(np.uint8)
    whole = len(img) // CHUNK * CHUNK
    lanes = lane_newlines(img)
    per_byte_lane = np.repeat(lanes, LANE)
    per_byte_chunk = np.repeat(lanes.reshape(-1, CHUNK // LANE).max(axis=1), CHUNK)
    return a[:whole], nl[:whole], ltype[:whole], per_byte_lane, per_byte_chunk


def record_of(img, pos):
    return img.count(b"\n", 0, pos) // 4


@pytest.mark.parametrize("kind", ["1_28", "1_150"])
def test_three_and_four_newlines_in_a_lane(ctx, kind):
    img = join(short_records(kind))
    a, nl, ltype, in_lane, in_chunk = byte_tables(img)
    lanes = lane_newlines(img)
    assert (lanes == 3).any() and (lanes >= 4).any() and lanes.reshape(-1, CHUNK // LANE).sum(axis=1).max() <= 256
    r, _ = check(ctx, img)
    assert r["code"] == 0
    # a finding in a lane of four or more newlines (the redo kernel's), in a lane of exactly three next to one, and - where
    # the image has such a chunk - in a lane of exactly three in a chunk that keeps its class tests
    later = np.arange(len(a)) > (1 << 20)
    cases = {"dense": in_lane >= 4, "three_beside_dense": (in_lane == 3) & (in_chunk >= 4), "three": (in_lane == 3) & (in_chunk == 3)}
    for name, sel in cases.items():
        for line, byte in ((1, b"X"), (3, b"!"), (3, b"~")):
            hits = np.flatnonzero(sel & later & (ltype == line) & ~nl)
            if name == "three" and kind == "1_28":
                continue  # (nearly every chunk of this image has a denser lane)
            assert len(hits), (kind, name, line)
            p = int(hits[len(hits) // 2])
            bad = img[:p] + byte + img[p + 1:]
            r, s = check(ctx, bad)
            if line == 1:
                assert r["code"] == 6 and r["record"] == record_of(img, p), (kind, name, p, r)
            else:
                assert r["code"] == 0 and (s["min_qual"] if byte == b"!" else s["max_qual"]) == byte[0], (kind, name, p, r, s)


def test_a_four_newline_lane_at_a_known_chunk(ctx):
    """Two records of ten bytes at the start of lane 20, slice 0, of a chunk of otherwise ordinary reads: eight newlines in
    that lane's 32 bytes.  The chunk's class tests are the redo kernel's: a bad base and quality bytes outside the boot
    range in the ordinary records in front of and behind the two, in the same chunk, must be found all the same."""
    recs0 = base_records(150)
    k = len(recs0) // 2
    tiny = [[b"a", b"A", b"I"], [b"b", b"C", b"H"]]
    recs = recs0[:k] + tiny + recs0[k:]
    recs, pos = place(recs, k, 0, 20 * LANE)
    img = join(recs)
    lanes = lane_newlines(img)
    assert lanes[pos // LANE] == 8 and (lanes >= 4).sum() == 1
    r, _ = check(ctx, img)
    assert r["code"] == 0 and r["n_records"] == len(recs)
    c0 = pos // CHUNK * CHUNK
    a, nl, ltype, _, _ = byte_tables(img)
    for lo, hi in ((c0, pos), (pos + 20, c0 + CHUNK)):
        for line, byte in ((1, b"X"), (3, b"!"), (3, b"~")):
            hits = lo + np.flatnonzero((ltype[lo:hi] == line) & ~nl[lo:hi])
            assert len(hits), (lo, hi, line)
            for p in (int(hits[0]), int(hits[-1])):
                bad = img[:p] + byte + img[p + 1:]
                r, s = check(ctx, bad)
                if line == 1:
                    assert r["code"] == 6 and r["record"] == record_of(img, p), (p, r)
                else:
                    assert r["code"] == 0 and (s["min_qual"] if byte == b"!" else s["max_qual"]) == byte[0], (p, r, s)


# ---- a wrong speculation --------------------------------------------------------------------------------------------
def test_wrong_speculation_stays_correct(ctx):
    """"+" as a one-character quality line.  Everywhere: one-base reads whose sequence line is the first one-byte line of
    most chunks.  And placed: one such record whose four newlines are split 1 + 3 over two lanes, so that its chunk keeps its
    class tests - under a type that the rank then proves wrong."""
    def name_len(rng, i):
        return int(rng.integers(90, 130))
    recs = records(12, 19000, 2, 40, name_len)
    for i in range(0, len(recs), 3):
        recs[i][1], recs[i][2] = recs[i][1][:1], b"+"
    img = join(recs)
    r, _ = check(ctx, img)
    assert r["code"] == 0
    k = 2 * len(recs) // 3 // 3 * 3 + 1
    p = img.index(b"@" + recs[k][0] + b"\n") + len(recs[k][0]) + 2
    r, _ = check(ctx, img[:p] + b"#" + img[p + 1:])
    assert r["code"] == 6 and r["record"] == k

    recs0 = base_records(150)
    k = len(recs0) // 2
    one = [b"one", b"A", b"+"]
    recs, pos = place(recs0[:k] + [one] + recs0[k:], k, 5, LANE - 1)  # the 'A' is lane 0's last byte
    img = join(recs)
    lanes = lane_newlines(img)
    assert img[pos:pos + 1] == b"A" and lanes[pos // LANE] == 2 and lanes[pos // LANE + 1] == 3 and lanes.max() == 3
    r, s = check(ctx, img)
    assert r["code"] == 0 and s["max_qual"] == 73 and s["min_qual"] == 35
    for d, byte, code in ((0, b"X", 6), (4, b"!", 0), (4, b"~", 0)):
        bad = img[:pos + d] + byte + img[pos + d + 1:]
        r, s = check(ctx, bad)
        assert r["code"] == code and (code == 0 or r["record"] == k), (d, r)
        if code == 0:
            assert (s["min_qual"] if byte == b"!" else s["max_qual"]) == byte[0], (d, r, s)


# ---- the name modes on very short reads -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["digests", "records"])
def test_name_modes_on_very_short_reads(ctx, mode):
    """`found` / t0 still feed the capture of a chunk that skips its class tests; its records are not trusted (the chunk
    is kInfoUnknown) and the name kernels take those names from the line index: entries, accounted bytes and a
    duplicate as through the line index alone and behind the two-pass path."""
    recs = short_records("1_28")
    n = len(recs)
    clean = join(recs)
    dup = join(recs[:n - 9] + [recs[n // 3]] + recs[n - 9:])
    flags = A.VALIDATE_NAME_DIGESTS if mode == "digests" else A.VALIDATE_NAMES
    for img in (clean, dup):
        st = A.probe_first_record(img, False)
        got = []
        for fl in (flags, 0, A.VALIDATE_TWO_PASS):
            acc = ctx.accumulator()
            r = ctx.validate(img, acc, st, flags=fl)
            assert r["path"] == (2 if fl == A.VALIDATE_TWO_PASS else 3), r
            idx = ctx.name_index(n + 16)
            if mode == "digests":
                idx.expect_lookups(False)
            ir = idx.insert_unique(st)
            s = acc.read()
            got.append((r["code"], r["record"], r["n_records"], s["num_rds"], ir["code"], ir["record"], ir["n_entries"], ir["index_mem"]))
            idx.close()
            acc.close()
        assert got[0] == got[1] == got[2], got
        if img is clean:
            assert got[0][0] == 0 and got[0][4] == 0 and got[0][6] == n
        else:
            assert got[0][4] != 0
