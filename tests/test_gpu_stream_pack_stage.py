"""The glue of the streaming pass around its class tests (stream_pass1_body / stage_chunk, fqg_stream_kernels.hip): the
32-bit mark pack (fqg_mark_pack.h), the slot loop and the entry loop of the staging, the byte behind the chunk that the
entry loop finds in the LDS copy, and the wavefront scan whose adds carry the DPP modifier.

  pack order     a finding at each of the 32 byte positions of a lane, in both slices
  newline offsets  reads of 25 - 60 bases: newlines at all 32 positions, one to three to a lane
  tail byte      a chunk that ends in '\\n' in front of '@', '+' and other bytes; "\\n+\\n" across the chunk's end
  stage capacity exactly 256 newlines in a chunk (the slots are full), and 257 (the image takes the two-pass path)
  name modes, the parted pass

Every image but the parted one is 2 - 4 MiB and is judged as tests/test_gpu_stream_typemasks.py judges: the result fields
and the accumulator of the streaming pass equal those of the two-pass path (FQG_VALIDATE_TWO_PASS), and both give what the
oracle (`fastq_info -r`) gives."""
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import loader as orc

pytestmark = pytest.mark.gpu
A = fq.abi
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK, SLICE, LANE = 4096, 2048, 32
STAGE_CAP = 256
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
        return r, acc.read(), acc.median(), acc.hist()
    finally:
        acc.close()


def against_oracle(r, s, med, img):
    want = orc.fastq_info(img, "t.fastq", flags=orc.FLAG_R)
    first = want["first"]
    assert r["code"] == first["code"], (r, first)
    if r["code"]:
        assert r["record"] == first["record"] and r["aux0"] == first["aux0"], (r, first)
    else:
        w = want["summary"]
        assert (s["num_rds"], s["min_rl"], s["max_rl"], s["min_qual"], s["max_qual"], med) == (
            w["num_reads"], w["min_rl"], w["max_rl"], w["min_qual"], w["max_qual"], w["median_rl"]), (s, med, w)


def check(ctx, img, want_path=3):
    """streaming pass == two-pass path == oracle; returns the streaming result, statistics and histogram"""
    assert (2 << 20) <= len(img) <= (4 << 20), len(img)
    r, s, med, h = run(ctx, img)
    assert r["path"] == want_path, r
    r2, s2, med2, h2 = run(ctx, img, A.VALIDATE_TWO_PASS)
    assert r2["path"] == 2, r2
    assert {k: r[k] for k in KEYS} == {k: r2[k] for k in KEYS}, (r, r2)
    if r["code"] == 0:
        assert s == s2 and med == med2 and h == h2, (s, s2, med, med2)
    against_oracle(r, s, med, img)
    return r, s, h


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


def chunk_newlines(img):
    a = np.frombuffer(img, dtype=np.uint8)[:len(img) // CHUNK * CHUNK]
    return (a == 10).reshape(-1, CHUNK).sum(axis=1)


def lane_newlines(img):
    a = np.frombuffer(img, dtype=np.uint8)[:len(img) // CHUNK * CHUNK]
    return (a == 10).reshape(-1, LANE).sum(axis=1)


L150 = 150
_BASE = []


def base_records():
    """ordinary reads of 150 bases, names of varying length: 2.2 MiB"""
    if not _BASE:
        _BASE.append(records(250, (9 << 18) // (2 * L150 + 40), L150, L150, name_len=lambda rng, i: int(rng.integers(0, 24))))
    return _BASE[0]


def names_agree(ctx, img, mode, n):
    """the capture of the pass (records or digests) feeds the name index as the line index alone and the two-pass path do"""
    flags = A.VALIDATE_NAME_DIGESTS if mode == "digests" else A.VALIDATE_NAMES
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
    return got[0]


# ---- pack order -----------------------------------------------------------------------------------------------------
def pack_order_image(what, sl, bit):
    """one byte of record k - in the middle of its sequence or quality line - at byte `bit` of a lane (0, 31 or 63 in
    turn) of slice `sl` of a chunk in the middle of the image"""
    recs0 = base_records()
    k = len(recs0) // 2 + 7
    lane = (0, 31, 63)[bit % 3]
    line = 1 if what == "bad_base" else 2
    name = recs0[k][0]
    delta = (len(name) + 2 if line == 1 else len(name) + 2 + L150 + 3) + L150 // 2
    recs, pos = place(recs0, k, delta, sl * SLICE + lane * LANE + bit)
    byte = {"bad_base": b"X", "qual_below": b"!", "qual_above": b"~"}[what]
    field = bytearray(recs[k][line])
    field[L150 // 2] = byte[0]
    recs[k][line] = bytes(field)
    img = join(recs)
    assert img[pos:pos + 1] == byte and img[pos - 1] != 10 and img[pos + 1] != 10
    assert len(img) // 3 < pos < 2 * len(img) // 3
    return img, k, len(recs)


@pytest.mark.parametrize("what", ["bad_base", "qual_below", "qual_above"])
@pytest.mark.parametrize("sl", [0, 1])
def test_pack_order(ctx, sl, what):
    for bit in range(LANE):
        img, k, _ = pack_order_image(what, sl, bit)
        r, s, _ = check(ctx, img)
        where = (what, sl, bit)
        if what == "bad_base":
            assert r["code"] == 6 and r["record"] == k, (where, r)
        elif what == "qual_below":  # (the boot range of these images is '#'..'I')
            assert r["code"] == 0 and s["min_qual"] == ord("!") and s["max_qual"] == 73, (where, r, s)
        else:
            assert r["code"] == 0 and s["min_qual"] == 35 and s["max_qual"] == ord("~"), (where, r, s)


# ---- newline offsets ------------------------------------------------------------------------------------------------
def test_newline_offsets(ctx):
    """reads of 25 - 60 bases under names of varying length: newlines at every position of a lane, lanes with one, two and
    three of them (never four: that needs reads under 25 bases), every chunk inside the staging area"""
    recs = records(251, 24000, 25, 60, name_len=lambda rng, i: int(rng.integers(0, 24)))
    img = join(recs)
    a = np.frombuffer(img, dtype=np.uint8)
    at = np.flatnonzero(a == 10)
    assert len(np.unique(at % LANE)) == LANE
    lanes = lane_newlines(img)
    assert set(np.unique(lanes)) == {0, 1, 2, 3} and chunk_newlines(img).max() <= STAGE_CAP
    r, s, h = check(ctx, img)
    assert r["code"] == 0 and r["n_lines"] == 4 * len(recs) and r["n_records"] == len(recs)
    # the histogram (equal to the two-pass path's, check()): as many reads of every length as the image holds, keyed as
    # the statistics count a length
    lens, counts = np.unique([len(x[1]) for x in recs], return_counts=True)
    off = s["min_rl"] - int(lens[0])
    assert h == {int(k) + off: int(v) for k, v in zip(lens, counts)}
    assert (s["num_rds"], s["max_rl"]) == (len(recs), int(lens[-1]) + off)


# ---- the byte behind the chunk --------------------------------------------------------------------------------------
# (which byte of record k stands where in its chunk, the byte it is replaced with or None, the code of the finding)
TAILS = {
    "at": ("at", 0, None),                 # the chunk ends in '\n', the next begins with '@'
    "plus": ("plus", 0, None),             # ... with '+'
    "seq": ("seq", 0, None),               # ... with another byte: a base
    "qual": ("qual", 0, None),             # ... a quality byte
    "not_at": ("at", 0, b"X"),             # ... a header without its '@'
    "not_plus": ("plus", 0, b"-"),         # ... a "+" line that is none
    "lookahead": ("plus", CHUNK - 1, None),       # "\n+" ends the chunk, the '\n' behind it begins the next
    "lookahead_slice": ("plus", SLICE - 1, None),  # the same across the slices
    "lookahead_not_plus": ("plus", CHUNK - 1, b"-"),
}


def tail_image(case):
    which, want, repl = TAILS[case]
    recs0 = base_records()
    k = len(recs0) // 2 + 3
    name = recs0[k][0]
    delta = {"at": 0, "seq": len(name) + 2, "plus": len(name) + L150 + 3, "qual": len(name) + L150 + 5}[which]
    recs, pos = place(recs0, k, delta, want)
    img = join(recs)
    assert img[pos - 1] == 10 and img[pos:pos + 1] == {"at": b"@", "plus": b"+"}.get(which, img[pos:pos + 1])
    if which == "plus":
        assert img[pos + 1] == 10
    if repl:
        img = img[:pos] + repl + img[pos + 1:]
    return img, k, len(recs)


@pytest.mark.parametrize("case", list(TAILS))
def test_tail_byte(ctx, case):
    img, k, n = tail_image(case)
    r, _, _ = check(ctx, img)
    if TAILS[case][2]:
        assert r["code"] != 0 and r["record"] == k, r
    else:
        assert r["code"] == 0 and r["n_records"] == n, r


# ---- the staging area, full and one over ----------------------------------------------------------------------------
def dense_chunk_image(n_newlines, bad_base=False):
    """a run of ten-byte records at the start of a chunk in the middle of ordinary reads, the name of the run's last record
    padded until the chunk holds exactly n_newlines newlines"""
    recs0 = base_records()
    k = len(recs0) // 2
    follow = join(recs0[k:k + 20])
    tiny = None
    for T in range(45, 70):
        for e in range(0, 400):
            cand = [[b"a", b"A", b"I"]] * (T - 1) + [[b"a" + b"x" * e, b"A", b"I"]]
            if (join(cand) + follow)[:CHUNK].count(b"\n") == n_newlines:
                tiny = cand
                break
        if tiny:
            break
    assert tiny
    recs, pos = place(recs0[:k] + tiny + recs0[k:], k, 0, 0)
    if bad_base:  # in the first ordinary record behind the run: it begins in the dense chunk
        j = k + len(tiny)
        recs[j][1] = recs[j][1][:5] + b"X" + recs[j][1][6:]
    img = join(recs)
    per = chunk_newlines(img)
    assert per[pos // CHUNK] == n_newlines and np.delete(per, pos // CHUNK).max() < 100
    return img, len(recs), k + len(tiny)


@pytest.mark.parametrize("bad_base", [False, True], ids=["clean", "bad_base"])
@pytest.mark.parametrize("n_newlines", [STAGE_CAP, STAGE_CAP + 1])
def test_stage_capacity(ctx, n_newlines, bad_base):
    img, n, j = dense_chunk_image(n_newlines, bad_base)
    r, s, _ = check(ctx, img, want_path=3 if n_newlines <= STAGE_CAP else 2)
    if bad_base:
        assert r["code"] == 6 and r["record"] == j, r
    else:
        assert r["code"] == 0 and r["n_records"] == n and s["num_rds"] == n and s["max_rl"] - s["min_rl"] == L150 - 1, (r, s)


# ---- both name modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["digests", "records"])
def test_name_modes(ctx, mode):
    img, _, n = tail_image("at")
    got = names_agree(ctx, img, mode, n)
    assert got[0] == 0 and got[4] == 0 and got[6] == n, got
    img, k, n = pack_order_image("bad_base", 1, 13)
    got = names_agree(ctx, img, mode, n)
    assert got[0] == 6 and got[1] == k, got


# ---- the parted pass ------------------------------------------------------------------------------------------------
def test_parted_pass_with_a_bad_base_in_the_last_part():
    """pass 1 beside the line workers (k_stream_pass1_lines shares the body): 57 MB cut into three parts at 16 MiB spans,
    a bad base in the last one - the finding and everything else as through one launch and as the oracle's"""
    n = 165_000
    rng = np.random.default_rng(252)
    seq = BASES[rng.integers(0, 4, n * L150)]
    qual = (rng.integers(2, 41, n * L150) + 33).astype(np.uint8)
    recs = [b"@SYN:1:FC:%d:%d 1:N:0:ACGT\n" % (i % 97, i) + seq[i * L150:(i + 1) * L150].tobytes() + b"\n+\n" +
            qual[i * L150:(i + 1) * L150].tobytes() + b"\n" for i in range(n)]
    k = int(n * 0.97)
    p = recs[k].index(b"\n")
    recs[k] = recs[k][:p + 78] + b"X" + recs[k][p + 79:]
    img = b"".join(recs)
    assert 3 * (16 << 20) < len(img) < (60 << 20)
    os.environ["FQGPU_STREAM_PARTS_MIN_SPANS"] = "3"
    try:
        with fq.Context(0) as ctx:
            got = []
            for parts in (1, 3):
                os.environ["FQGPU_STREAM_PARTS"] = str(parts)
                r, s, med, _ = run(ctx, img)
                assert r["path"] == 3, r
                got.append(r)
                against_oracle(r, s, med, img)
            assert {key: got[0][key] for key in KEYS} == {key: got[1][key] for key in KEYS}, got
            assert got[1]["code"] == 6 and got[1]["record"] == k, got
    finally:
        os.environ.pop("FQGPU_STREAM_PARTS_MIN_SPANS", None)
        os.environ.pop("FQGPU_STREAM_PARTS", None)
