"""The mark packs of the streaming pass on the matrix pipe (pack_marks32_wave, fqg_mark_pack.h, in stream_pass1_body): one
MFMA packs 16 bytes of all 64 lanes, so what must hold on the device is the LANE layout of the instruction - every lane gets
the marks of its own bytes, none of lane j + 16, j + 32 or j + 48 and none of its neighbours in a group of four - and the
byte order inside a lane.  tests/test_mark_pack_wave.py checks the host restatement of that layout; here the kernel runs.

  not-ACGTN pack  one bad base at chunk offset 2048 k + 32 L + p: both slices k, all 64 lanes L, p in P
  in-range pack   one quality byte below the boot window's minimum at the same offsets
  newline pack    reads of 25 - 60 bases: a newline at every one of the 4096 offsets of a chunk
  name modes, the parted pass
  beside line workers  the same findings in every lane, in the second part of an image of 17 MiB cut into two parts

Where the packs run: the launches of a parted pass that also carry line workers (k_stream_pass1_lines) pack with the MFMAs,
the launch of its own (k_stream_pass1: every image of 2 MiB, and the first part) with v_dot4.  The tests on 2 MiB images
hold whichever form that kernel has; the tests "beside line workers" are the ones that run the MFMAs today.

Images are 2 - 4 MiB (the parted one apart) and are judged as tests/test_gpu_stream_pack_stage.py judges: the result fields and
the accumulator of the streaming pass equal those of the two-pass path (FQG_VALIDATE_TWO_PASS), and both give what the
oracle (`fastq_info -r`) gives."""
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import loader as orc

pytestmark = pytest.mark.gpu
A = fq.abi
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK, SLICE, LANE, WAVE = 4096, 2048, 32, 64
BOOT = 64 << 10
P = (0, 3, 4, 7, 8, 15, 16, 31)  # the ends of the words, of the two dot products of a result and of the two MFMAs
KEYS = ("code", "record", "aux0", "aux1", "n_records", "n_lines", "consumed", "tail_lines", "stopped")
L150 = 150


@pytest.fixture(scope="module")
def ctx():
    c = fq.Context(0)
    yield c
    c.close()


def run(ctx, img, flags=0):
    """img: bytes, or a bytearray that the caller changes in place from image to image"""
    st = A.probe_first_record(bytes(img[:100000]), False)
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


def check(ctx, img):
    """streaming pass == two-pass path == oracle; returns the streaming result, statistics, median and histogram"""
    assert (2 << 20) <= len(img) <= (4 << 20), len(img)
    r, s, med, h = run(ctx, img)
    assert r["path"] == 3, r
    r2, s2, med2, h2 = run(ctx, img, A.VALIDATE_TWO_PASS)
    assert r2["path"] == 2, r2
    assert {k: r[k] for k in KEYS} == {k: r2[k] for k in KEYS}, (r, r2)
    if r["code"] == 0:
        assert s == s2 and med == med2 and h == h2, (s, s2, med, med2)
    against_oracle(r, s, med, img)
    return r, s, med, h


def synth(seed, n, lo, hi):
    """n records with reads of lo..hi bases, qualities '#'..'I', names padded by 0..23 bytes -> (image, read lengths)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    pads = rng.integers(0, 24, n)
    total = int(lens.sum())
    seq = BASES[rng.integers(0, 4, total)].tobytes()
    qual = (rng.integers(2, 41, total) + 33).astype(np.uint8).tobytes()
    out, at = [], 0
    for i in range(n):
        L = int(lens[i])
        out.append(b"@R%d" % i + b"_" * int(pads[i]) + b"\n" + seq[at:at + L] + b"\n+\n" + qual[at:at + L] + b"\n")
        at += L
    return b"".join(out), lens


class Base:
    """ordinary reads of 150 bases under names of varying length (2.2 MiB), with the line type of every byte: a chunk
    offset is then a matter of choosing the chunk.  first: findings go behind this position."""

    def __init__(self, seed=260, size=9 << 18, first=BOOT):
        self.first = first
        self.img, _ = synth(seed, size // (2 * L150 + 40), L150, L150)
        a = np.frombuffer(self.img, dtype=np.uint8)
        nl = np.flatnonzero(a == 10)
        self.line = np.searchsorted(nl, np.arange(len(a)), side="left")  # the line a byte belongs to (a '\n' to its own)
        self.is_nl = a == 10
        self.n_chunks = len(a) // CHUNK
        self.clean = None  # what the image gives as it is (filled by the first test that needs it)
        self.buf = None    # the image as a buffer to change in place (check_parted)

    def spot(self, off, line_type):
        """the position with chunk offset `off` nearest the middle of the image that lies on a line of that type, not at
        its first or last byte; in a whole chunk beyond the boot window and in front of the image's last two chunks"""
        chunks = np.arange(self.first // CHUNK + 1, self.n_chunks - 2)
        pos = chunks * CHUNK + off
        ok = ((self.line[pos] & 3) == line_type) & (self.line[pos - 1] == self.line[pos]) & ~self.is_nl[pos] & ~self.is_nl[pos + 1]
        pos = pos[ok]
        assert len(pos), (off, line_type)
        return int(pos[np.argmin(np.abs(pos - (self.first + len(self.img)) // 2))])

    def with_byte(self, pos, byte):
        assert pos > self.first
        return self.img[:pos] + byte + self.img[pos + 1:]


@pytest.fixture(scope="module")
def base(ctx):
    b = Base()
    b.clean = check(ctx, b.img)
    assert b.clean[0]["code"] == 0 and (b.clean[1]["min_qual"], b.clean[1]["max_qual"]) == (35, 73), b.clean[:2]
    return b


# ---- the not-ACGTN pack ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("k", [0, 1])
def test_bad_base_in_every_lane(ctx, base, k, p):
    for lane in range(WAVE):
        pos = base.spot(k * SLICE + lane * LANE + p, 1)
        r, _, _, _ = check(ctx, base.with_byte(pos, b"X"))  # (record and position against the oracle's: check())
        assert r["code"] == 6 and r["record"] == int(base.line[pos]) // 4, ((k, lane, p), pos, r)


# ---- the in-range pack ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("k", [0, 1])
def test_low_quality_in_every_lane(ctx, base, k, p):
    r0, s0, med0, h0 = base.clean
    for lane in range(WAVE):
        pos = base.spot(k * SLICE + lane * LANE + p, 3)
        r, s, med, h = check(ctx, base.with_byte(pos, b"!"))
        where = ((k, lane, p), pos)
        assert {key: r[key] for key in KEYS} == {key: r0[key] for key in KEYS}, (where, r, r0)
        assert s["min_qual"] == ord("!"), (where, s)
        assert {key: v for key, v in s.items() if key != "min_qual"} == {key: v for key, v in s0.items() if key != "min_qual"}, (where, s, s0)
        assert med == med0 and h == h0, where


# ---- the newline pack -----------------------------------------------------------------------------------------------
def test_newline_at_every_offset_of_a_chunk(ctx):
    """reads of 25 - 60 bases: the chunks the pack sees (whole ones in front of the image's last two) hold a newline at
    every byte position of every lane of both slices, one to three to a lane"""
    n = 24000
    img, lens = synth(261, n, 25, 60)
    a = np.frombuffer(img, dtype=np.uint8)
    whole = (len(a) // CHUNK - 2) * CHUNK
    at = np.flatnonzero(a[:whole] == 10)
    seen = np.zeros((2, WAVE, LANE), dtype=bool)
    seen[(at % CHUNK) // SLICE, (at % SLICE) // LANE, at % LANE] = True
    assert seen.all()
    per_lane = (a[:whole] == 10).reshape(-1, LANE).sum(axis=1)
    assert set(np.unique(per_lane)) == {0, 1, 2, 3}
    r, s, _, h = check(ctx, img)  # (record counts and the histogram against the two-pass path's: check())
    assert r["code"] == 0 and r["n_lines"] == 4 * n and r["n_records"] == n and s["num_rds"] == n
    vals, counts = np.unique(lens, return_counts=True)
    off = s["min_rl"] - int(vals[0])
    assert h == {int(v) + off: int(c) for v, c in zip(vals, counts)}
    assert s["max_rl"] == int(vals[-1]) + off


# ---- both name modes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["digests", "records"])
def test_name_modes(ctx, base, mode):
    """the name-capturing instantiations share the body: a bad base in lane 37 of slice 1, and the image as it is"""
    flags = A.VALIDATE_NAME_DIGESTS if mode == "digests" else A.VALIDATE_NAMES
    pos = base.spot(SLICE + 37 * LANE + 8, 1)
    n = base.clean[0]["n_records"]
    for img, code, record in ((base.with_byte(pos, b"X"), 6, int(base.line[pos]) // 4), (base.img, 0, None)):
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
        assert got[0][0] == code, got
        if code:
            assert got[0][1] == record, got
        else:
            assert got[0][4] == 0 and got[0][6] == n, got


# ---- the parted pass ------------------------------------------------------------------------------------------------
def test_parted_pass():
    """pass 1 beside the line workers (k_stream_pass1_lines shares the body): 57 MB cut into three parts at 16 MiB spans, a
    bad base in lane 21 of slice 0 of a chunk of the last part and a low quality byte in the second - as through one launch
    and as the oracle's, first with the quality byte alone"""
    n = 165_000
    rng = np.random.default_rng(262)
    seq = BASES[rng.integers(0, 4, n * L150)]
    qual = (rng.integers(2, 41, n * L150) + 33).astype(np.uint8)
    recs = [b"@SYN:1:FC:%d:%d 1:N:0:ACGT\n" % (i % 97, i) + seq[i * L150:(i + 1) * L150].tobytes() + b"\n+\n" +
            qual[i * L150:(i + 1) * L150].tobytes() + b"\n" for i in range(n)]
    start = np.concatenate(([0], np.cumsum([len(x) for x in recs])))

    def find(k0, line, off):
        """the first record from k0 on with a byte of its sequence (line 1) or quality (line 3) at chunk offset off"""
        for k in range(k0, n):
            first = int(start[k]) + recs[k].index(b"\n") + 1 + (0 if line == 1 else L150 + 3)
            j = (off - first) % CHUNK
            if 0 < j < L150 - 1:
                return k, first - int(start[k]) + j
        raise AssertionError((k0, line, off))

    kq, jq = find(int(n * 0.5), 3, SLICE + 58 * LANE + 16)
    recs[kq] = recs[kq][:jq] + b"!" + recs[kq][jq + 1:]
    img_q = b"".join(recs)
    kb, jb = find(int(n * 0.97), 1, 21 * LANE + 7)
    recs[kb] = recs[kb][:jb] + b"X" + recs[kb][jb + 1:]
    img_b = b"".join(recs)
    assert 3 * (16 << 20) < len(img_b) < (60 << 20) and img_q[int(start[kq]) + jq] == ord("!") and img_b[int(start[kb]) + jb] == ord("X")
    os.environ["FQGPU_STREAM_PARTS_MIN_SPANS"] = "3"
    try:
        with fq.Context(0) as ctx:
            for img in (img_q, img_b):
                got = []
                for parts in (1, 3):
                    os.environ["FQGPU_STREAM_PARTS"] = str(parts)
                    r, s, med, _ = run(ctx, img)
                    assert r["path"] == 3, r
                    got.append((r, s))
                against_oracle(r, s, med, img)
                assert {key: got[0][0][key] for key in KEYS} == {key: got[1][0][key] for key in KEYS}, got
                if img is img_q:
                    assert got[1][0]["code"] == 0 and got[0][1] == got[1][1] and got[1][1]["min_qual"] == ord("!"), got
                else:
                    assert got[1][0]["code"] == 6 and got[1][0]["record"] == kb, got
    finally:
        os.environ.pop("FQGPU_STREAM_PARTS_MIN_SPANS", None)
        os.environ.pop("FQGPU_STREAM_PARTS", None)


# ---- beside line workers: the packs on the matrix pipe ----------------------------------------------------------------
SPAN = 16 << 20  # parts are cut at spans of 4096 chunks


@pytest.fixture(scope="module")
def parted():
    """a context whose passes are cut into parts from two spans on, and an image of 17.6 MiB: the first 16 MiB pass through
    k_stream_pass1, the rest through k_stream_pass1_lines beside the line workers of the first part.  Judged once against
    the oracle as it is; the images with a finding are judged against the two-pass path and the finding's known place
    (the oracle reads 17 MiB in a tenth of a second: once per test, not per lane)."""
    os.environ["FQGPU_STREAM_PARTS_MIN_SPANS"] = "1"
    os.environ["FQGPU_STREAM_PARTS"] = "2"
    try:
        with fq.Context(0) as c:
            b = Base(seed=263, size=SPAN + (5 << 19), first=SPAN + BOOT)
            assert SPAN + (1 << 20) < len(b.img) < SPAN + (3 << 20)
            c.profile(True)
            c.profile_reset()
            r, s, med, h = run(c, b.img)
            ran = {k: v[0] for k, v in c.profile_read().items()}
            c.profile(False)
            assert r["path"] == 3 and ran.get("k_stream_pass1_lines", 0) == 1 and ran.get("k_stream_pass1", 0) == 1, (r, ran)
            against_oracle(r, s, med, b.img)
            b.clean = (r, s, med, h)
            yield c, b
    finally:
        os.environ.pop("FQGPU_STREAM_PARTS_MIN_SPANS", None)
        os.environ.pop("FQGPU_STREAM_PARTS", None)


def check_parted(c, b, pos, byte, with_oracle):
    """the image of b with `byte` at pos (written into one buffer and taken back: 17 MiB are not copied per lane)"""
    if b.buf is None:
        b.buf = bytearray(b.img)
    assert pos > b.first
    img, old = b.buf, b.buf[pos]
    img[pos] = byte[0]
    try:
        return check_parted_image(c, img, with_oracle)
    finally:
        img[pos] = old


def check_parted_image(c, img, with_oracle):
    r, s, med, h = run(c, img)
    assert r["path"] == 3, r
    r2, s2, med2, h2 = run(c, img, A.VALIDATE_TWO_PASS)
    assert r2["path"] == 2, r2
    assert {k: r[k] for k in KEYS} == {k: r2[k] for k in KEYS}, (r, r2)
    if r["code"] == 0:
        assert s == s2 and med == med2 and h == h2, (s, s2, med, med2)
    if with_oracle:
        against_oracle(r, s, med, bytes(img))
    return r, s, med, h


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("k", [0, 1])
def test_bad_base_in_every_lane_beside_line_workers(parted, k, p):
    c, b = parted
    for lane in range(WAVE):
        pos = b.spot(k * SLICE + lane * LANE + p, 1)
        r, _, _, _ = check_parted(c, b, pos, b"X", with_oracle=lane == 5 * p % WAVE)
        assert r["code"] == 6 and r["record"] == int(b.line[pos]) // 4, ((k, lane, p), pos, r)


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("k", [0, 1])
def test_low_quality_in_every_lane_beside_line_workers(parted, k, p):
    c, b = parted
    r0, s0, med0, h0 = b.clean
    for lane in range(WAVE):
        pos = b.spot(k * SLICE + lane * LANE + p, 3)
        r, s, med, h = check_parted(c, b, pos, b"!", with_oracle=lane == 5 * p % WAVE)
        where = ((k, lane, p), pos)
        assert {key: r[key] for key in KEYS} == {key: r0[key] for key in KEYS}, (where, r, r0)
        assert s["min_qual"] == ord("!"), (where, s)
        assert {key: v for key, v in s.items() if key != "min_qual"} == {key: v for key, v in s0.items() if key != "min_qual"}, (where, s, s0)
        assert med == med0 and h == h0, where
