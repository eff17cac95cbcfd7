"""The steps of the line kernel without a search (k_stream_lines_fast and the line workers of k_stream_pass1_lines,
fqg_stream_kernels.hip) at their own edges.  A step is 128 records - two groups of 64, a record a lane - whose 513 staged
entries the wavefront fetches in slots of 64, one per covering chunk; steps it does not take (step 0, the last records,
ranks spread over more than 16 chunks, a chunk with more than 64 newlines, a window that misses) are marked for the
general kernel.  Every case is checked against the oracle: the finding and its record, or the record count and the six
statistics with the median.  Images are 2 - 3 MiB, just over the 1 MiB threshold of the streaming path, but for the one
that needs two parts."""
import functools
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import loader as orc

pytestmark = pytest.mark.gpu
A = fq.abi
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNK = 4096
STEP = 128  # records of a step
NAME = b"SYN:1:FC:%d:%d 1:N:0:ACGT"


def record(rng, i, L, name=NAME):
    seq = BASES[rng.integers(0, 4, L)].tobytes()
    qual = (rng.integers(2, 41, L) + 33).astype(np.uint8).tobytes()
    return b"@" + (name % (i % 97, i)) + b"\n" + seq + b"\n+\n" + qual + b"\n"


def records(seed, n, lo, hi, name=NAME, blocks=0):
    """n records of lo .. hi bases, a length per record - or, blocks > 0, in blocks of that many records of ONE length:
    every tenth block of lo bases, the others of hi"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    if blocks:
        lens = np.where((np.arange(n) // blocks) % 10 == 0, lo, hi)
    return [record(rng, i, int(lens[i]), name) for i in range(n)]


@functools.lru_cache(maxsize=None)
def base150(n=7333):
    """2.5 MiB of 150-base reads, 7333 = 57 * 128 + 37 records: 57 full steps and an incomplete one (shared; nobody
    changes the list)"""
    return tuple(records(3, n, 150, 150))


def validate(img, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        with fq.Context(0) as ctx:
            st = A.probe_first_record(img, False)
            acc = ctx.accumulator()
            r = ctx.validate(img, acc, st)
            s, med = acc.read(), acc.median()
            acc.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return r, s, med


def against_oracle(got, img, finding=None):
    """finding: None = a clean image, else the record the finding is expected in"""
    r, s, med = got
    want = orc.fastq_info(img, "p.fastq", flags=orc.FLAG_R)
    assert r["path"] == 3, r
    assert r["code"] == want["first"]["code"], (r, want["first"])
    assert (r["code"] != 0) == (finding is not None), (r, finding)
    if r["code"]:
        assert r["record"] == want["first"]["record"] == finding and r["aux0"] == want["first"]["aux0"], (r, want["first"], finding)
    else:
        w = want["summary"]
        assert (s["num_rds"], s["min_rl"], s["max_rl"], s["min_qual"], s["max_qual"], med) == (
            w["num_reads"], w["min_rl"], w["max_rl"], w["min_qual"], w["max_qual"], w["median_rl"]), (s, med, w)


def density(img):
    return img.count(b"\n") / -(-len(img) // CHUNK)


def damaged(r, what):
    """one record with one finding"""
    head, seq, plus, qual = r[:-1].split(b"\n")
    if what == "no_at":
        head = b"X" + head[1:]
    elif what == "plus_x":
        plus = b"+x"
    elif what == "seq_longer":
        qual = qual[:-1]
    elif what == "seq_shorter":
        seq = seq[:-1]
    else:
        assert what == "empty_seq"
        seq, qual = b"", b""
    return head + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n"


# ---- density bounds ----
# name: lengths, records, blocks of one length, the name that sets the bytes around a read, the newlines per chunk the
# image must have.  The bound of 60 newlines in an average chunk is the host's (above it the general kernel runs alone),
# the 64 of one chunk the kernel's own (a step with such a chunk is refused: `many`).
NAME16, NAME19 = NAME + b"ACGT" * 4, NAME + b"ACGT" * 4 + b"ACG"
DENSITY = {
    "150bp": (150, 150, 7333, 0, NAME, (46.0, 50.0)),
    # 100 - 112 bases behind the short name: 64 - 70 newlines a chunk, nearly every chunk beyond 64
    "100_112bp": (100, 112, 10500, 0, NAME, (64.0, 70.0)),
    # ... behind a longer name: chunks of 60 - 66 newlines, none beyond 64, the image between the two bounds
    "100_112bp_60_to_64": (100, 112, 10000, 0, NAME16, (60.5, 64.0)),
    # ... and in blocks of 400 records of 100 and of 112 bases behind a name three bytes longer: the image just below 60
    # a chunk - the kernel without a search runs -, the blocks of 100 bases in chunks of 65 and 66 - those steps are refused
    "100_112bp_below_60": (100, 112, 10000, 400, NAME19, (58.0, 60.0)),
    # 225 - 245 bases: 31 - 34 newlines a chunk, the 513 ranks of a step in 16 chunks (taken) or 17 (refused)
    "225_245bp": (225, 245, 5200, 0, NAME, (32.0, 33.5)),
}


@pytest.mark.parametrize("shape", list(DENSITY))
def test_density_bounds(shape):
    lo, hi, n, blocks, name, (dlo, dhi) = DENSITY[shape]
    img = b"".join(records(11, n, lo, hi, name, blocks))
    assert 2 << 20 <= len(img) <= 3 << 20, len(img)
    d = density(img)
    per = np.bincount(np.flatnonzero(np.frombuffer(img, np.uint8) == 10) // CHUNK)
    print(shape, "newlines per chunk:", round(d, 2), "chunks beyond 64:", int((per > 64).sum()), "of", len(per))
    assert dlo < d < dhi, d
    if shape == "100_112bp":
        assert (per > 64).sum() > len(per) // 2
    if shape == "100_112bp_60_to_64":
        assert (per > 64).sum() == 0
    if shape == "100_112bp_below_60":  # both kinds of chunk, many of each
        assert (per > 64).sum() > 20 and (per <= 60).sum() > 200, np.bincount(per)
    if shape == "225_245bp":  # steps of 16 and of 17 covering chunks
        nl = np.flatnonzero(np.frombuffer(img, np.uint8) == 10)
        steps = range(1, n // STEP)
        cov = [int(nl[512 * s + 511] // CHUNK - nl[512 * s - 1] // CHUNK) + 1 for s in steps]
        assert cov.count(16) > 3 and cov.count(17) > 3, np.bincount(cov)
    against_oracle(validate(img), img)


# ---- drift inside a 150-base image ----
@pytest.mark.parametrize("stretch", ["30bp", "3kb"])
def test_a_stretch_of_other_reads_inside_a_150_base_image(stretch):
    """128 KiB of 30-base reads (176 newlines a chunk: the window estimated from the image's mean misses, the steps are
    marked and the general kernel does them) or of 3 kb reads (a chunk holds hardly a newline: the window estimated
    begins chunks too early) between 150-base reads"""
    recs = list(base150())
    L = 30 if stretch == "30bp" else 3000
    mid = records(17, (128 << 10) // (2 * L) + 1, L, L)
    mid = mid[:int(np.searchsorted(np.cumsum([len(r) for r in mid]), 128 << 10)) + 1]  # ends with the record that reaches 128 KiB
    assert (128 << 10) <= sum(len(r) for r in mid) < (136 << 10)
    k = 3000
    img = b"".join(recs[:k] + mid + recs[k:])
    assert len(img) <= 3 << 20
    against_oracle(validate(img), img)


# ---- findings by kind ----
@pytest.mark.parametrize("what", ["no_at", "plus_x", "seq_longer", "seq_shorter", "empty_seq"])
def test_findings_by_kind(what):
    recs = list(base150())
    k = 10 * STEP + 77  # lane 13 of the second group of step 10
    recs[k] = damaged(recs[k], what)
    img = b"".join(recs)
    against_oracle(validate(img), img, finding=k)


# ---- findings by place ----
def entry_chunks(recs, k):
    """the chunks the five staged entries of record k lie in: the newline in front of it and its four"""
    start = sum(len(r) for r in recs[:k])
    pos = [start - 1] + [start + i for i, c in enumerate(recs[k]) if c == 10]
    assert len(pos) == 5
    return sorted({p // CHUNK for p in pos})


def place(where):
    """(records, the record the finding goes to, strip the final newline) - lengths 141 .. 149 around the place, so a
    neighbour counted twice or not at all moves the statistics of the clean image"""
    recs = list(base150())
    n = len(recs)
    full = n // STEP  # steps [0, full) are complete
    strip = False
    if where == "record_0":
        k = 0
    elif where == "first_of_first_fast_step":
        k = STEP
    elif where == "last_of_first_fast_step":
        k = 2 * STEP - 1
    elif where == "entries_in_two_chunks":
        k = next(i for i in range(5 * STEP, 6 * STEP) if len(entry_chunks(recs, i)) == 2)
    elif where == "entries_in_three_chunks":
        # one read of 4.3 kb among the 150-base reads: header in one chunk, sequence end in the next, quality end in the third
        rng = np.random.default_rng(23)
        k = None
        for i in range(5 * STEP + 20, 6 * STEP - 20):
            trial = recs[:i] + [record(rng, i, 4300)] + recs[i + 1:]
            if len(entry_chunks(trial, i)) == 3:
                recs, k = trial, i
                break
        assert k is not None
    elif where == "last_of_last_full_step":
        k = full * STEP - 1
    elif where == "first_of_incomplete_step":
        k = full * STEP
    elif where == "last_record":
        k = n - 1
    else:
        assert where == "last_record_no_final_newline"
        k, strip = n - 1, True
    assert 0 < n % STEP < STEP
    rng = np.random.default_rng(29)
    for j in range(max(0, k - 4), min(n, k + 5)):
        if j != k:
            recs[j] = record(rng, j, 141 + (j - k + 4))
    return recs, k, strip


PLACES = ["record_0", "first_of_first_fast_step", "last_of_first_fast_step", "entries_in_two_chunks",
          "entries_in_three_chunks", "last_of_last_full_step", "first_of_incomplete_step", "last_record",
          "last_record_no_final_newline"]


@pytest.mark.parametrize("where", PLACES)
def test_findings_by_place(where):
    recs, k, strip = place(where)
    clean = b"".join(recs)
    clean = clean[:-1] if strip else clean
    against_oracle(validate(clean), clean)
    recs[k] = damaged(recs[k], "seq_longer")
    img = b"".join(recs)
    img = img[:-1] if strip else img
    against_oracle(validate(img), img, finding=k)


# ---- the workers inside a pass-1 launch ----
SPAN = 16 << 20


@functools.lru_cache(maxsize=1)
def two_parts():
    recs = records(31, 63500, 150, 150)
    ends = np.cumsum([len(r) for r in recs])
    assert 20 << 20 <= int(ends[-1]) < 21 << 20
    return tuple(recs), int(np.searchsorted(ends, SPAN, side="right"))  # ... and the record that holds byte 16 MiB


@pytest.mark.parametrize("where", ["clean", "last_of_part_0", "first_of_part_1"])
def test_line_workers_inside_a_pass1_launch(where):
    """20 MiB in two parts (the cut at the 16 MiB span): the line workers of part 0 ride in the launch of pass 1 of part
    1.  One launch and two parts give the same, and what the oracle gives; the finding once in the last record that
    lies in part 0 and once in the first that lies in part 1 (the record between them straddles the cut)"""
    recs, cut = two_parts()
    recs = list(recs)
    k = {"clean": None, "last_of_part_0": cut - 1, "first_of_part_1": cut + 1}[where]
    if k is not None:
        recs[k] = damaged(recs[k], "seq_longer")
    img = b"".join(recs)
    got = [validate(img, {"FQGPU_STREAM_PARTS_MIN_SPANS": "2", "FQGPU_STREAM_PARTS": str(parts)}) for parts in (1, 2)]
    keys = ("code", "record", "aux0", "aux1", "n_records", "n_lines", "consumed", "tail_lines", "stopped", "path")
    assert {x: got[0][0][x] for x in keys} == {x: got[1][0][x] for x in keys}, (got[0][0], got[1][0])
    assert got[0][1:] == got[1][1:] or k is not None, (got[0][1:], got[1][1:])
    for g in got:
        against_oracle(g, img, finding=k)
