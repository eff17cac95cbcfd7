"""Where a read length leaves the LDS histogram of the line kernels (fqg_stream_kernels.hip).  The kernel without a search
(stream_lines_fast_body: k_stream_lines_fast, and the line workers inside k_stream_pass1_lines) counts lengths below
kLinesFastHist in LDS and sends the others to the global histogram by atomics, in two places: the flush of a run of groups
with one length, and the records that differ from their group's first.  The general kernel (k_stream_lines) does the same
at kLinesHist.  The histogram index of a read is its sequence line's length with the newline: bases + 1.

  long reads among reads of 150   single reads of H - 3 .. H + 1 and of 3069 .. 3073 bases (indices H - 2 .. H + 2 and
                                  3070 .. 3074: both cut-overs, whichever way one counts), each once as the FIRST record of
                                  a group of 64 (the run flush) and once inside a group (the odd records), at most one
                                  to a step of 128 records.  In an image of 2 MiB (k_stream_lines_fast alone), and in one
                                  of 18.8 MiB cut into two parts, with the long reads in both parts: those of the first
                                  16 MiB are counted by line workers inside the fused launch.  Both name modes once.
  every read of one length        H - 2, H - 1 and H bases: the run flush alone, through the general kernel (a newline
                                  density of a line in 1.5 chunks)

Every image: the oracle (`fastq_info -r`) accepts it on the CPU before it goes to the GPU; exit status, num_rds, min_rl,
max_rl and the median equal the oracle's; the histogram equals the lengths the image was made of, and that of the two-pass
path; the one-launch pass (FQGPU_STREAM_PARTS=1) gives the same as the pass in parts."""
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import loader as orc

pytestmark = pytest.mark.gpu
A = fq.abi
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
H = 3008          # kLinesFastHist
H_GENERAL = 3072  # kLinesHist, and the size of both before
L150 = 150
STEP, GROUP = 128, 64  # records of a step of the line kernels, of a wavefront's group
SPAN = 16 << 20   # parts are cut at spans of 4096 chunks
LONG = sorted(set(range(H - 3, H + 2)) | set(range(H_GENERAL - 3, H_GENERAL + 2)))  # bases
KEYS = ("code", "record", "aux0", "aux1", "n_records", "n_lines", "consumed", "tail_lines", "stopped")


def image(seed, lens):
    """records with reads of lens[i] bases, qualities '#'..'I', names padded by 0..23 bytes -> (image, first byte of each)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens)
    pads = rng.integers(0, 24, len(lens))
    total = int(lens.sum())
    seq = BASES[rng.integers(0, 4, total)].tobytes()
    qual = (rng.integers(2, 41, total) + 33).astype(np.uint8).tobytes()
    out, at = [], 0
    for i in range(len(lens)):
        n = int(lens[i])
        out.append(b"@R%d" % i + b"_" * int(pads[i]) + b"\n" + seq[at:at + n] + b"\n+\n" + qual[at:at + n] + b"\n")
        at += n
    start = np.concatenate(([0], np.cumsum([len(x) for x in out])))
    return b"".join(out), start


def place(lens, first_step):
    """the long reads into lens, from step first_step on: each length once as the first record of the step's second group
    and, a step later, once inside the first group -> the step behind the last one used"""
    step = first_step
    for n in LONG:
        lens[step * STEP + GROUP] = n
        lens[(step + 1) * STEP + 37] = n
        step += 2
    return step


def accepted(img):
    """the oracle's verdict, on the CPU: the image is a valid file"""
    want = orc.fastq_info(img, "t.fastq", flags=orc.FLAG_R)
    assert want["exit"] == 0 and want["first"]["code"] == 0, (want["exit"], want["first"], want["stderr"][:200])
    return want


def run(ctx, img, flags=0):
    st = A.probe_first_record(bytes(img[:100000]), False)
    acc = ctx.accumulator()
    try:
        r = ctx.validate(img, acc, st, flags=flags)
        return r, acc.read(), acc.median(), acc.hist(), st
    finally:
        acc.close()


def judge(got, want, lens):
    r, s, med, h = got[:4]
    w = want["summary"]
    assert r["code"] == want["first"]["code"] == 0, (r, want["first"])
    assert (s["num_rds"], s["min_rl"], s["max_rl"], med) == (w["num_reads"], w["min_rl"], w["max_rl"], w["median_rl"]), (s, med, w)
    off = int(w["min_rl"]) - int(np.min(lens))  # the index of a read of n bases
    assert off == 1, (w, int(np.min(lens)))
    vals, counts = np.unique(lens, return_counts=True)
    assert h == {int(v) + off: int(c) for v, c in zip(vals, counts)}, sorted(h.items())[-12:]


def passes(ctx, img, want, lens, parts):
    """the pass as the environment cuts it (`parts` launches of pass 1), the one-launch pass, the two-pass path"""
    ctx.profile(True)
    ctx.profile_reset()
    first = run(ctx, img)
    ran = {k: v[0] for k, v in ctx.profile_read().items()}
    ctx.profile(False)
    assert first[0]["path"] == 3, first[0]
    assert ran.get("k_stream_pass1", 0) == 1 and ran.get("k_stream_pass1_lines", 0) == parts - 1, ran
    judge(first, want, lens)
    os.environ["FQGPU_STREAM_PARTS"] = "1"
    try:
        one = run(ctx, img)
    finally:
        os.environ["FQGPU_STREAM_PARTS"] = "2"
    two = run(ctx, img, A.VALIDATE_TWO_PASS)
    assert one[0]["path"] == 3 and two[0]["path"] == 2, (one[0], two[0])
    for other in (one, two):
        assert {k: other[0][k] for k in KEYS} == {k: first[0][k] for k in KEYS}, (other[0], first[0])
        assert other[1:4] == first[1:4], (other[1], first[1], other[2], first[2])
    return first


@pytest.fixture(scope="module")
def ctx():
    """a context whose passes are cut into two parts from two spans on (an image of 2 MiB is one span: one launch)"""
    os.environ["FQGPU_STREAM_PARTS_MIN_SPANS"] = "1"
    os.environ["FQGPU_STREAM_PARTS"] = "2"
    try:
        with fq.Context(0) as c:
            yield c
    finally:
        os.environ.pop("FQGPU_STREAM_PARTS_MIN_SPANS", None)
        os.environ.pop("FQGPU_STREAM_PARTS", None)


def test_long_reads_among_reads_of_150(ctx):
    lens = np.full(7000, L150)
    assert place(lens, 3) * STEP < len(lens) - STEP
    img, _ = image(270, lens)
    assert (2 << 20) <= len(img) <= (3 << 20), len(img)
    passes(ctx, img, accepted(img), lens, parts=1)


@pytest.fixture(scope="module")
def parted_image():
    """18.8 MiB: the long reads once in the first 16 MiB - their lines are the work of the line workers inside the fused
    launch - and once behind them, where k_stream_lines_fast counts"""
    n = (SPAN + (5 << 19)) // (2 * L150 + 22)
    lens = np.full(n, L150)
    behind = place(lens, 40)
    _, start = image(271, lens)  # (the long reads behind the first span move no record in front of them)
    tail_step = int(np.searchsorted(start, SPAN + (64 << 10))) // STEP + 2
    assert behind < tail_step - 8
    assert place(lens, tail_step) * STEP < n - 2 * STEP
    img, start = image(271, lens)
    assert SPAN + (1 << 20) < len(img) < SPAN + (3 << 20), len(img)
    assert start[behind * STEP] < SPAN - (1 << 20) and start[tail_step * STEP] > SPAN
    return img, lens, accepted(img)


def test_long_reads_beside_line_workers(ctx, parted_image):
    img, lens, want = parted_image
    passes(ctx, img, want, lens, parts=2)


@pytest.mark.parametrize("mode", ["records", "digests"])
def test_long_reads_beside_line_workers_name_modes(ctx, parted_image, mode):
    """the instantiations that capture names: the same statistics, and every name in the index"""
    img, lens, want = parted_image
    flags = A.VALIDATE_NAME_DIGESTS if mode == "digests" else A.VALIDATE_NAMES
    ctx.profile(True)
    ctx.profile_reset()
    got = run(ctx, img, flags)
    ran = {k: v[0] for k, v in ctx.profile_read().items()}
    ctx.profile(False)
    assert got[0]["path"] == 3 and ran.get("k_stream_pass1_lines(%s)" % ("digests" if mode == "digests" else "names"), 0) == 1, (got[0], ran)
    idx = ctx.name_index(len(lens) + 16)
    try:
        if mode == "digests":
            idx.expect_lookups(False)
        ir = idx.insert_unique(got[4])
        assert ir["code"] == 0 and ir["n_entries"] == len(lens), ir
    finally:
        idx.close()
    judge(got, want, lens)
    os.environ["FQGPU_STREAM_PARTS"] = "1"
    try:
        one = run(ctx, img, flags)
    finally:
        os.environ["FQGPU_STREAM_PARTS"] = "2"
    assert one[0]["path"] == 3 and one[1:4] == got[1:4], (one[0], one[1], got[1])
    assert {k: one[0][k] for k in KEYS} == {k: got[0][k] for k in KEYS}, (one[0], got[0])


@pytest.mark.parametrize("bases", [H - 2, H - 1, H])
def test_every_read_of_one_length(ctx, bases):
    lens = np.full((9 << 18) // (2 * bases + 22), bases)
    img, _ = image(272 + bases, lens)
    assert (2 << 20) <= len(img) <= (3 << 20), len(img)
    passes(ctx, img, accepted(img), lens, parts=1)
