"""bam2fastq on the GPU: the drop-in program bin/bam2fastq against the golden invocations of the reference binary
(tests/golden/bam2fastq.json: exit status, stderr, the set of files, the INFLATED bytes of each), the bulk call
fqg_bam2fastq through the C-ABI against the oracle (tests/bam2fastq_oracle.py) on seeded streams - tiles that fit LDS
and tiles that do not, with and without a 10x option, device-resident input, caller-supplied offsets, a piece that is
not the first - and the inputs this build refuses, findings behind the first record, and a run in several pieces."""
import gzip
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import b2f_gen, bamgen
from tests import bam2fastq_oracle as b2f
from tests.util import GOLD, REPO, SideBySide

pytestmark = pytest.mark.gpu
BIN = os.path.join(REPO, "bin", "bam2fastq")
GOLDEN = json.load(open(os.path.join(GOLD, "bam2fastq.json")))


def run_program(args, stdin=None, env=None):
    """bin/bam2fastq in tests/golden with OUT replaced by a scratch prefix: (status, stdout, stderr, {file: inflated})"""
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = [a.replace("OUT", rel + "/o") if a.endswith("OUT") else a for a in args]
        p = subprocess.run(["bam2fastq"] + real, executable=BIN, cwd=GOLD, capture_output=True, timeout=300,
                           stdin=open(os.path.join(GOLD, stdin), "rb") if stdin else subprocess.DEVNULL,
                           env=dict(os.environ, **(env or {})))
        files = {}
        for n in sorted(os.listdir(tmp)):
            raw = open(os.path.join(tmp, n), "rb").read()
            files[n] = gzip.decompress(raw) if p.returncode == 0 else None
    return p.returncode, p.stdout, p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), files


# (the programs of all cases start side by side the first time one is asked for: tests/util.py)
GOLDEN_RUNS = SideBySide(lambda i: run_program(GOLDEN[i]["args"], GOLDEN[i]["stdin"]), range(len(GOLDEN)))


def case_id(c):
    return (" ".join(c["args"]) + (" < " + c["stdin"] if c["stdin"] else ""))[-70:] or "no arguments"


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=[case_id(c) for c in GOLDEN])
def test_golden_invocations(i):
    case = GOLDEN[i]
    rc, out, err, files = GOLDEN_RUNS.get(i)
    assert rc == case["exit"], err[-500:]
    assert err == case["stderr"]
    assert out == b""
    assert sorted(files) == sorted(case["files"])  # (no file the reference did not open, and every one it did)
    if rc == 0:
        for n, data in files.items():
            assert len(data) == case["files"][n]["bytes"], n
            assert hashlib.sha256(data).hexdigest() == case["files"][n]["sha256"], n


@pytest.fixture(scope="module")
def ctx():
    import fastq_utils_amd as fq
    c = fq.Context(0)
    yield c
    c.close()


def make_stream(rng, n, tenx, long_every=0):
    """fastq2bam records (and, without a 10x option, records of other BAMs and secondary ones); every `long_every`-th
    read has thousands of bases: its tile does not fit LDS"""
    recs = []
    for i in range(n):
        long_read = int(rng.integers(3000, 9999)) if long_every and i % long_every == long_every - 1 else 0
        if tenx or rng.random() < 0.6:
            recs.append(b2f_gen.fastq2bam_record(rng, i, paired=not tenx and rng.random() < 0.5, cell=tenx or rng.random() < 0.7,
                                                 umi=["RX", "UB"][int(rng.integers(0, 2))] if tenx else ("RX" if rng.random() < 0.6 else ""),
                                                 sample=rng.random() < 0.3, long_read=long_read,
                                                 name=b"no at sign %d" % i if rng.random() < 0.1 else None))
        else:
            recs.append(b2f_gen.plain_record(rng, i, long_read=long_read))
    return b2f_gen.stream(recs)


def check(got, want):
    assert want["fatal"] is None and got["code"] == 0
    assert got["n_alignments"] == want["n_alignments"]
    assert got["warn_record"] == want["warn_record"]
    assert got["first_record"] == want["first_record"]
    for s in range(6):
        assert got["out_bytes"][s] == len(want["streams"][s]), s
        assert got["streams"][s] == bytes(want["streams"][s]), s


_CASES = {}


def case(n, tenx, long_every):
    """(stream, what the oracle makes of it): computed once, shared"""
    key = (n, tenx, long_every)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n + 10 * long_every + tenx)
        stream = make_stream(rng, n, tenx, long_every)
        _CASES[key] = (stream, b2f.convert(stream, tenx=tenx))
    return _CASES[key]


@pytest.mark.parametrize("long_every", [0, 7])
@pytest.mark.parametrize("tenx", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 700, 5000])
def test_bulk_call_against_the_oracle(ctx, n, tenx, long_every):
    stream, want = case(n, int(tenx), long_every)
    assert any(want["streams"])
    check(ctx.bam2fastq(stream, tenx=tenx), want)


def test_both_paths_are_taken(ctx):
    """The LDS areas are sized by the mean record (fqg_bam2fastq_abi.inc).  FQGPU_B2F_T=1 makes every alignment a tile
    of its own: in the mixed stream (mean 1.5 KB: an input area of 2 KB) every short read fits and no read of 3 000
    bases or more does.  In the second stream the fastq2bam records of 9 999 bases (25 KB with their `op`) are beyond
    the 16 KB input area and the 15 KB records of the other kind are inside it: the largest tile that goes through LDS."""
    stream, want = case(700, 0, 7)
    os.environ["FQGPU_B2F_T"] = "1"
    try:
        check(ctx.bam2fastq(stream), want)
    finally:
        del os.environ["FQGPU_B2F_T"]
    rng = np.random.default_rng(5)
    longest = b2f_gen.stream([b2f_gen.fastq2bam_record(rng, i, long_read=9999 - (i & 1), sample=True) for i in range(70)] +
                             [b2f_gen.plain_record(rng, i, long_read=9999) for i in range(70)])
    check(ctx.bam2fastq(longest), b2f.convert(longest))


_EDGES = {}


def edge_case(n, rem):
    """(stream of n short alignments whose last record's aux is padded until len(stream) % 16 == rem, what the oracle
    makes of it): computed once, shared"""
    if (n, rem) not in _EDGES:
        rng = np.random.default_rng(16 * n + rem)
        recs = [b2f_gen.fastq2bam_record(rng, i, sample=i % 3 == 0) if i % 4 else b2f_gen.plain_record(rng, i) for i in range(n - 1)]
        for pad in range(16):
            stream = b2f_gen.stream(recs + [b2f_gen.fastq2bam_record(np.random.default_rng(n), n - 1, extra=bamgen.aux_z(b"XA", b"x" * pad))])
            if len(stream) % 16 == rem:
                break
        assert len(stream) % 16 == rem
        _EDGES[(n, rem)] = (stream, b2f.convert(stream))
    return _EDGES[(n, rem)]


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device+5"])
@pytest.mark.parametrize("rem", [0, 1, 15])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_staging_edges(ctx, n, rem, resident):
    """the tile's span ends with the stream, 0, 1 and 15 bytes behind a 16-byte boundary: the last unit of the staging
    loop, read byte by byte; one tile, a full one, a full one and one alignment"""
    stream, want = edge_case(n, rem)
    if resident:
        import torch
        t = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda:0")
        t[5:5 + len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
        got = ctx.bam2fastq(t.data_ptr() + 5, offsets=b2f.record_offsets(stream), nbytes=len(stream))
    else:
        got = ctx.bam2fastq(stream)
    assert want["n_alignments"] == n and any(want["streams"])
    check(got, want)


def test_device_resident_stream_offsets_and_first_alignment(ctx):
    import torch
    stream, _ = case(5000, 1, 7)
    offs = b2f.record_offsets(stream)
    want = b2f.convert(stream, tenx=True)
    for shift in (0, 5):  # a stream that does not start at a 16-byte boundary is copied first
        t = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda:0")
        t[shift:shift + len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to("cuda:0")
        check(ctx.bam2fastq(t.data_ptr() + shift, tenx=True, offsets=offs, nbytes=len(stream)), want)
    # caller-supplied offsets: every third alignment only; as a piece that is not the first of its file
    some = offs[::3]
    got = ctx.bam2fastq(stream, tenx=True, offsets=some, first_alignment=123456)
    check(got, b2f.convert(stream, tenx=True, offsets=some, first_alignment=123456))


HDR = bamgen.header(((b"chr1", 10),))
OK = b2f_gen.record(b"ok", b"\1\2\4\10", None, bamgen.aux_z(b"on", b"ok@1:N") + bamgen.aux_z(b"op", b"IIII") + bamgen.aux_z(b"CR", b"AC") +
                    bamgen.aux_z(b"CY", b"FF") + bamgen.aux_z(b"RX", b"GT") + bamgen.aux_z(b"QX", b"EE"))


def refused(ctx, rec, code, tenx=False):
    for k in (0, 3):
        stream = HDR + OK * k + rec + OK
        with pytest.raises(b2f.Refused) as e:
            b2f.convert(stream, tenx=tenx)
        assert (e.value.code, e.value.record) == (code, k)
        got = ctx.bam2fastq(stream, tenx=tenx)
        assert (got["code"], got["record"], got["n_alignments"]) == (code, k, k)
        # nothing of that record, or of one behind it, is written: what there is are the k records in front of it
        check(dict(got, code=0), b2f.convert(HDR + OK * k, tenx=tenx))


def test_refused_inputs(ctx):
    """what the reference has no defined output for comes back as a code, at its record"""
    z = bamgen.aux_z
    refused(ctx, b2f_gen.record(b"long", bytes(10000), None, b""), b2f.E_TOO_LONG)
    refused(ctx, b2f_gen.record(b"long", bytes(10000), None, z(b"on", b"x") + z(b"CR", b"A") + z(b"CY", b"F") + z(b"RX", b"A") + z(b"QX", b"F")),
            b2f.E_TOO_LONG, tenx=True)
    check(ctx.bam2fastq(HDR + b2f_gen.record(b"fits", bytes(9999), None, b"")), b2f.convert(HDR + b2f_gen.record(b"fits", bytes(9999), None, b"")))
    refused(ctx, b2f_gen.record(b"noz", b"\1", None, z(b"on", b"name")[:-1]), b2f.E_AUX)            # a Z value without NUL
    refused(ctx, b2f_gen.record(b"cut", b"\1", None, z(b"on", b"n") + b"XIi\1\0"), b2f.E_AUX)       # an integer cut short
    refused(ctx, b2f_gen.record(b"arr", b"\1", None, b"XBBi" + b"\x40\0\0\0"), b2f.E_AUX)           # a B array beyond the record
    refused(ctx, b2f_gen.record(b"neg", b"\1", None, b"XBBc" + b"\xff\xff\xff\xff"), b2f.E_AUX)     # ... of negative length
    refused(ctx, b2f_gen.record(b"tag", b"\1", None, z(b"on", b"n") + b"X"), b2f.E_AUX)             # half a tag name
    refused(ctx, b2f_gen.record(b"typ", b"\1", None, z(b"on", b"n") + b"XY"), b2f.E_AUX)            # a name without a type
    refused(ctx, b2f_gen.record(b"seq", b"\1\2", None, b"", l_qseq=400), b2f.E_AUX)                 # bases beyond the record
    # secondary alignments are never looked at: the same records write nothing and stop nothing
    sec = b2f_gen.record(b"long", bytes(10000), None, b"XIi\1", flag=b2f_gen.SECONDARY)
    check(ctx.bam2fastq(HDR + OK + sec + OK), b2f.convert(HDR + OK + sec + OK))


@pytest.mark.parametrize("missing,code", [(b"CR", b2f.E_CELL), (b"CY", b2f.E_CELL_QUAL), (b"RX", b2f.E_UMI), (b"QX", b2f.E_UMI_QUAL),
                                          (b"QT", b2f.E_SAMPLE_QUAL), (b"on", b2f.E_NOT_FASTQ2BAM)])
def test_fatal_finding_behind_the_first_record(ctx, missing, code):
    z = bamgen.aux_z
    tags = [(b"on", b"bad@2:N"), (b"op", b"II"), (b"CR", b"AC"), (b"CY", b"FF"), (b"RX", b"GT"), (b"QX", b"EE"), (b"BC", b"SAMPLE7"), (b"QT", b"DDDDDDD")]
    bad = b2f_gen.record(b"bad", b"\1\2", None, b"".join(z(t, v) for t, v in tags if t != missing))
    k = 130   # (in the third tile of 64)
    stream = HDR + OK * k + bad + OK * 5
    want = b2f.convert(stream, tenx=True, first_alignment=1000)
    got = ctx.bam2fastq(stream, tenx=True, first_alignment=1000)
    assert want["fatal"].code == code
    assert (got["code"], got["record"], got["entry"], got["n_alignments"]) == (code, k, 1000 + k + 1, k)
    assert got["first_record"] == want["first_record"]
    assert [bytes(s) for s in want["streams"]] == got["streams"]
    if code == b2f.E_SAMPLE_QUAL:
        assert stream[got["aux"]:got["aux"] + 8] == b"SAMPLE7\0"
    # without a 10x option the same stream is converted to the end
    check(ctx.bam2fastq(stream), b2f.convert(stream))


def test_program_in_several_pieces():
    """FQGPU_CHUNK_MB=1 cuts the 7 MB stream of test_one_cell.bam into pieces: the same files and the same stderr
    (every `opening` line once, at its place) as in one piece"""
    args = ["--bam", "data_umi/test_one_cell.bam", "--out", "OUT"]
    whole = run_program(args)
    pieces = run_program(args, env={"FQGPU_CHUNK_MB": "1"})
    assert whole[0] == 0 and pieces == whole
    case = next(c for c in GOLDEN if c["args"] == args)
    assert pieces[2] == case["stderr"]
    for n, data in pieces[3].items():
        assert hashlib.sha256(data).hexdigest() == case["files"][n]["sha256"]


def test_empty_input(ctx):
    got = ctx.bam2fastq(HDR)
    assert got["code"] == 0 and got["n_alignments"] == 0 and got["out_bytes"] == [0] * 6
