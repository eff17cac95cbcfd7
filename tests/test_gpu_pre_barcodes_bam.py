"""fastq_pre_barcodes --bam: the alignment records libbam makes of the program's SAM lines, written from the GPU.

Through the C ABI (fqg_barcode_params.out_sam = FQG_OUT_BAM) against sam2bam_oracle(pre_barcodes_oracle(...)) on the
seeded cases of tests/pb_bam_cases.py, at three tile sizes; and through bin/fastq_pre_barcodes --bam: the golden --sam
invocations and the made-up inputs against what the vendored libbam made of the reference's text
(tests/golden/pre_barcodes_bam.json), in both loops, with the host and the device compressor.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import pre_barcodes_oracle as pbo
from tests import bam2fastq_oracle as b2f
from tests import pb_bam_cases, pb_bam_gen
from tests import sam2bam_oracle as s2b
from tests.util import GOLD, GPU_PROGRAMS_ANY_INPUT, REPO, SideBySide, strip_progress, thinned

pytestmark = pytest.mark.gpu
BIN = os.path.join(REPO, "bin", "fastq_pre_barcodes")
BAM2FASTQ = os.path.join(REPO, "bin", "bam2fastq")
SAM_GOLD = json.load(open(os.path.join(GOLD, "pre_barcodes.json")))
BAM_GOLD = json.load(open(os.path.join(GOLD, "pre_barcodes_bam.json")))

# ---- through the C ABI -----------------------------------------------------------------------------------------------
ABI_CASES = pb_bam_cases.cases()
_CTX = {}


def ctx():
    if not _CTX:
        import fastq_utils_amd as fq
        _CTX["c"] = fq.Context(0)
    return _CTX["c"]


@pytest.mark.parametrize("i", range(len(ABI_CASES)), ids=[c["name"] for c in ABI_CASES])
def test_abi_records_against_the_oracles(i):
    from fastq_utils_amd import abi as A
    assert pb_bam_cases.check_case(ctx(), A, ABI_CASES[i]) == ""


def test_abi_out_sam_1_still_writes_sam_text():
    from fastq_utils_amd import abi as A
    c = ABI_CASES[3]
    assert c["name"] == "pe_umi_only"
    files = {pb_bam_cases.REF_NAME[x] + ".fastq": img for x, img in c["images"].items()}
    want = pbo.run_pre_barcodes(pb_bam_cases.argv_of(c), lambda n: files[n])["stdout"].encode("latin-1").split(b"\n", 2)[2]
    frames, states = {}, {}
    try:
        for x, img in c["images"].items():
            st = A.probe_first_record(img, True)
            assert ctx().validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)["code"] == 0
            frames[x], states[x] = ctx().retain_frame(), st
        r = ctx().barcodes_transform(frames, states, c["n"], umi=c["umi"], sam=A.OUT_SAM)
        assert ctx().barcodes_output(0, r["out_bytes"][0]) == want
    finally:
        for f in frames.values():
            f.release()


def _abi_other_tiles(lds, **more):
    e = dict(os.environ, FQGPU_BC_LDS=lds, **more) if lds else dict({k: v for k, v in os.environ.items() if k != "FQGPU_BC_LDS"}, **more)
    p = subprocess.run([sys.executable, "-m", "tests.pb_bam_cases"], cwd=REPO, env=e, capture_output=True, timeout=600)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


TILE_RUNS = SideBySide(_abi_other_tiles, ["4096", "65536"])


@pytest.mark.parametrize("lds", ["4096", "65536"], ids=["tiny_tiles", "large_tiles"])
def test_abi_records_at_other_tile_sizes(lds):
    """every case above again in a process of its own: the library reads FQGPU_BC_LDS once"""
    rc, out, err = TILE_RUNS.get(lds)
    assert out.strip(), err[-2000:]
    res = json.loads(out.strip().split("\n")[-1])
    assert res["lds"] == lds and res["cases"] == len(ABI_CASES)
    assert res["failed"] == [] and rc == 0


def test_abi_records_with_two_wavefronts_in_the_grid():
    """every case once more with FQGPU_TILE_WAVES=2: a wavefront of the plan and of the emit kernel walks many tiles"""
    rc, out, err = _abi_other_tiles(None, FQGPU_TILE_WAVES="2")
    assert out.strip(), err[-2000:]
    res = json.loads(out.strip().split("\n")[-1])
    assert res["lds"] is None and res["cases"] == len(ABI_CASES)
    assert res["failed"] == [] and rc == 0


def test_abi_header_is_the_oracles():
    from fastq_utils_amd import abi as A
    argv = ["bin/fastq_pre_barcodes", "--read1", "a b.fq", "--bam", "--outfile1", "-"]
    assert A.bam_header(argv) == s2b.header_for_argv(argv[0], argv[1:])
    assert A.bam_header(["x"]) == s2b.header_for_argv("x", [])


# ---- through the program ---------------------------------------------------------------------------------------------
def run(args, cwd, env=None):
    e = dict(os.environ)
    if env:
        e.update(env)
    p = subprocess.run(["fastq_pre_barcodes"] + args, executable=BIN, cwd=cwd, capture_output=True, timeout=600, env=e)
    return p.returncode, p.stdout, p.stderr.decode("latin-1")


def as_bam(args):
    return ["--bam" if a == "--sam" else a for a in args]


def check_file(raw, argv):
    """a BGZF file that ends in the end-of-file block, cut at multiples of 65280 bytes; its header is the host function's
    for argv.  -> the record bytes"""
    from fastq_utils_amd import abi as A
    assert raw.endswith(s2b.EOF_BLOCK)
    stream, sizes = s2b.bgzf_inflate(raw)
    assert sizes[-1] == 0 and all(n == 65280 for n in sizes[:-2]) and (len(sizes) < 2 or 0 < sizes[-2] <= 65280)
    head = A.bam_header(["fastq_pre_barcodes"] + argv)
    assert stream[:len(head)] == head
    return stream[len(head):]


ENVS = {"block_loop": (), "serial_loop": (("FQGPU_SERIAL_LOOP", "1"),), "device_gzip": (("FQGPU_GZIP_GPU", "1"),),
        "device_gzip_serial_loop": (("FQGPU_GZIP_GPU", "1"), ("FQGPU_SERIAL_LOOP", "1")),
        "two_contexts_tiny_blocks": (("FQGPU_DEVICES", "0,0"), ("FQGPU_BLOCK_RECORDS", "3"), ("FQGPU_GZIP_GPU", "1"))}
GOLDEN_BAM = [c for c in BAM_GOLD if "golden" in c]


def golden_run(job):
    i, env = job
    case = GOLDEN_BAM[i]
    args = as_bam([a.replace("OUT1", "-") for a in case["args"]])
    return (args,) + run(args, GOLD, dict(env))


GOLDEN_RUNS = SideBySide(golden_run, [(i, ENVS[e]) for e in ENVS for i in range(len(GOLDEN_BAM))],
                         select=lambda ks: [k for k in ks if k[1] == ()] + [k for k in ks if k[1] != () and GOLDEN_BAM[k[0]] in thinned(GOLDEN_BAM)])


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("i", range(len(GOLDEN_BAM)), ids=["golden%d" % c["golden"] for c in GOLDEN_BAM])
def test_golden_sam_invocations_as_bam(i, env):
    case = GOLDEN_BAM[i]
    sam_case = SAM_GOLD[case["golden"]]
    args, rc, out, err = GOLDEN_RUNS.get((i, ENVS[env]))
    if case["libbam_exit"] != 0:   # (--read1_size 0: an empty SEQ, QUAL and op:Z: - libbam aborts at its first line)
        assert rc == 2 and "ERROR: read #1: the SAM line of read1 cannot be written as a BAM record" in err
        return
    assert rc == sam_case["exit"] == 0, err
    assert strip_progress(err) == strip_progress(sam_case["stderr"])
    recs = check_file(out, args)
    assert len(recs) == case["bytes"] and hashlib.sha256(recs).hexdigest() == case["sha256"]


MADE_UP = pb_bam_gen.cases()
# A tab inside the header: in the SAM text it cannot be told from the tab between two fields, and here the piece behind
# it happens to be a well-formed field, so libbam - and sam2bam_oracle, which sees the text - take the line.  The
# program knows where the string came from and refuses it (the one sub-case in which it is stricter than libbam).
REFUSED_THOUGH_THE_TEXT_PARSES = {"refused_tab_in_name": 2}   # the read number


def made_up_run(job):
    name, env = job
    files, args, _ = MADE_UP[name]
    with tempfile.TemporaryDirectory() as d:
        for fn, img in files.items():
            with open(os.path.join(d, fn), "wb") as f:
                f.write(img)
        return (as_bam(args),) + run(as_bam(args), d, dict(env))


MADE_UP_RUNS = SideBySide(made_up_run, [(n, ENVS[e]) for e in ("block_loop", "serial_loop", "device_gzip") for n in sorted(MADE_UP)],
                          workers=GPU_PROGRAMS_ANY_INPUT)


@pytest.mark.parametrize("env", ["block_loop", "serial_loop", "device_gzip"])
@pytest.mark.parametrize("name", sorted(MADE_UP))
def test_made_up_inputs_as_bam(name, env):
    case = next(c for c in BAM_GOLD if c.get("made_up") == name)
    args, rc, out, err = MADE_UP_RUNS.get((name, ENVS[env]))
    want = s2b.sam2bam(case["sam"].encode("latin-1"))
    if want["refused"] or name in REFUSED_THOUGH_THE_TEXT_PARSES:   # where libbam aborted - and the rules that are stricter than libbam
        number = REFUSED_THOUGH_THE_TEXT_PARSES.get(name) or int(case["sam"].encode("latin-1").split(b"\n")[want["refused"][0] - 1].split(b"\t")[0])
        assert rc == 2, err
        assert "ERROR: read #%d: the SAM line of read1 cannot be written as a BAM record" % number in err
        return
    assert case["libbam_exit"] == 0
    assert rc == case["exit"] == 0, err
    assert strip_progress(err) == strip_progress(case["stderr"])
    recs = check_file(out, args)
    assert len(recs) == case["bytes"] and hashlib.sha256(recs).hexdigest() == case["sha256"]
    assert recs.hex() == case.get("stream_hex", recs.hex())


def plain_pairs(rng, n, lo=40, hi=120):
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)
    r1, r2 = [], []
    for i in range(n):
        for out, mate in ((r1, b"1"), (r2, b"2")):
            L = int(rng.integers(lo, hi))
            out.append(b"@P:%d:%d %s:N:0:ACGT\n" % (i % 11, i, mate) + bases[rng.integers(0, 5, L)].tobytes() + b"\n+\n" +
                       rng.integers(35, 75, L).astype(np.uint8).tobytes() + b"\n")
    return b"".join(r1), b"".join(r2)


PAIRED = ["--read1", "r1.fastq", "--read2", "r2.fastq", "--umi_read", "read1", "--umi_offset", "0", "--umi_size", "8", "--cell_read", "read2",
          "--cell_offset", "2", "--cell_size", "10", "--phred_encoding", "33", "--outfile1", "-", "--bam"]


def test_many_batches_are_one_stream_of_full_blocks_and_bam2fastq_reads_it_back():
    """4000 pairs in batches of 300: the file is the same under every loop and compressor setting as far as it inflates
    (the blocks: 65280 bytes each, the end-of-file block last), the host compressor's files are the same bytes whatever
    the batches are, and so are the device compressor's.  Round trip: bam2fastq's oracle - a check that does not go
    through sam2bam_oracle - gives back READ1 and READ2 (names as fastq2bam stores them: blanks are '@'), and so does
    bin/bam2fastq."""
    r1, r2 = plain_pairs(np.random.default_rng(5), 4000)
    with tempfile.TemporaryDirectory() as d:
        for fn, img in (("r1.fastq", r1), ("r2.fastq", r2)):
            with open(os.path.join(d, fn), "wb") as f:
                f.write(img)
        got = {}
        for name, env in (("host", {"FQGPU_BLOCK_RECORDS": "300"}), ("host_serial", {"FQGPU_SERIAL_LOOP": "1", "FQGPU_CHUNK_MB": "1"}),
                          ("device", {"FQGPU_BLOCK_RECORDS": "300", "FQGPU_GZIP_GPU": "1"}),
                          ("device_serial", {"FQGPU_SERIAL_LOOP": "1", "FQGPU_CHUNK_MB": "1", "FQGPU_GZIP_GPU": "1"}),
                          ("two_contexts", {"FQGPU_BLOCK_RECORDS": "300", "FQGPU_DEVICES": "0,0", "FQGPU_GZIP_GPU": "1"})):
            rc, out, err = run(PAIRED, d, env)
            assert rc == 0, err
            got[name] = out
        recs = check_file(got["host"], PAIRED)
        assert len(recs) > 2 * 65280
        assert got["host"] == got["host_serial"] == got["two_contexts"]   # (several contexts: the host compressor)
        assert got["device"] == got["device_serial"] and got["device"] != got["host"]
        assert check_file(got["device"], PAIRED) == recs
        files = {"r1.fastq": r1, "r2.fastq": r2}
        sam = pbo.run_pre_barcodes(["--sam" if a == "--bam" else a for a in PAIRED], lambda n: files[n])["stdout"].encode("latin-1")
        assert recs == b"".join(s2b.sam2bam(sam)["records"])
        stream, _ = s2b.bgzf_inflate(got["host"])
        back = b2f.convert(stream)
        assert back["fatal"] is None
        assert bytes(back["streams"][b2f.R1]) == r1.replace(b" 1:N:0", b"@1:N:0")
        assert bytes(back["streams"][b2f.R2]) == r2.replace(b" 2:N:0", b"@2:N:0")
        with open(os.path.join(d, "x.bam"), "wb") as f:
            f.write(got["device"])
        p = subprocess.run(["bam2fastq", "--bam", "x.bam", "--out", "o"], executable=BAM2FASTQ, cwd=d, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode("latin-1")
        assert gzip.decompress(open(os.path.join(d, "o_1.fastq.gz"), "rb").read()) == r1.replace(b" 1:N:0", b"@1:N:0")
        assert gzip.decompress(open(os.path.join(d, "o_2.fastq.gz"), "rb").read()) == r2.replace(b" 2:N:0", b"@2:N:0")


@pytest.mark.parametrize("gz", ["0", "1"], ids=["host_gzip", "device_gzip"])
def test_a_run_that_starts_over_writes_the_file_of_its_reframed_input(gz):
    """A header line beyond the 1000 bytes of the reference's buffer, late in a plain file: the run has written blocks
    when the GPU finds it and starts over on input cut where gzgets cuts it (the rest of that header is the read's
    sequence); the second run skips as many bytes of stdout as the first one wrote - they must be the same bytes.  The file
    is the one the re-framed run writes alone, and its records are the oracles'."""
    rng = np.random.default_rng(77)
    r1, _ = plain_pairs(rng, 3000, 90, 110)
    recs = r1.split(b"\n")
    k = 2600
    recs[4 * k:4 * k + 2] = [b"@" + b"h" * 998 + b"ACGTACGTAC"]   # (three lines: this one, "+", ten quality characters)
    recs[4 * k + 2] = recs[4 * k + 2][:10]
    img = b"\n".join(recs)
    args = ["--read1", "r1.fastq", "--umi_read", "read1", "--umi_offset", "0", "--umi_size", "6", "--outfile1", "-", "--bam"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "r1.fastq"), "wb") as f:
            f.write(img)
        rc, out, err = run(args, d, {"FQGPU_BLOCK_RECORDS": "200", "FQGPU_GZIP_GPU": gz})
        rc2, out2, err2 = run(args, d, {"FQGPU_REFRAME": "1", "FQGPU_GZIP_GPU": gz})
        assert rc == rc2 == 0, (err, err2)
        assert out == out2
        assert strip_progress(err) == strip_progress(err2)
        got = check_file(out, args)
        sam = pbo.run_pre_barcodes(["--sam" if a == "--bam" else a for a in args], lambda n: img)["stdout"].encode("latin-1")
        want = s2b.sam2bam(sam)
        assert want["refused"] is None and len(want["records"]) == 3000
        assert got == b"".join(want["records"])
        assert b"onZ" + b"h" * 998 + b"\0" in got


def test_timing_and_json_metrics_keep_working():
    r1, r2 = plain_pairs(np.random.default_rng(6), 500)
    with tempfile.TemporaryDirectory() as d:
        for fn, img in (("r1.fastq", r1), ("r2.fastq", r2)):
            with open(os.path.join(d, fn), "wb") as f:
                f.write(img)
        rc, out, err = run(PAIRED, d, {"FQGPU_JSON_METRICS": os.path.join(d, "m.json"), "FQGPU_TIMING": "1"})
        assert rc == 0, err
        m = json.load(open(os.path.join(d, "m.json")))
        assert m["reads"] == 500 and m["discarded"] == 0
        assert "fqgpu timing:" in err
        check_file(out, PAIRED)
