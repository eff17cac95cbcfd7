"""FQGPU_INFLATE_GPU=1: the three programs that read a BAM file with their BGZF input inflated on the device.

The golden invocations of bam2fastq, bam_add_tags and bam_umi_count run once more with the variable: exit status, stdout,
stderr and every output file are the golden's, byte for byte; on every fourth run FQGPU_INFLATE_DEBUG=1 adds the line
that says which inflate ran.  Fixed cases: a block zlib refuses (the message and status of the host path), a wrong stored
CRC-32 (not looked at, as the host path does not), FQGPU_INFLATE_GPU=0, bam_umi_count over two contexts, which keeps
the host inflate, and the chain of two programs: a BAM file that fastq_pre_barcodes --bam compressed on the device,
inflated on the device by bam2fastq."""
import gzip
import hashlib
import os
import re
import subprocess
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import bamgen, bgzfgen
from tests import test_gpu_bam2fastq as t_b2f
from tests import test_gpu_bam_tags as t_tags
from tests import test_gpu_umi as t_umi
from tests.test_oracle_umi import golden_files, want_exit
from tests.util import GOLD, GPU_PROGRAMS, thinned

pytestmark = pytest.mark.gpu
ON = {"FQGPU_INFLATE_GPU": "1"}
DEBUG_LINE = re.compile(r"\[inflate\] [^\n]*\n")


def env_of(k, base=ON):
    return dict(base, FQGPU_INFLATE_DEBUG="1") if k % 4 == 0 else dict(base)


def split_debug(err):
    """(stderr without the debug lines, the debug lines)"""
    return DEBUG_LINE.sub("", err), DEBUG_LINE.findall(err)


def sweep(cases, one):
    """one(k, case) -> (what differs or None, debug lines); all cases side by side"""
    cases = thinned(cases)
    with ThreadPoolExecutor(GPU_PROGRAMS) as ex:
        results = list(ex.map(lambda kc: one(*kc), enumerate(cases)))
    bad = [r[0] for r in results if r[0]]
    assert not bad, f"{len(bad)} of {len(cases)} differ; first: {bad[:3]}"
    said = [line for r in results for line in r[1]]
    assert said and all(line.startswith("[inflate] device: ") for line in said), said[:5]   # the device path was taken
    return len(cases)


def test_bam2fastq_golden_invocations():
    def one(k, case):
        rc, out, err, files = t_b2f.run_program(case["args"], case["stdin"], env=env_of(k))
        err, said = split_debug(err)
        ok = (rc == case["exit"] and err == case["stderr"] and out == b"" and sorted(files) == sorted(case["files"]) and
              (rc != 0 or all(len(d) == case["files"][n]["bytes"] and hashlib.sha256(d).hexdigest() == case["files"][n]["sha256"]
                              for n, d in files.items())))
        return (None if ok else (t_b2f.case_id(case), rc, err[-300:])), said

    assert sweep(t_b2f.GOLDEN, one) > 0


def run_tags(args, env):
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = [rel + "/o.bam" if a == "OUT" else a for a in args]
        p = subprocess.run(["bam_add_tags"] + real, executable=t_tags.BIN, cwd=GOLD, capture_output=True, timeout=300,
                           env=dict(os.environ, **env))
        path = os.path.join(tmp, "o.bam")
        written = open(path, "rb").read() if os.path.exists(path) else None
    return p.returncode, p.stdout, p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), written


def test_bam_add_tags_golden_invocations():
    def one(k, case):
        rc, out, err, written = run_tags(case["args"], env_of(k))
        err, said = split_debug(err)
        ok = rc == case["exit"] and err == case["stderr"]
        if ok and not case["stdout_is_bam"]:
            ok = (written is not None) == case["out_created"] and out.decode("latin-1") == case.get("stdout", "")
        if ok and "out_sha256" in case:
            data = gzip.decompress(out if case["stdout_is_bam"] else written)
            ok = len(data) == case["out_bytes"] and hashlib.sha256(data).hexdigest() == case["out_sha256"]
        return (None if ok else (" ".join(case["args"]), rc, err[-300:])), said

    assert sweep(t_tags.GOLDEN, one) > 0


def run_umi(args, env, cwd=GOLD):
    with tempfile.TemporaryDirectory(dir=cwd) as tmp:
        rel = os.path.relpath(tmp, cwd)
        real = [a.replace("OUTU", rel + "/u.mtx").replace("OUTR", rel + "/r.mtx") for a in args]
        p = subprocess.run(["bam_umi_count"] + real, executable=t_umi.BIN, cwd=cwd, capture_output=True, timeout=300,
                           env=dict(os.environ, **env))
        got = {}
        for base in ("u.mtx", "r.mtx"):
            for ext in ("", "_rows", "_cols"):
                path = os.path.join(tmp, base + ext)
                if os.path.exists(path):
                    got["SCRATCH/" + base + ext] = open(path, "rb").read().decode("latin-1")
    return p.returncode, p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), got


def test_bam_umi_count_golden_invocations():
    def one(k, case):
        rc, err, got = run_umi(case["args"], env_of(k))
        err, said = split_debug(err)
        ok = (rc if rc >= 0 else 128 - rc) == want_exit(case)
        if ok and case["exit"] == -6:
            ok = "Assertion `len1+1 < FEAT_ID_MAX_LEN' failed" in err
        elif ok:
            ok = err == case["stderr"] and (case["exit"] != 0 or got == golden_files(case))
        return (None if ok else (" ".join(case["args"]), rc, err[-300:])), said

    assert sweep(t_umi.CLI_CASES, one) > 0


# ---- fixed cases ------------------------------------------------------------------------------
def bgzf_file(stream, piece=3000):
    return [bgzfgen.text_block(stream[k:k + piece]) for k in range(0, len(stream), piece)] + [bgzfgen.EOF]


@pytest.fixture(scope="module")
def tags_bam():
    stream, _ = t_tags.make_stream(np.random.default_rng(77), 400)
    return stream, bgzf_file(stream)


def with_file(raw, fn):
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        path = os.path.join(tmp, "in.bam")
        open(path, "wb").write(raw)
        return fn(os.path.relpath(path, GOLD), os.path.relpath(tmp, GOLD))


def all_three(raw, env):
    """(status, stdout, stderr, files) of the three programs on one file"""
    def run(rel, tmp):
        out = []
        rc, so, err, files = t_b2f.run_program(["--bam", rel, "--out", "OUT"], env=env)
        out.append((rc, so, err.replace(tmp + "/", "IN/"), files))
        rc, so, err, written = run_tags(["--inbam", rel, "--outbam", "OUT"], env)
        out.append((rc, so, err.replace(tmp + "/", "IN/"), written and gzip.decompress(written)))
        rc, err, got = run_umi(["--bam", rel, "--ucounts", "OUTU"], env)
        out.append((rc, err.replace(tmp + "/", "IN/"), got))
        return out
    return with_file(raw, run)


def test_a_block_that_does_not_inflate(tags_bam):
    _, blocks = tags_bam
    assert len(blocks) > 4
    r, damaged = np.random.default_rng(5), None
    for _ in range(50):   # a flipped bit in the third block's payload that zlib refuses
        b = bytearray(blocks[2])
        bit = int(r.integers(18 * 8, (len(b) - 8) * 8))
        b[bit >> 3] ^= 1 << (bit & 7)
        raw = b"".join(blocks[:2]) + bytes(b) + b"".join(blocks[3:])
        if bgzfgen.verdict(raw)["bad_block"] == 2:
            damaged = raw
            break
    assert damaged is not None
    off, on = all_three(damaged, {}), all_three(damaged, ON)
    assert on == off
    for res in on:
        assert res[0] == 2 and "\nERROR: IN/in.bam is not a readable BGZF / BAM file\n" in res[-2 if len(res) == 3 else 2]


def test_a_wrong_stored_crc(tags_bam):
    stream, blocks = tags_bam
    b = bytearray(blocks[1])
    b[-8] ^= 0x40
    raw = blocks[0] + bytes(b) + b"".join(blocks[2:])
    v = bgzfgen.verdict(raw)
    assert v["bad_block"] == bgzfgen.NONE and v["crc_block"] == 1
    off, on = all_three(raw, {}), all_three(raw, ON)
    assert on == off
    assert on[1][0] == 0 and on[1][3] is not None and len(on[1][3]) >= len(stream)   # bam_add_tags wrote its BAM


def test_the_variable_set_to_0_is_the_default_path(tags_bam):
    raw = b"".join(tags_bam[1])
    env = {"FQGPU_INFLATE_GPU": "0", "FQGPU_INFLATE_DEBUG": "1"}
    rc, out, err, written = with_file(raw, lambda rel, tmp: run_tags(["--inbam", rel, "--outbam", "OUT"], env))
    assert rc == 0 and split_debug(err)[1] == ["[inflate] host: %d blocks\n" % len(tags_bam[1])]
    rc1, out1, err1, written1 = with_file(raw, lambda rel, tmp: run_tags(["--inbam", rel, "--outbam", "OUT"], dict(ON, FQGPU_INFLATE_DEBUG="1")))
    assert split_debug(err1)[1] == ["[inflate] device: %d blocks\n" % len(tags_bam[1])]
    assert (rc1, out1, gzip.decompress(written1)) == (rc, out, gzip.decompress(written))


def test_bam_umi_count_over_two_contexts_keeps_the_host_inflate():
    bam, _ = bamgen.tagged_bam(np.random.default_rng(3), n_cells=6, genes=10)
    runs = {}
    for name, env in (("two", dict(ON, FQGPU_DEVICES="0,0", FQGPU_INFLATE_DEBUG="1")), ("one", dict(ON, FQGPU_INFLATE_DEBUG="1")), ("off", {})):
        rc, err, got = with_file(bam, lambda rel, tmp: run_umi(["--bam", rel, "--ucounts", "OUTU"], env))
        err, said = split_debug(err)
        runs[name] = (rc, re.sub(r"\S*in\.bam", "IN", err), got, said)
    assert runs["two"][3][0].startswith("[inflate] host: ") and runs["one"][3][0].startswith("[inflate] device: ")
    assert runs["off"][0] == 0 and runs["off"][3] == []
    assert runs["two"][:3] == runs["one"][:3] == runs["off"][:3]


def test_a_file_compressed_on_the_device_is_inflated_on_the_device():
    from tests import test_gpu_pre_barcodes_bam as t_pb
    r1, r2 = t_pb.plain_pairs(np.random.default_rng(19), 700)
    with tempfile.TemporaryDirectory() as d:
        for fn, img in (("r1.fastq", r1), ("r2.fastq", r2)):
            with open(os.path.join(d, fn), "wb") as f:
                f.write(img)
        rc, bam, err = t_pb.run(t_pb.PAIRED, d, {"FQGPU_GZIP_GPU": "1"})
    assert rc == 0, err
    v = bgzfgen.verdict(bam)
    assert v["n_blocks"] >= 4 and v["bad_block"] == v["crc_block"] == bgzfgen.NONE   # three blocks of records or more
    runs = {}
    for name, env in (("device", dict(ON, FQGPU_INFLATE_DEBUG="1")), ("host", {})):
        rc, out, err, files = with_file(bam, lambda rel, tmp: t_b2f.run_program(["--bam", rel, "--out", "OUT"], env=env))
        err, said = split_debug(re.sub(r"\S*in\.bam", "IN", err))
        runs[name] = (rc, out, err, files, said)
    assert runs["device"][4] == ["[inflate] device: %d blocks\n" % v["n_blocks"]] and runs["host"][4] == []
    assert runs["device"][:4] == runs["host"][:4]
    rc, out, err, files = runs["device"][:4]
    assert rc == 0 and out == b"", err
    assert files["o_1.fastq.gz"] == r1.replace(b" 1:N:0", b"@1:N:0")
    assert files["o_2.fastq.gz"] == r2.replace(b" 2:N:0", b"@2:N:0")
