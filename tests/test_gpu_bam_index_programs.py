"""FQGPU_INDEX_GPU=1 (with FQGPU_INFLATE_GPU=1): the three programs that read a BAM file with the record index made on the
device - the inflated stream never comes back to the host.

The golden invocations of bam2fastq, bam_add_tags and bam_umi_count run with the two switches and FQGPU_INDEX_DEBUG=1, once
without and once with FQGPU_GZIP_GPU=1: exit status, stdout and every output file are the golden's (what the run without
the switches gives: tests/test_gpu_bam2fastq.py, test_gpu_bam_tags.py, test_gpu_umi.py), stderr too once the [index] line
is taken out, and that line says `device` with the record count of the host's walk over the input.  Fixed cases: files of
tests/bgzfgen.py that inflate and are, or are not, BAM streams, a last record cut short, a header whose references run
past the stream, the switch without FQGPU_INFLATE_GPU, and bam_umi_count over two contexts, which keeps the host's walk."""
import gzip
import hashlib
import os
import re
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import bamgen, bamidx_gen, bgzfgen
from tests import test_gpu_bam2fastq as t_b2f
from tests import test_gpu_bam_tags as t_tags
from tests import test_gpu_umi as t_umi
from tests.test_gpu_inflate_programs import all_three, bgzf_file, run_tags, run_umi, with_file
from tests.test_oracle_umi import golden_files, want_exit
from tests.util import GOLD, GPU_PROGRAMS, thinned

pytestmark = pytest.mark.gpu
ON = {"FQGPU_INFLATE_GPU": "1", "FQGPU_INDEX_GPU": "1", "FQGPU_INDEX_DEBUG": "1"}
BOTH = (ON, dict(ON, FQGPU_GZIP_GPU="1"))
DEBUG_LINE = re.compile(r"\[index\] [^\n]*\n")


def split_debug(err):
    """(stderr without the [index] lines, the lines)"""
    return DEBUG_LINE.sub("", err), DEBUG_LINE.findall(err)


def index_line(raw, where="device"):
    """what FQGPU_INDEX_DEBUG=1 says of the file `raw`, from the host's walk; None for a file that does not inflate"""
    try:
        stream = gzip.decompress(raw) if raw else b""
    except (OSError, EOFError, zlib.error):
        return None
    lib = bamidx_gen.library_walk(stream)   # fqg_bam_index_records
    if lib is None:
        return "[index] %s: refused\n" % where
    return "[index] %s: %d records\n" % (where, len(lib[0]))


def input_line(args, stdin=None):
    """the [index] line of an invocation: of the .bam file it names (however getopt_long lets the option be spelled) or
    is fed; None when there is none, or none that inflates"""
    path = stdin
    for a in args:
        for part in (a, a.split("=", 1)[-1], a[2:]):   # --bam x, --bam=x, -bx
            if part.endswith(".bam") and os.path.isfile(os.path.join(GOLD, part)):
                path = part
    if not path or not os.path.isfile(os.path.join(GOLD, path)):
        return None
    return index_line(open(os.path.join(GOLD, path), "rb").read())


def said_right(said, want, rc, err):
    """the one line the host's walk gives, or none at all where the program left before it had a stream - which a run
    that succeeded on a file did not (--help beside a file name succeeds too)"""
    if said:
        return want is not None and said == [want]
    return want is None or rc != 0 or "Usage: " in err


def sweep(cases, one, env):
    """the invocations that take a BAM file, thinned, under `env`"""
    cases = [c for c in cases if input_line(c["args"], c.get("stdin")) is not None]
    assert len(cases) >= 10
    cases = [(c, env) for c in thinned(cases)]
    with ThreadPoolExecutor(GPU_PROGRAMS) as ex:
        results = list(ex.map(lambda ce: one(*ce), cases))
    bad = [r[0] for r in results if r[0]]
    assert not bad, f"{len(bad)} of {len(cases)} differ; first: {bad[:3]}"
    said = [line for r in results for line in r[1]]
    assert sum(line.startswith("[index] device: ") and line.endswith(" records\n") for line in said) >= 2, said[:5]
    assert not any(" host" in line for line in said), said[:5]
    return len(cases)


@pytest.mark.parametrize("env", BOTH, ids=("host_gzip", "FQGPU_GZIP_GPU"))
def test_bam2fastq_golden_invocations(env):
    def one(case, env):
        rc, out, err, files = t_b2f.run_program(case["args"], case["stdin"], env=env)
        err, said = split_debug(err)
        ok = (rc == case["exit"] and err == case["stderr"] and out == b"" and sorted(files) == sorted(case["files"]) and
              (rc != 0 or all(len(d) == case["files"][n]["bytes"] and hashlib.sha256(d).hexdigest() == case["files"][n]["sha256"]
                              for n, d in files.items())))
        ok = ok and said_right(said, input_line(case["args"], case["stdin"]), rc, err)
        return (None if ok else (t_b2f.case_id(case), rc, err[-300:], said)), said

    assert sweep(t_b2f.GOLDEN, one, env) > 0


@pytest.mark.parametrize("env", BOTH, ids=("host_gzip", "FQGPU_GZIP_GPU"))
def test_bam_add_tags_golden_invocations(env):
    def one(case, env):
        rc, out, err, written = run_tags(case["args"], env)
        err, said = split_debug(err)
        ok = rc == case["exit"] and err == case["stderr"]
        if ok and not case["stdout_is_bam"]:
            ok = (written is not None) == case["out_created"] and out.decode("latin-1") == case.get("stdout", "")
        if ok and "out_sha256" in case:
            data = gzip.decompress(out if case["stdout_is_bam"] else written)
            ok = len(data) == case["out_bytes"] and hashlib.sha256(data).hexdigest() == case["out_sha256"]
        ok = ok and said_right(said, input_line(case["args"]), rc, err)
        return (None if ok else (" ".join(case["args"]), rc, err[-300:], said)), said

    assert sweep(t_tags.GOLDEN, one, env) > 0


@pytest.mark.parametrize("env", BOTH, ids=("host_gzip", "FQGPU_GZIP_GPU"))
def test_bam_umi_count_golden_invocations(env):
    def one(case, env):
        rc, err, got = run_umi(case["args"], env)
        err, said = split_debug(err)
        ok = (rc if rc >= 0 else 128 - rc) == want_exit(case)
        if ok and case["exit"] == -6:
            ok = "Assertion `len1+1 < FEAT_ID_MAX_LEN' failed" in err
        elif ok:
            ok = err == case["stderr"] and (case["exit"] != 0 or got == golden_files(case))
        ok = ok and said_right(said, input_line(case["args"]), rc, err)
        return (None if ok else (" ".join(case["args"]), rc, err[-300:], said)), said

    assert sweep(t_umi.CLI_CASES, one, env) > 0


# ---- fixed cases ------------------------------------------------------------------------------
def strip_all(results):
    """the results of all_three with the [index] lines out of the three stderr texts; and the lines"""
    out, said = [], []
    for res in results:
        k = 1 if len(res) == 3 else 2   # (bam_umi_count has no stdout entry)
        err, lines = split_debug(res[k])
        out.append(res[:k] + (err,) + res[k + 1:])
        said.append(lines)
    return out, said


def damaged_bams():
    stream, _ = t_tags.make_stream(np.random.default_rng(78), 300)
    offs, used = bamidx_gen.library_walk(stream)
    assert len(offs) == 300 and used == len(stream)
    q = 8 + struct.unpack_from("<i", stream, 4)[0]   # n_ref
    l_name = struct.unpack_from("<i", stream, q + 4)[0]
    files = {"whole": stream, "last-record-cut": stream[:-9], "cut-inside-a-block-size": stream[:offs[-1] + 2],
             "header-only": stream[:offs[0]], "references-past-the-stream": stream[:q + 4] + struct.pack("<i", len(stream)) + stream[q + 8:],
             "header-cut": stream[:q + 8 + l_name // 2], "wrong-magic": b"BAM\2" + stream[4:], "a-block-size-of-31": stream[:offs[150]] +
             struct.pack("<i", 31) + stream[offs[150] + 4:]}
    return {name: b"".join(bgzf_file(s)) for name, s in files.items()}


@pytest.fixture(scope="module")
def bam_level_files():
    """name -> (the file, what the three programs do with it without the switches)"""
    W = bgzfgen.well_formed()
    files = {name: W[name] for name in ("bam-l6", "fastq-l6", "empty-l6", "one-l6")}
    files.update(damaged_bams())
    with ThreadPoolExecutor(GPU_PROGRAMS) as ex:
        off = list(ex.map(lambda raw: strip_all(all_three(raw, {}))[0], files.values()))
    return {name: (raw, o) for (name, raw), o in zip(files.items(), off)}


def test_the_host_path_accepts_and_refuses_them_at_the_bam_level(bam_level_files):
    not_bam = "\nERROR: IN/in.bam is not a BAM file\n"
    for name in ("fastq-l6", "empty-l6", "one-l6", "references-past-the-stream", "header-cut", "wrong-magic"):
        assert all(res[0] == 2 and not_bam in res[-2] for res in bam_level_files[name][1]), name
    for name in ("whole", "last-record-cut"):
        assert bam_level_files[name][1][1][0] == 0, name   # bam_add_tags wrote its file


@pytest.mark.parametrize("env", BOTH, ids=("host_gzip", "FQGPU_GZIP_GPU"))
def test_files_that_are_and_are_not_bam_streams(bam_level_files, env):
    def one(item):
        name, (raw, off) = item
        on, said = strip_all(all_three(raw, env))
        if on != off or said != [[index_line(raw)]] * 3:
            return name, said, [a[:3] for a, b in zip(on, off) if a != b][:1]

    with ThreadPoolExecutor(GPU_PROGRAMS) as ex:
        bad = [r for r in ex.map(one, bam_level_files.items()) if r]
    assert not bad, bad[:3]


def test_the_switch_alone_is_the_default_path():
    bam, _ = bamgen.tagged_bam(np.random.default_rng(3), n_cells=6, genes=10)
    want = index_line(bam, "host")

    def tags(env):
        rc, out, err, written = with_file(bam, lambda rel, tmp: run_tags(["--inbam", rel, "--outbam", "OUT"], env))
        return rc, out, re.sub(r"\S*in\.bam", "IN", err), written

    off = tags({})
    assert off[0] == 0 and split_debug(off[2])[1] == []
    for env in ({"FQGPU_INDEX_GPU": "1", "FQGPU_INDEX_DEBUG": "1"}, {"FQGPU_INFLATE_GPU": "1", "FQGPU_INDEX_GPU": "0", "FQGPU_INDEX_DEBUG": "1"},
                {"FQGPU_INDEX_DEBUG": "1"}):
        rc, out, err, written = tags(env)
        err, said = split_debug(err)
        assert said == [want] and (rc, out, err, gzip.decompress(written)) == off[:3] + (gzip.decompress(off[3]),), env


def test_bam_umi_count_over_two_contexts_keeps_the_host_walk():
    bam, _ = bamgen.tagged_bam(np.random.default_rng(3), n_cells=6, genes=10)
    runs = {}
    for name, env in (("two", dict(ON, FQGPU_DEVICES="0,0")), ("one", ON), ("off", {})):
        rc, err, got = with_file(bam, lambda rel, tmp: run_umi(["--bam", rel, "--ucounts", "OUTU"], env))
        err, said = split_debug(err)
        runs[name] = (rc, re.sub(r"\S*in\.bam", "IN", err), got, said)
    assert runs["two"][3] == [index_line(bam, "host")] and runs["one"][3] == [index_line(bam, "device")] and runs["off"][3] == []
    assert runs["off"][0] == 0 and runs["two"][:3] == runs["one"][:3] == runs["off"][:3]
