"""FQGPU_GZIP_GPU=1 in fastq_pre_barcodes and bam_add_tags, after the pattern of tests/test_gpu_gzip_gpu.py.

fastq_pre_barcodes: a pick of golden invocations (good ones, --interleaved and --sam among them, and some of every other
exit status), one of them with `--outfile1 -`, one generated pair of about 3 MiB read in 1 MiB pieces and one pair with
over-long lines (the program starts over on it).  Each runs in the record-block loop (default block size, 3 and 50
records a block: many units far smaller than a member, the carry chain) and in the serial loop.  With the variable exit
status, stdout, stderr and the set of files are the golden's and the default run's, every .gz is a run of members of
exactly FQG_GZ_MEMBER_TEXT bytes of text (the rest in the last) and byte for byte what fqg_deflate makes of its text, and
all loops, block sizes and a second run write identical files.  A run that ends at a finding leaves through _exit
without closing its files, as the reference does: the file then holds the whole members only - 65 280 bytes of text each
here, 1 MiB each on the host path, so the default run's text is a prefix of this one's.  FQGPU_DEVICES=0,0 is the
documented exception (the host compressor), FQGPU_GZIP_GPU=0 the default path.

bam_add_tags: every golden invocation and one generated BAM of about 3 MiB whose header is longer than one block, to a
file and to stdout: BGZF blocks of at most FQG_GZ_MEMBER_TEXT bytes, the end-of-file block last, byte for byte what
fqg_bgzf_deflate makes of the inflated file."""
import gzip
import hashlib
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from oracle import bam_tags_oracle as bto
from tests import bamgen
from tests import test_gpu_bam_tags as t_bt
from tests import test_gpu_pre_barcodes as t_pb
from tests.test_gpu_bgzf import EOF, blocks_of
from tests.test_gpu_gzip_gpu import HOST_MEMBER, M, digest, generated, member_texts
from tests.util import GOLD, GPU_PROGRAMS_ANY_INPUT, REPO, SideBySide, strip_progress

pytestmark = pytest.mark.gpu
SWITCHES = ("FQGPU_DEVICES", "FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_GZIP_LEVEL", "FQGPU_SERIAL_LOOP", "FQGPU_BLOCK_RECORDS")
PAIRED = ["--read1", "GEN/%s_1.fastq", "--read2", "GEN/%s_2.fastq", "--cell_read", "read2", "--cell_offset", "0", "--cell_size", "12",
          "--umi_read", "read1", "--umi_offset", "4", "--umi_size", "7", "--read2_offset", "12", "--phred_encoding", "33", "--outfile1", "OUT1", "--outfile2", "OUT2"]
_LONG = {}
_MAKING = threading.Lock()  # (the programs of a sweep start from several threads: tests/util.py)


def gen_file(name):
    with _MAKING:
        if name.startswith("long_"):
            if not _LONG:
                _LONG["long_1.fastq"], _LONG["long_2.fastq"] = t_pb.make_long_mix(np.random.default_rng(77), 3000)
            return _LONG[name]
        return generated(name)


# ---- fastq_pre_barcodes ---------------------------------------------------------------------------------------------
def pb_invocations():
    """(args, environment, golden case or None, kind)"""
    G = t_pb.GOLDEN
    fastq_ok = [c for c in G if c["exit"] == 0 and c["files"] and "--sam" not in c["args"]]
    inter = [c for c in fastq_ok if "--interleaved" in c["args"]]
    plain = [c for c in fastq_ok if "--interleaved" not in c["args"]]
    sam_ok = [c for c in G if c["exit"] == 0 and "--sam" in c["args"] and "--help" not in c["args"]]
    pick, seen = plain[:3] + plain[-2:] + inter[:3] + sam_ok[:1] + [c for c in sam_ok if c["files"]][:1], {}
    for c in G:
        if c["exit"] != 0:
            seen[c["exit"]] = seen.get(c["exit"], 0) + 1
            if seen[c["exit"]] <= 3:
                pick.append(c)
    inv = [(c["args"], {}, c, "golden") for c in pick]
    first = plain[0]
    inv.append((["-" if a == "OUT1" else a for a in first["args"]], {}, first, "stdout"))
    inv.append(([a % "gen" if "%s" in a else a for a in PAIRED], {"FQGPU_CHUNK_MB": "1"}, None, "generated"))
    inv.append(([a % "long" if "%s" in a else a for a in PAIRED], {"FQGPU_CHUNK_MB": "1"}, None, "long_lines"))
    return inv


PB = pb_invocations()
GPU = {"FQGPU_GZIP_GPU": "1"}
PB_MODES = {
    # (the device compressor takes precedence over the host compressor's two switches: one run with each)
    "block": dict(GPU, FQGPU_GZIP_FAST="1"), "block_again": dict(GPU, FQGPU_GZIP_LEVEL="9"),
    "block_3": dict(GPU, FQGPU_BLOCK_RECORDS="3"), "block_50": dict(GPU, FQGPU_BLOCK_RECORDS="50"),
    "serial": dict(GPU, FQGPU_SERIAL_LOOP="1"), "default": {},
    "zero": {"FQGPU_GZIP_GPU": "0"}, "two_contexts": dict(GPU, FQGPU_DEVICES="0,0"), "two_contexts_default": {"FQGPU_DEVICES": "0,0"},
}
PB_GPU_MODES = ("block", "block_again", "block_3", "block_50", "serial")


def pb_run(key):
    """(exit, stdout bytes, stderr without the ticker, {OUT1 / OUT2: the file's bytes})"""
    i, mode = key
    args, env, _, _ = PB[i]
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    e.update(PB_MODES[mode])
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = []
        for a in args:
            if a.startswith("GEN/"):
                with open(os.path.join(tmp, a[4:]), "wb") as f:
                    f.write(gen_file(a[4:]))
                a = rel + "/" + a[4:]
            real.append(a.replace("OUT1", rel + "/o1.fastq.gz").replace("OUT2", rel + "/o2.fastq.gz"))
        p = subprocess.run(["fastq_pre_barcodes"] + real, executable=t_pb.BIN, cwd=GOLD, capture_output=True, timeout=300, env=e)
        files = {tag: open(os.path.join(tmp, fn), "rb").read() for tag, fn in (("OUT1", "o1.fastq.gz"), ("OUT2", "o2.fastq.gz"))
                 if os.path.exists(os.path.join(tmp, fn))}
    # (--sam prints its command line into the @PG line)
    return p.returncode, p.stdout.replace(rel.encode() + b"/", b"SCRATCH/"), strip_progress(p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/")), files


def pb_keys():
    keys = []
    for i, (_, _, _, kind) in enumerate(PB):
        keys += [(i, m) for m in PB_GPU_MODES + ("default",)]
        if kind == "generated":
            keys += [(i, "zero"), (i, "two_contexts"), (i, "two_contexts_default")]
    return keys


# (the pair with over-long lines starts itself again as a child: tests/util.py)
PB_RUNS = SideBySide(pb_run, pb_keys(), workers=GPU_PROGRAMS_ANY_INPUT)


@pytest.fixture(scope="module")
def ctx():
    import fastq_utils_amd as fq
    c = fq.Context(0)
    yield c
    c.close()


def inflate(raw):
    return gzip.decompress(raw) if raw else b""


def check_members(ctx, n, raw, ended_well, host_raw):
    """one .gz of a run with the variable beside the default run's"""
    host = member_texts(host_raw)
    host_text = b"".join(host)
    if not ended_well:
        # the run left at a finding without closing the file: whole members only, both ways
        assert all(len(t) == HOST_MEMBER for t in host), n
        if not raw:
            assert not host_text
            return
    texts = member_texts(raw)
    text = b"".join(texts)
    assert texts and all(len(t) == M for t in texts[:-1]) and len(texts[-1]) <= M, (n, [len(t) for t in texts])
    if ended_well:
        assert len(texts) == max(1, -(-len(text) // M)), n
        # the file is what the library makes of its text (most golden outputs are shorter than one member: the sizes of
        # the members alone would not tell the two compressors apart)
        assert raw == ctx.deflate(text)["members"], n
        assert host_text == text, n
        assert all(len(t) == HOST_MEMBER for t in host[:-1]) and len(host) == max(1, -(-len(text) // HOST_MEMBER)), n
    else:
        assert len(texts[-1]) == M and raw == ctx.deflate(text, final=False)["members"], n
        assert text.startswith(host_text) and len(text) - len(host_text) < HOST_MEMBER, n


@pytest.mark.parametrize("i", range(len(PB)), ids=["%s %s" % (v[3], " ".join(v[0])[-60:] or "(no arguments)") for v in PB])
def test_fastq_pre_barcodes_with_the_device_compressor(i, ctx):
    args, _, case, kind = PB[i]
    gpu, default = PB_RUNS.get((i, "block")), PB_RUNS.get((i, "default"))
    to_stdout = kind == "stdout"
    for got in (gpu, default):
        rc, out, err, files = got
        if case is None:
            assert rc == 0, err[-600:]
            continue
        assert rc == case["exit"], err[-600:]
        if to_stdout:  # (the golden invocation wrote a file: its text, on stdout)
            assert inflate(out).decode("latin-1") == case["files"]["OUT1"] and "OUT1" not in files
            continue
        assert err == strip_progress(case["stderr"])
        assert out.decode("latin-1") == case["stdout"]
        if rc == 0:
            for tag, want in case["files"].items():
                assert (inflate(files[tag]).decode("latin-1") if tag in files else None) == want, tag
    # the variable changes nothing but the bytes of the gzip output
    assert (gpu[0], gpu[2], sorted(gpu[3])) == (default[0], default[2], sorted(default[3]))
    streams, host_streams = dict(gpu[3]), dict(default[3])
    if to_stdout:
        streams["-"], host_streams["-"] = gpu[1], default[1]
    else:
        assert gpu[1] == default[1]  # (--sam: the text on stdout is untouched)
    # every loop, every block size and a second run: the same bytes, file by file and on stdout
    for mode in PB_GPU_MODES[1:]:
        assert PB_RUNS.get((i, mode)) == gpu, mode
    if kind == "long_lines":
        # the first run wrote whole members, the child that started over wrote the files again: the default run's text
        assert gpu[3] and {n: digest(inflate(raw)) for n, raw in gpu[3].items()} == {n: digest(inflate(raw)) for n, raw in default[3].items()}
    for n, raw in streams.items():
        check_members(ctx, n, raw, gpu[0] == 0, host_streams[n])
    if kind == "generated":
        assert min(len(member_texts(raw)) for raw in gpu[3].values()) >= 3 and len(gpu[3]) == 2
        assert sum(len(gen_file(a[4:])) for a in args if a.startswith("GEN/")) > 2 << 20
        # FQGPU_GZIP_GPU=0 is the default path byte for byte
        assert PB_RUNS.get((i, "zero")) == default
        # several contexts: the documented exception - the host compressor, whatever the variable says
        two, two_default = PB_RUNS.get((i, "two_contexts")), PB_RUNS.get((i, "two_contexts_default"))
        assert two == two_default and two[0] == 0
        assert {n: digest(raw) for n, raw in two[3].items()} == {n: digest(raw) for n, raw in default[3].items()}
        for raw in two[3].values():
            host = member_texts(raw)
            assert all(len(t) == HOST_MEMBER for t in host[:-1]) and len(host) == max(1, -(-sum(map(len, host)) // HOST_MEMBER))


def test_the_pick_covers_what_it_should():
    kinds = [v[3] for v in PB]
    cases = [v[2] for v in PB if v[2] is not None]
    assert {"golden", "stdout", "generated", "long_lines"} <= set(kinds)
    assert {c["exit"] for c in t_pb.GOLDEN} == {c["exit"] for c in cases}
    assert any("--interleaved" in c["args"] and c["exit"] == 0 and c["files"] for c in cases)
    assert any("--sam" in c["args"] and c["exit"] == 0 for c in cases)


# ---- bam_add_tags ---------------------------------------------------------------------------------------------------
_BAM = {}


def generated_bam():
    """about 3 MiB of stream whose header (3 000 references) is longer than one block; (the BGZF file, the names)"""
    with _MAKING:
        if not _BAM:
            stream, names = t_bt.make_stream(np.random.default_rng(31), 26000, refs=3000)
            _BAM["bam"], _BAM["stream"] = bamgen.bgzf(stream, level=1), stream
        return _BAM["bam"]


def bt_invocations():
    inv = [(c["args"], c) for c in t_bt.GOLDEN]
    inv.append((["--inbam", "GEN/gen.bam", "--outbam", "OUT", "--tx"], None))
    inv.append((["--inbam", "GEN/gen.bam", "--outbam", "-"], None))
    return inv


BT = bt_invocations()
BT_MODES = {"gpu": GPU, "gpu_again": dict(GPU, FQGPU_GZIP_LEVEL="9"), "default": {}}


def bt_run(key):
    i, mode = key
    args, _ = BT[i]
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(BT_MODES[mode])
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = []
        for a in args:
            if a == "GEN/gen.bam":
                with open(os.path.join(tmp, "gen.bam"), "wb") as f:
                    f.write(generated_bam())
                a = rel + "/gen.bam"
            real.append(rel + "/o.bam" if a == "OUT" else a)
        p = subprocess.run(["bam_add_tags"] + real, executable=t_bt.BIN, cwd=GOLD, capture_output=True, timeout=300, env=e)
        path = os.path.join(tmp, "o.bam")
        written = open(path, "rb").read() if os.path.exists(path) else None
    return p.returncode, p.stdout, p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), written


BT_RUNS = SideBySide(bt_run, [(i, m) for i in range(len(BT)) for m in BT_MODES])


@pytest.mark.parametrize("i", range(len(BT)), ids=[" ".join(v[0])[-70:] or "no arguments" for v in BT])
def test_bam_add_tags_with_the_device_compressor(i, ctx):
    args, case = BT[i]
    gpu, again, default = (BT_RUNS.get((i, m)) for m in ("gpu", "gpu_again", "default"))
    assert gpu == again  # two runs, the same bytes
    assert (gpu[0], gpu[2]) == (default[0], default[2])
    to_stdout = "-" in args
    if case is not None:
        assert gpu[0] == case["exit"] and gpu[2] == case["stderr"]
        assert to_stdout == case["stdout_is_bam"]
    else:
        assert gpu[0] == 0, gpu[2][-500:]
    raw, host_raw = (gpu[1], default[1]) if to_stdout else (gpu[3], default[3])
    if not to_stdout:
        assert gpu[1] == default[1]
    wrote = gpu[0] == 0 and "--help" not in args
    if not wrote:
        assert raw == host_raw  # a run that ends at a refusal writes what the default run writes (an empty file, or none)
        return
    data = gzip.decompress(raw)
    assert data == gzip.decompress(host_raw)
    if case is not None:
        assert (len(data), hashlib.sha256(data).hexdigest()) == (case["out_bytes"], case["out_sha256"])
    blocks = blocks_of(raw)
    assert blocks[-1] == (EOF, b"") and raw.endswith(EOF)
    assert all(len(t) == M for _, t in blocks[:-2]) and 0 < len(blocks[-2][1]) <= M and len(blocks) == -(-len(data) // M) + 1
    assert raw == ctx.bgzf_deflate(data)["members"]
    assert raw != host_raw  # (the default run's blocks are zlib's)
    if case is None:
        assert bto.parse_header(_BAM["stream"])[1] > M and len(data) > 2 << 20
