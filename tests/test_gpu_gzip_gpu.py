"""FQGPU_GZIP_GPU=1 in the four programs that take it (fastq_split_interleaved, fastq_trim_poly_at, fastq_filterpair,
bam2fastq): golden invocations of each - findings and usage errors among them - and one generated input of about
3 MiB read in 1 MiB pieces, so that several pieces chain their carries.  With the variable exit status, stdout, stderr
and the set of files are the golden's, what the files inflate to is the golden's, every file is a run of gzip members of
exactly FQG_GZ_MEMBER_TEXT bytes of text (the last one the rest) and byte for byte what fqg_deflate makes of that text,
and a second run writes the same bytes (one run has FQGPU_GZIP_FAST=1 beside it, the other FQGPU_GZIP_LEVEL=9).  Without it
(and with FQGPU_GZIP_GPU=0) the files are those of the host path: members of 1 MiB of text, the same bytes both times."""
import gzip
import hashlib
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests import b2f_gen, bamgen, split_gen
from tests import test_gpu_bam2fastq as t_b2f
from tests import test_gpu_filterpair as t_fp
from tests import test_gpu_filters as t_tp
from tests import test_gpu_split_interleaved as t_split
from tests.util import GOLD, REPO, SideBySide, strip_progress

pytestmark = pytest.mark.gpu
M = 65280  # FQG_GZ_MEMBER_TEXT
HOST_MEMBER = 1 << 20  # GzipMembers without the variable
GENERATED = {}


def generated(name):
    """the generated inputs, made once: name -> bytes"""
    if not GENERATED:
        recs = split_gen.pairs(23, 9000, "casava", (60, 151), (20, 151))  # about 3 MiB, interleaved
        GENERATED["gen_inter.fastq"] = b"".join(recs)
        GENERATED["gen_1.fastq"], GENERATED["gen_2.fastq"] = split_gen.deinterleave(GENERATED["gen_inter.fastq"])
        rng = np.random.default_rng(8)
        stream = b2f_gen.stream([b2f_gen.fastq2bam_record(rng, i, paired=i % 3 != 0, sample=True, long_read=90 + i % 60) for i in range(12000)])
        GENERATED["gen.bam"] = bamgen.bgzf(stream, level=1)
    return GENERATED[name]


def pick(cases, n_ok, n_bad):
    """the first n_ok invocations that end well and the first n_bad of every other exit status"""
    out, seen = [], {}
    for c in cases:
        k = c["exit"]
        seen[k] = seen.get(k, 0) + 1
        if seen[k] <= (n_ok if k == 0 else n_bad):
            out.append(c)
    return out


# ---- the four programs: (name, argv with OUT / GEN/<name> still in it, stdin, extra environment, golden case or None) ----
def invocations():
    inv = []
    for c in pick([c for c in t_split.GOLDEN if not c["args"][:1] or not c["args"][0].startswith("GEN/")], 7, 2):
        inv.append(("fastq_split_interleaved", c["args"], None, {}, c))
    inv.append(("fastq_split_interleaved", ["GEN/gen_inter.fastq", "OUT"], None, {"FQGPU_CHUNK_MB": "1"}, None))
    tp = pick(t_tp.GOLDEN["trim_poly_at"], 7, 3)
    for c in tp:
        inv.append(("fastq_trim_poly_at", c["args"], None, {}, c))
    first_ok = next(c for c in tp if c["exit"] == 0 and "OUT" in c["args"])
    inv.append(("fastq_trim_poly_at", ["-" if a == "OUT" else a for a in first_ok["args"]], None, {}, dict(first_ok, to_stdout=True)))
    inv.append(("fastq_trim_poly_at", ["--file", "GEN/gen_inter.fastq", "--outfile", "OUT"], None, {"FQGPU_CHUNK_MB": "1"}, None))
    for c in pick(t_fp.GOLDEN, 7, 2):
        inv.append(("fastq_filterpair", c["args"], None, {}, c))
    inv.append(("fastq_filterpair", ["GEN/gen_1.fastq", "GEN/gen_2.fastq"], None, {"FQGPU_CHUNK_MB": "1"}, None))
    for c in pick([c for c in t_b2f.GOLDEN if "test_one_cell" not in " ".join(c["args"])], 7, 1):
        inv.append(("bam2fastq", c["args"], c["stdin"], {}, c))
    inv.append(("bam2fastq", ["--bam", "GEN/gen.bam", "--out", "OUT"], None, {"FQGPU_CHUNK_MB": "1"}, None))
    return inv


INV = invocations()
# (the device compressor takes precedence over the host compressor's two switches: one run with each)
MODES = {"gpu": {"FQGPU_GZIP_GPU": "1", "FQGPU_GZIP_FAST": "1"}, "gpu_again": {"FQGPU_GZIP_GPU": "1", "FQGPU_GZIP_LEVEL": "9"},
         "default": {}, "zero": {"FQGPU_GZIP_GPU": "0"}}


def run(key):
    """(exit, stdout, stderr with the scratch folder named SCRATCH/, {new file: its bytes})"""
    i, mode = key
    prog, args, stdin, env, _ = INV[i]
    e = dict(os.environ)
    for k in ("FQGPU_DEVICES", "FQGPU_GZIP_GPU", "FQGPU_GZIP_FAST", "FQGPU_GZIP_LEVEL"):
        e.pop(k, None)
    e.update(env)
    e.update(MODES[mode])
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = []
        for a in args:
            if a.startswith("GEN/"):
                with open(os.path.join(tmp, a[4:]), "wb") as f:
                    f.write(generated(a[4:]))
                a = rel + "/" + a[4:]
            if prog == "fastq_trim_poly_at":
                a = rel + "/o.fastq.gz" if a == "OUT" else a
            elif prog == "fastq_filterpair":
                a = rel + "/" + a if a in ("O1", "O2") else a
            elif a.endswith("OUT"):
                a = a.replace("OUT", rel + "/o")
            real.append(a)
        if prog == "fastq_filterpair" and len(real) in (2, 3):
            real = real[:2] + [rel + "/p1.fastq.gz", rel + "/p2.fastq.gz", rel + "/up.fastq.gz"] + real[2:]
        before = set(os.listdir(tmp))
        p = subprocess.run([prog] + real, executable=os.path.join(REPO, "bin", prog), cwd=GOLD, capture_output=True, timeout=300, env=e,
                           stdin=open(os.path.join(GOLD, stdin), "rb") if stdin else subprocess.DEVNULL)
        files = {n: open(os.path.join(tmp, n), "rb").read() for n in sorted(set(os.listdir(tmp)) - before)}
    return p.returncode, p.stdout, p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), files


KEYS = [(i, m) for i in range(len(INV)) for m in ("gpu", "gpu_again", "default")] + \
       [(i, "zero") for i in range(len(INV)) if INV[i][4] is None]
RUNS = SideBySide(run, KEYS, workers=12)


@pytest.fixture(scope="module")
def ctx():
    import fastq_utils_amd as fq
    c = fq.Context(0)
    yield c
    c.close()


def member_texts(raw):
    out = []
    while raw:
        d = zlib.decompressobj(31)
        out.append(d.decompress(raw))
        assert d.eof
        raw = d.unused_data
    return out


def digest(data):
    return len(data), hashlib.sha256(data).hexdigest()


def check_golden(prog, case, got):
    rc, out, err, files = got
    assert rc == case["exit"], err[-400:]
    if case.get("to_stdout"):
        t_tp.same_text(case["out"], gzip.decompress(out))
        return
    assert out.decode("latin-1") == (case["stdout"] if prog != "bam2fastq" else "")
    if prog in ("fastq_split_interleaved", "fastq_trim_poly_at"):
        assert strip_progress(err) == strip_progress(case["stderr"])
    else:
        assert err == case["stderr"]
    if prog == "fastq_trim_poly_at":
        if case["out"] is not None:
            t_tp.same_text(case["out"], gzip.decompress(files["o.fastq.gz"]) if files.get("o.fastq.gz") else b"")
        return
    if prog == "fastq_filterpair":
        files = {n[:-len(".fastq.gz")]: raw for n, raw in files.items()} if rc == 0 else {}
    assert sorted(files) == sorted(case["files"])
    for n, want in case["files"].items():
        if rc == 0 and want is not None:
            assert digest(gzip.decompress(files[n])) == (want.get("bytes", want.get("len")), want["sha256"]), n


@pytest.mark.parametrize("i", range(len(INV)), ids=["%s %s" % (v[0], " ".join(v[1])[-50:] or "(no arguments)") for v in INV])
def test_program_with_the_device_compressor(i, ctx):
    prog, _, _, _, case = INV[i]
    gpu, again, default = RUNS.get((i, "gpu")), RUNS.get((i, "gpu_again")), RUNS.get((i, "default"))
    if case is not None:
        check_golden(prog, case, gpu)
        check_golden(prog, case, default)
    else:
        assert gpu[0] == 0, gpu[2][-400:]
    # the variable changes nothing but the bytes of the gzip files
    assert (gpu[0], gpu[2], sorted(gpu[3])) == (default[0], default[2], sorted(default[3]))
    assert gpu == again  # the same bytes, file by file and on stdout
    streams = dict(gpu[3])
    host_streams = dict(default[3])
    if case is not None and case.get("to_stdout"):
        streams["-"], host_streams["-"] = gpu[1], default[1]
    else:
        assert gpu[1] == default[1]
    for n, raw in streams.items():
        if not n.endswith(".gz") and n != "-":
            continue
        if gpu[0] != 0 and not raw:
            continue  # (a run that ended at a finding: nothing had filled a member)
        texts = member_texts(raw)
        assert texts and all(len(t) == M for t in texts[:-1]) and len(texts[-1]) <= M, (n, [len(t) for t in texts])
        assert len(texts) == max(1, -(-sum(map(len, texts)) // M)), n
        if gpu[0] == 0:
            # the file is what the library makes of its text (most golden outputs are shorter than one member: the sizes
            # of the members alone would not tell the two compressors apart)
            assert raw == ctx.deflate(b"".join(texts))["members"], n
            host = member_texts(host_streams[n])
            assert b"".join(host) == b"".join(texts), n
            assert all(len(t) == HOST_MEMBER for t in host[:-1]) and len(host) == max(1, -(-sum(map(len, host)) // HOST_MEMBER)), n
    if case is None:
        # several pieces chained their carries; and FQGPU_GZIP_GPU=0 is the host path, byte for byte
        # (1 MiB pieces of an input of more than 2 MiB: three pieces at least wrote to the largest file)
        assert max(len(member_texts(raw)) for n, raw in gpu[3].items() if n.endswith(".gz")) >= 3
        assert sum(len(gzip.decompress(generated(a[4:])) if a.endswith(".bam") else generated(a[4:]))
                   for a in INV[i][1] if a.startswith("GEN/")) > 2 << 20
        zero = RUNS.get((i, "zero"))
        assert {n: digest(raw) for n, raw in zero[3].items()} == {n: digest(raw) for n, raw in default[3].items()}
        assert zero[:3] == default[:3]
