"""GPU parity for bin/fastq_split_interleaved: every golden invocation of the reference program
(tests/golden/split_interleaved.json) for exit status, stdout, stderr, which files exist and - for exit 0 - the inflated
bytes of both outputs; and the piece loop: pieces that frame an odd number of records, findings behind the first piece."""
import gzip
import hashlib
import json
import os
import subprocess
import tempfile

import pytest

from tests import split_gen
from tests.util import GOLD, REPO, SideBySide, strip_progress

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(GOLD, "split_interleaved.json")))
BIN = os.path.join(REPO, "bin", "fastq_split_interleaved")
BIG = {}


def big(name):
    if not BIG:
        BIG.update(split_gen.big_files())
    return BIG[name]


def run_case(args, env=None):
    """(exit, stdout, stderr with the scratch folder named SCRATCH/, {new file: inflated bytes})"""
    e = dict(os.environ)
    e.pop("FQGPU_DEVICES", None)
    e.update(env or {})
    with tempfile.TemporaryDirectory(dir=GOLD) as tmp:
        rel = os.path.relpath(tmp, GOLD)
        real = []
        for a in args:
            if a.startswith("GEN/"):
                with open(os.path.join(tmp, a[4:]), "wb") as f:
                    f.write(big(a[4:]))
                a = rel + "/" + a[4:]
            real.append(rel + "/o" if a == "OUT" else a)
        before = set(os.listdir(tmp))
        p = subprocess.run(["fastq_split_interleaved"] + real, executable=BIN, cwd=GOLD, capture_output=True, timeout=600, env=e,
                           stdin=subprocess.DEVNULL)
        files = {}
        for n in sorted(set(os.listdir(tmp)) - before):
            raw = open(os.path.join(tmp, n), "rb").read()
            files[n] = gzip.decompress(raw) if p.returncode == 0 else None
    return p.returncode, p.stdout.decode("latin-1"), p.stderr.decode("latin-1").replace(rel + "/", "SCRATCH/"), files


def check(case, got):
    rc, out, err, files = got
    assert rc == case["exit"], err
    assert out == case["stdout"]
    assert strip_progress(err) == strip_progress(case["stderr"])
    assert sorted(files) == sorted(case["files"])
    for name, want in case["files"].items():
        if want is None:
            continue
        assert (len(files[name]), hashlib.sha256(files[name]).hexdigest()) == (want["bytes"], want["sha256"]), name
        if "content" in want:
            assert files[name].decode("latin-1") == want["content"]


# (the programs of all cases start side by side the first time one is asked for: tests/util.py)
RUNS = SideBySide(lambda i: run_case(GOLDEN[i]["args"]), range(len(GOLDEN)))


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=[" ".join(c["args"])[-60:] or "(no arguments)" for c in GOLDEN])
def test_golden(i):
    check(GOLDEN[i], RUNS.get(i))


def golden_of(first_arg):
    return [c for c in GOLDEN if c["args"][:1] == [first_arg]][0]


def pieces_of_1mib(image):
    """records framed by every piece of the loop when pieces are 1 MiB: a piece is what the last one carried plus 1 MiB
    (the whole rest at the end), and an odd last record is carried with the tail"""
    ends, at = [], 0
    for ln in split_gen.lines_of(image):
        at += len(ln)
        ends.append(at)
    rec_end = ends[3::4]
    counts, start, fresh, done = [], 0, 0, 0
    while True:
        fresh = min(fresh + (1 << 20), len(image))
        n = sum(1 for e in rec_end[done:] if e <= fresh)
        counts.append(n)
        if fresh == len(image):
            return counts
        done += n - (n & 1)


def test_pieces_with_an_odd_number_of_records_give_the_one_piece_result():
    image = big("big_clean.fastq")
    counts = pieces_of_1mib(image)
    assert len(counts) >= 3 and any(n & 1 for n in counts[:-1]), counts
    case = golden_of("GEN/big_clean.fastq")
    one = run_case(case["args"])
    many = run_case(case["args"], {"FQGPU_CHUNK_MB": "1"})
    check(case, many)
    assert many == one
    assert (many[3]["o_1.fastq.gz"], many[3]["o_2.fastq.gz"]) == split_gen.deinterleave(image)


@pytest.mark.parametrize("name", ["big_mismatch.fastq", "big_trunc.fastq"])
def test_findings_behind_the_first_piece_carry_the_reference_line_numbers(name):
    case = golden_of("GEN/" + name)
    line = int(case["stderr"].split(": line ")[1].split(":")[0])
    assert case["exit"] != 0 and line > 4 * pieces_of_1mib(big("big_clean.fastq"))[0]  # (behind the first piece's records)
    check(case, run_case(case["args"], {"FQGPU_CHUNK_MB": "1"}))
