"""The Python restatement of bam2fastq (tests/bam2fastq_oracle.py) against the reference's recorded runs
(tests/golden/bam2fastq.json, written by tools/gen_golden.py from the reference program itself): exit status, stderr,
the set of files opened, and for every run that ended well the inflated size and hash of each file.  No GPU."""
import hashlib
import json
import os

import pytest

from oracle import umi_oracle
from tests import bam2fastq_oracle as b2f
from tests.util import GOLD

GOLDEN = json.load(open(os.path.join(GOLD, "bam2fastq.json")))
_STREAMS = {}


def inflated(path):
    """the inflated bytes of a fixture BAM (read once, shared by the cases that use it), None when there is no such file"""
    if path not in _STREAMS:
        full = os.path.join(GOLD, path)
        _STREAMS[path] = umi_oracle.bgzf_inflate(open(full, "rb").read()) if os.path.exists(full) else None
    return _STREAMS[path]


def case_id(c):
    return (" ".join(c["args"]) + (" < " + c["stdin"] if c["stdin"] else ""))[-70:] or "no arguments"


def oracle_run(case):
    args = ["SCRATCH/o" if a == "OUT" else a.replace("=OUT", "=SCRATCH/o").replace("-oOUT", "-oSCRATCH/o") for a in case["args"]]
    writable = lambda name: not name.startswith("no/such/folder")
    return b2f.run(args, inflated, stdin=inflated(case["stdin"]) if case["stdin"] else b"", writable=writable)


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=[case_id(c) for c in GOLDEN])
def test_oracle_reproduces_the_reference(i):
    case = GOLDEN[i]
    status, err, files = oracle_run(case)
    assert status == case["exit"]
    assert err == case["stderr"]
    assert case["stdout"] == ""
    assert sorted(os.path.basename(n) for n in files) == sorted(case["files"])
    if status == 0:
        for name, data in files.items():
            want = case["files"][os.path.basename(name)]
            assert len(data) == want["bytes"]
            assert hashlib.sha256(data).hexdigest() == want["sha256"]
            if "content" in want:
                assert data.decode("latin-1") == want["content"]


def test_the_invocation_list_covers_what_the_fixtures_were_written_for():
    """every exit status and every message of the loop is in the golden file at least once"""
    text = "".join(c["stderr"] for c in GOLDEN)
    for needle in ("missing cell tag", "missing cell quality tag", "missing umi tag", "missing umi quality tag",
                   "missing sample quality tag", "Unable to continue", "Warning: bam file was not generated",
                   "is ambiguous", "invalid option", "requires an argument", "Failed to open BAM file"):
        assert needle in text, needle
    opened = {n[1:] for c in GOLDEN for n in c["files"]}
    assert opened >= {"_1.fastq.gz", "_2.fastq.gz", "_cell.fastq.gz", "_umi.fastq.gz", "_sample.fastq.gz", ".fastq.gz",
                      "_R1.fastq.gz", "_R2.fastq.gz", "_I1.fastq.gz"}
