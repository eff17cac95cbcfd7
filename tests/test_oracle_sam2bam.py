"""tests/sam2bam_oracle.py against what the vendored libbam (samtools 0.1.19) made of the reference's SAM text
(tests/golden/pre_barcodes_bam.json, tools/gen_golden.py pre_barcodes_bam).  No GPU."""
import hashlib
import json
import os
import re

import pytest

from oracle import pre_barcodes_oracle as pbo
from tests import pb_bam_gen
from tests import sam2bam_oracle as s2b
from tests.util import GOLD

CASES = json.load(open(os.path.join(GOLD, "pre_barcodes_bam.json")))
SAM_GOLD = json.load(open(os.path.join(GOLD, "pre_barcodes.json")))
IDS = [("golden%d" % c["golden"]) if "golden" in c else c["made_up"] for c in CASES]
# Made-up inputs that libbam takes and the program refuses.  A base >= 0x80: libbam reads in front of its table and goes
# on; the oracle refuses the line.  A tab inside the header whose pieces happen to be well-formed fields: nothing in the
# SAM text tells it from a separator, so the oracle takes the line as libbam does - only the program, which knows
# where the string came from, can refuse (tests/test_gpu_pre_barcodes_bam.py).
STRICTER = {"refused_tab_in_name", "refused_high_base"}


def sam_of(case):
    return (SAM_GOLD[case["golden"]]["stdout"] if "golden" in case else case["sam"]).encode("latin-1")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_oracle_reproduces_libbam(i):
    case = CASES[i]
    got = s2b.sam2bam(sam_of(case))
    if case["libbam_exit"] != 0:
        # libbam aborted: the oracle refuses, and at the line libbam names
        assert case["libbam_exit"] == -6
        assert got["refused"] is not None
        m = re.search(r"Parse error at line (\d+):", case["libbam_stderr"])
        assert m and got["refused"][0] == int(m.group(1)), (got["refused"], case["libbam_stderr"])
        return
    if got["refused"] is not None:
        assert case.get("made_up") in STRICTER, got["refused"]
        front = b"".join(got["records"])
        assert bytes.fromhex(case["stream_hex"]).startswith(front) and len(front) > 0
        return
    recs = b"".join(got["records"])
    assert got["header"] == s2b.header(case["header_text"].encode("latin-1"))
    assert (len(got["records"]), len(recs)) == (case["records"], case["bytes"])
    assert hashlib.sha256(recs).hexdigest() == case["sha256"]
    if "stream_hex" in case:
        assert recs.hex() == case["stream_hex"]


def test_every_made_up_case_is_recorded_and_the_refused_ones_fail_in_libbam_or_are_known_to_be_stricter():
    recorded = {c["made_up"]: c for c in CASES if "made_up" in c}
    assert set(recorded) == set(pb_bam_gen.cases())
    for name, c in recorded.items():
        if name.startswith("refused_"):
            assert c["libbam_exit"] == -6 or name in STRICTER, name
        else:
            assert c["libbam_exit"] == 0, name


@pytest.mark.parametrize("name", sorted(pb_bam_gen.cases()))
def test_made_up_sam_text_is_what_the_pre_barcodes_oracle_prints(name):
    # (the GPU tests build their expectation as sam2bam(pre_barcodes_oracle(...)): both halves against the recorded runs)
    files, args, _ = pb_bam_gen.cases()[name]
    case = next(c for c in CASES if c.get("made_up") == name)
    want = pbo.run_pre_barcodes(args, lambda n: files[n])
    assert want["exit"] == case["exit"]
    assert want["stdout"] == case["sam"]


def test_second_mate_cell_barcode_is_glued_to_the_field_in_front():
    case = next(c for c in CASES if c.get("made_up") == "pairs_umi_cell_sample")
    recs = s2b.sam2bam(sam_of(case))["records"]
    first, second = recs[0], recs[1]
    assert b"CRZ" in first and b"CRZ" not in second and b"CYZ" in second
    assert re.search(rb"QXZ[^\0]* CR:Z:[ACGT]{8}\0CYZ", second)
    case = next(c for c in CASES if c.get("made_up") == "pairs_cell_only")
    second = s2b.sam2bam(sam_of(case))["records"][1]
    assert re.search(rb"opZ[^\0]* CR:Z:[ACGT]{8}\0CYZ", second) and b"CRZ" not in second


def test_header_of_an_argv_drops_the_last_word():
    h = s2b.header_for_argv("bin/fastq_pre_barcodes", ["--read1", "a.fq", "--bam", "--outfile1", "-"])
    text = b"@HD\tVN:1.0 SO:unknown\n@PG\tID:1 PN:fastq_pre_barcodes CL:bin/fastq_pre_barcodes --read1 a.fq --bam --outfile1\n"
    assert h == b"BAM\1" + len(text).to_bytes(4, "little") + text + b"\0\0\0\0"
