"""The Python statement of fastq_split_interleaved (tests/split_interleaved_oracle.py) against every golden invocation
of the reference program (tests/golden/split_interleaved.json, tools/gen_golden.py).  No GPU."""
import hashlib
import json
import os

import pytest

from tests import split_gen, split_interleaved_oracle as so
from tests.util import GOLD, strip_progress

GOLDEN = json.load(open(os.path.join(GOLD, "split_interleaved.json")))
BIG = {}


def big(name):
    if not BIG:
        BIG.update(split_gen.big_files())
    return BIG[name]


@pytest.mark.parametrize("i", range(len(GOLDEN)), ids=[" ".join(c["args"])[-60:] or "(no arguments)" for c in GOLDEN])
def test_oracle_matches_the_reference(i):
    case = GOLDEN[i]
    args = [a.replace("GEN/", "SCRATCH/") if a.startswith("GEN/") else ("o" if a == "OUT" else a) for a in case["args"]]
    image = big(case["args"][0][4:]) if case["args"] and case["args"][0].startswith("GEN/") else None
    got = so.run(args, GOLD, image)
    assert got["exit"] == case["exit"]
    assert got["stdout"] == case["stdout"]
    assert strip_progress(got["stderr"]) == strip_progress(case["stderr"])
    assert sorted(got["files"]) == sorted(case["files"])
    for name, want in case["files"].items():
        if want is None:
            continue
        text = got["files"][name]
        assert (len(text), hashlib.sha256(text).hexdigest()) == (want["bytes"], want["sha256"])
        if "content" in want:
            assert text.decode("latin-1") == want["content"]


def test_the_seeded_inputs_cover_what_they_are_for():
    by_input = {c["args"][0]: c for c in GOLDEN if len(c["args"]) == 2 and c["args"][1] == "OUT"}
    want = {"clean_casava": 0, "clean_slash": 0, "clean_nosuffix": 0, "mismatch_pair0": 3, "mismatch_mid": 3, "invalid_m1": 3,
            "invalid_m2": 3, "odd": 3, "no_final_newline": 0, "empty": 0, "nul_in_header": 0, "nul_in_sequence": 3, "mates_26_150": 0}
    want.update({"trunc_m%d_l%d" % (m, k): 1 for m in (1, 2) for k in (1, 2, 3)})
    for name, status in want.items():
        assert by_input["data/syn_split_%s.fastq.gz" % name]["exit"] == status, name
    assert by_input["GEN/big_clean.fastq"]["exit"] == 0 and by_input["GEN/big_mismatch.fastq"]["exit"] == 3
    assert by_input["GEN/big_trunc.fastq"]["exit"] == 1
    assert 5 << 19 < len(big("big_clean.fastq")) < 4 << 20  # about 3 MiB
