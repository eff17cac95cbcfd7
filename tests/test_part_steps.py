"""The steps of the line workers in the parted streaming pass (fastq_utils_amd/csrc/fqg_part_steps.h) on the CPU:
tests/cxx/part_steps_check.cpp includes the header the kernel compiles and chains its decision over every sequence of one
to four parts with densities from {20, 31.9, 32, 45, 60, 60.1, 90} newlines per chunk and parts of 1, 13, 4096 and 5000
chunks: the steps done are contiguous from step 0, lines_done_steps is their end, the parts that run are the in-range ones
in front of the first that is not, and images in range throughout get the ranges the kernel gave them before.  The rule the
kernel had before, restated there, must leave gaps on some sequences (old_gaps).  Built twice: plain, and with the
undefined-behaviour sanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "part_steps_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_done_steps_are_contiguous(tmp_path, flags):
    exe = str(tmp_path / "part_steps_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    n_seq = sum(28 ** n for n in range(1, 5))  # 7 densities x 4 sizes a part
    assert st["cases"] == 2 * n_seq - st["skipped"] and n_seq - st["skipped"] > 100000
    assert st["in_range"] + st["declined"] == st["cases"]
    assert st["in_range"] > 1000 and st["declined"] > 1000 and st["odd"] > st["cases"]
    assert st["old_gaps"] > 1000, "the check does not see the gap it is there for"
