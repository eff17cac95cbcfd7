"""The geometry of the read-name table built part by part (fastq_utils_amd/csrc/fqg_names_build_plan.h) on the CPU:
tests/cxx/names_build_plan_check.cpp includes the header names_build follows and holds build_plan against a table worked
out by hand - which table sizes get parts of 2^12 or 2^13 slots behind one or two levels of buckets, which get none, what a
forced part size does -, against bits0 + bits1 + part_log == k for every k in 10..34, against the size gate at its edge
for an empty and a filled index in every mode, and against one bucket size.  Built twice: plain, and with the
undefined-behaviour sanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "names_build_plan_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_build_plan_follows_the_rules(tmp_path, flags):
    exe = str(tmp_path / "names_build_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    assert st["fails"] == 0 and st["rows"] == 11 and st["swept"] == 25 * 3 * 2 and st["gates"] == 4
    assert 0 < st["applied"] < st["swept"]
