"""The 32-bit mark pack of the streaming pass (fastq_utils_amd/csrc/fqg_mark_pack.h) on the CPU: tests/cxx/mark_pack_check.cpp
includes the header the kernel compiles and compares pack_marks32 with the form it replaced (two pack_marks16 halves
joined with a shift) and with a byte loop, on every single mark position, every pair of positions, all and none set, and
200 000 random patterns.  Built twice: plain, and with the undefined-behaviour sanitizer (the join shifts marks out of
the top of a word, which must be all it leans on)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "mark_pack_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_pack_marks32_is_the_old_form(tmp_path, flags):
    exe = str(tmp_path / "mark_pack_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    assert st["single"] == 32 and st["pair"] == 496
    assert st["random"] >= 100000 and st["cases"] == 2 + 32 + 496 + st["random"]
