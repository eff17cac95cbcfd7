"""The window of a step of the line kernel without a search (fastq_utils_amd/csrc/fqg_line_window.h) on the CPU:
tests/cxx/line_window_check.cpp includes the header the kernel compiles and compares the integer window start with the
double-precision formula the kernel had before over 28 .. 64 newlines per chunk in steps of 1/8, images of 257 and 4096
chunks (every step) and of 8.5 M chunks (10 000 spread steps): equal or one chunk earlier, never later.  Built twice:
plain, and with the address and undefined-behaviour sanitizers (a stand-alone program; nothing Python loads)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "line_window_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_integer_window_start_is_the_double_one_or_one_less(tmp_path, flags):
    exe = str(tmp_path / "line_window_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    n_dens = (64 - 28) * 8 + 1
    assert st["cases"] > n_dens * (10_000 + 257 * 28 // 512 + 4096 * 28 // 512)
    assert st["equal"] + st["one_less"] == st["cases"]
    # the bias is 2^-16 of a chunk: the integer start is the earlier one only where the estimate lies that close above a
    # whole chunk (and where the fraction's rounding reaches it) - a few per thousand steps, not none
    assert 0 < st["one_less"] < st["cases"] // 50, st
    assert st["clamped"] > 0, "no step whose window is held at the end of the chunk table"
