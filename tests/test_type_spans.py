"""The span form of the line-type masks of the streaming pass (fastq_utils_amd/csrc/fqg_type_spans.h) on the CPU:
tests/cxx/type_spans_check.cpp includes the header the kernel compiles and compares it with the form it replaced (two
prefix-XORs over the shifted newline mask, newline bytes taken out by the caller) and with a byte-by-byte count, on
every 32-bit mask with at most three bits set and all four types of the first byte; its return value must tell exactly
the masks with four or more bits.  Built twice: plain, and with the undefined-behaviour sanitizer (the form leans on
unsigned wrap-around, which must be all it leans on)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "type_spans_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_span_form_is_the_old_form(tmp_path, flags):
    exe = str(tmp_path / "type_spans_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    assert st["exact_enumerated"] == 21956          # (1 + 32 + 496 + 4 960) masks x 4 types
    assert st["over_enumerated"] == 35960           # every mask with exactly four bits
    assert st["random_dense"] >= 5000 and st["over"] == st["over_enumerated"] + st["random_dense"]
