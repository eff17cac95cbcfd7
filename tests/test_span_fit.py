"""The rule that says whether a tile's span fits its LDS input area (span_units / span_fits,
fastq_utils_amd/csrc/fqg_fastq_tile.h) on the CPU: tests/cxx/span_fit_check.cpp includes the header the kernels compile - the
flag kernels and the emit kernels that land what the rule counts all call it - and checks it against a restatement in
bytes for every skew, every in_cap that is a multiple of 16 from 48 to 4096 and the span lengths at the rule's edges;
where the rule says "fits", 16 * units <= in_cap - 32 (no store at or past in_cap); for two and three files numbered
through, the running total refuses exactly when the restated sum does.  Built twice: plain, and with the
undefined-behaviour sanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "span_fit_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_span_fit_rule(tmp_path, flags):
    exe = str(tmp_path / "span_fit_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    # 254 values of in_cap x 16 skews x (5 + up to 81 lengths); a check that never refuses proves nothing
    assert st["fits"] + st["refused"] > 300000
    assert st["fits"] > 1000 and st["refused"] > 1000
    assert st["multi_fits"] > 1000 and st["multi_refused"] > 1000
