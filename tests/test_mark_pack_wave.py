"""The mark pack of a whole wavefront on the matrix pipe (pack_marks32_wave, fastq_utils_amd/csrc/fqg_mark_pack.h) on the CPU:
tests/cxx/mark_pack_wave_check.cpp includes the header the kernel compiles, runs the host form - the MFMA restated with its
lane layout, the same weight table and the same joins - and compares every lane with pack_marks32: all and none set, every
single mark position of every lane with the other 63 lanes all-ones and again all-zero, and 100 000 random wavefronts.
Built twice: plain, and with the undefined-behaviour sanitizer (the results of the MFMA are signed; the joins must shift
them as unsigned words).  Whether the instruction has this layout on the device is tests/test_gpu_stream_pack_lanes.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "mark_pack_wave_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_pack_marks32_wave_is_pack_marks32_per_lane(tmp_path, flags):
    exe = str(tmp_path / "mark_pack_wave_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    assert st["single"] == 2 * 64 * 32
    assert st["random"] >= 100000 and st["cases"] == 2 + st["single"] + st["random"]
