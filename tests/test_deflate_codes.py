"""The code construction of the device deflate compressor (fastq_utils_amd/csrc/fqg_deflate_codes.h) on the CPU:
tests/cxx/deflate_codes_check.cpp includes the header the kernel compiles and checks, on one-symbol, two-symbol, equal,
Fibonacci-weighted and 2 000 random tables of counts, that no length passes its limit (15 bits; 7 for the code-length
code), that the code is complete, that at least two symbols have a code, and that the run-length coded header decodes
back to the same lengths.  Built twice: plain, and with the undefined-behaviour sanitizer.

tests/cxx/deflate_model.cpp restates the kernel's decisions around the same header as one byte loop (the bytes the device
must write: tests/test_gpu_deflate.py compares them); here zlib inflates what it writes, member by member."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "deflate_codes_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_codes_and_header(tmp_path, flags):
    exe = str(tmp_path / "deflate_codes_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    st = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", p.stdout)}
    assert st["failures"] == 0
    assert st["tables"] == 2007                       # 4 one-symbol, two symbols, all equal, Fibonacci, 2 000 random
    assert st["limited15"] > 0 and st["limited7"] > 0  # both limits were met
    assert st["symbols"] == 256 + 32768               # every match length and every distance


def test_sequential_model_of_the_kernel_inflates(tmp_path):
    import random
    import zlib

    from tests.test_pgzip import fastq_text

    exe = str(tmp_path / "deflate_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "cxx", "deflate_model.cpp"), "-lz"], check=True)
    r = random.Random(3)
    M = 65280
    fastq = fastq_text(700, 1)
    words = b"".join(r.choice([b"the ", b"quick ", b"brown ", b"fox\n", b"jumps ", b"over "]) for _ in range(20000))
    for name, data in (("empty", b""), ("one", b"@"), ("fastq", fastq[:2 * M + 7]), ("words", words[:M + 1]), ("zeros", bytes(M + 300)),
                       ("noise", r.randbytes(M - 1)), ("period_32768", (r.randbytes(32768) * 2)[:M]),
                       ("period_32769", (r.randbytes(32769) * 2)[:M])):
        (tmp_path / "in").write_bytes(data)
        subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "out.gz")], check=True, capture_output=True, timeout=120)
        gz, at, n = (tmp_path / "out.gz").read_bytes(), 0, 0
        while gz:
            d = zlib.decompressobj(31)
            text = d.decompress(gz)
            assert d.eof and text == data[at:at + M] and len(gz) - len(d.unused_data) <= len(text) + 23, (name, n)
            at, n, gz = at + len(text), n + 1, d.unused_data
        assert at == len(data) and n == max(1, -(-len(data) // M)), name
