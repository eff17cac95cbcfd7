"""GzipMembers::write_members (fastq_utils_amd/host/fq_parallel.h): members a context thread had the device compressor
make, unit by unit with the carry chain, and the tail of the last unit the writer took through close().  CPU only: a
fake GzipDevice cuts at FQG_GZ_MEMBER_TEXT bytes and compresses with zlib (tests/cxx/gzip_members_chain_check.cpp, which
checks the file itself and is built once more with AddressSanitizer and UBSan)."""
import gzip
import os
import subprocess
import zlib

import pytest

from tests.util import REPO

SRC = os.path.join(REPO, "tests", "cxx", "gzip_members_chain_check.cpp")
M = 65280  # FQG_GZ_MEMBER_TEXT
UNITS = [0, 1, M - 1, M, 3 * M + 5]
# (units, how many of them the writer takes; -1: all)
RUNS = {
    "in_order": (UNITS, -1),
    "reversed": (UNITS[::-1], -1),
    "small_between_large": ([3 * M + 5, 1, 0, M, 1, M - 1, 0, M - 1, 3 * M + 5, M], -1),
    "tails_that_add_up_to_a_member": ([M - 1, 1, M - 1, M - 1, 1, 1], -1),
    "many_tiny_units": ([1] * 40 + [M - 1] + [1] * 3, -1),
    "one_exact_member": ([M], -1),
    "only_empty_units": ([0, 0, 0], -1),
    "no_units": ([], -1),
    "writer_stops_after_three": ([M - 1, 3 * M + 5, 1, M, 3 * M + 5, 0, 1], 3),
    "writer_stops_behind_an_empty_unit": ([3 * M + 5, 0, M - 1, M], 2),
    "writer_takes_nothing": ([3 * M + 5, M], 0),
}


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain") / ("gzip_members_chain_check_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + ["-o", exe, SRC, "-lz"], check=True)
    return exe


@pytest.mark.parametrize("name", sorted(RUNS))
def test_the_file_is_the_text_taken_cut_as_one_call_cuts_it(driver, tmp_path, name):
    units, taken = RUNS[name]
    gz, txt = tmp_path / "out.gz", tmp_path / "taken.txt"
    p = subprocess.run([driver, str(gz), str(txt), str(taken)] + [str(n) for n in units], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode("latin-1")[-2000:])
    raw, text = gz.read_bytes(), txt.read_bytes()
    assert len(text) == sum(units if taken < 0 else units[:taken])
    assert gzip.decompress(raw) == text
    cut, rest = [], raw
    while rest:
        d = zlib.decompressobj(31)
        cut.append(len(d.decompress(rest)))
        assert d.eof
        rest = d.unused_data
    assert cut == [M] * (len(text) // M) + ([len(text) % M] if len(text) % M or not text else [])
    if not text:
        assert cut == [0]  # an empty gzip stream is still a gzip stream: one member of empty content
