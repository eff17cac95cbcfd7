"""The record index of fqg_bam_index_device (fastq_utils_amd/csrc/fqg_bam_index_core.h) on the CPU.

tests/cxx/bam_index_model.cpp includes the header the kernels compile and runs it as they do - windows, segments resolved
backwards in rounds of thirty-six positions, the ring of the last positions, the follower, the stretches - with every
buffer allocated to its exact size.  Built three times (plain, undefined-behaviour sanitizer, address sanitizer:
stand-alone programs, nothing is preloaded), it must give the loop of fqg_bam_index_records - n, used and every offset -
on every stream of tests/bamidx_gen.py - the synthetic shapes and the real files: the inflated stream of every .bam under
tests/golden, whole, and bamgen.config4 - at segments of 64, 128 and 4096 bytes in windows of two and of five segments, with
a ring so small that every record of 64 bytes or more is a hop and with the default one.  The bounds of the core are
established here, before a stream is handed to a GPU."""
import os
import subprocess

import pytest

from tests import bamidx_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "bam_index_model.cpp")
BUILDS = {"plain": ["-O2"], "ubsan": ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"],
          "asan": ["-O1", "-g", "-fsanitize=address"]}
GEOMETRY = [(seg, k * seg) for seg in (64, 128, 4096) for k in (2, 5)]


@pytest.fixture(scope="module", params=list(BUILDS))
def model(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_index_model") / ("bam_index_model_" + request.param))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + BUILDS[request.param] + ["-o", exe, SRC], check=True)
    return exe


def run(model, tmp_path, cases, seg, window, ring):
    (tmp_path / "pack").write_bytes(bamidx_gen.pack(cases))
    p = subprocess.run([model, str(tmp_path / "pack"), str(tmp_path / "out"), str(seg), str(window), str(ring)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and p.stdout == "streams %d\n" % len(cases), (p.returncode, p.stdout[-300:], p.stderr[-3000:])
    return bamidx_gen.unpack((tmp_path / "out").read_bytes(), len(cases))


def check(model, tmp_path, cases, seg, window, ring):
    got = run(model, tmp_path, cases, seg, window, ring)
    for (name, stream, first), (offs, used) in zip(cases, got):
        want = bamidx_gen.walk(stream, first)
        assert (len(offs), used) == (len(want[0]), want[1]), (name, seg, window, ring)
        assert offs == want[0], (name, seg, window, ring)


@pytest.mark.parametrize("seg,window", GEOMETRY)
def test_every_stream_of_the_generator(model, tmp_path, seg, window):
    cases = bamidx_gen.streams(seg, window)
    for ring in (128, 8192):
        check(model, tmp_path, cases, seg, window, ring)


@pytest.fixture(scope="module")
def real_files():
    return bamidx_gen.real_files()


@pytest.mark.parametrize("seg,window", GEOMETRY)
def test_real_files(model, tmp_path, real_files, seg, window):
    """every golden stream, uncut (27 MB in all, a --tx header of more than a megabyte among them), at every geometry,
    both rings, all three builds"""
    for ring in (128, 8192):
        check(model, tmp_path, real_files, seg, window, ring)


def test_the_generator_is_what_it_says():
    cases = {name: (s, first) for name, s, first in bamidx_gen.streams(64, 128)}
    assert len(bamidx_gen.walk(*cases["minimal-200"])[0]) == 200
    assert bamidx_gen.walk(*cases["no-records"]) == ([], 12) and bamidx_gen.walk(*cases["first-at-the-end"]) == ([], 52)
    assert bamidx_gen.walk(*cases["stop-31-at-1"])[0] == [12] and len(bamidx_gen.walk(*cases["stop-max-at-8"])[0]) == 8
    assert [len(bamidx_gen.walk(*cases["cut-%d" % c])[0]) for c in (1, 40)] == [8, 8]
    for d in range(4):  # the field straddles (or touches) the seam at 12 + 2 * 64
        offs = bamidx_gen.walk(*cases["seg-field-%d-before-seam" % d])[0]
        assert offs[1] == 12 + 128 - d and len(offs) == 6
    for r in range(36):
        assert bamidx_gen.walk(*cases["seg-entry-at-%d" % r])[0][1] == 12 + 64 + r
    s, first = cases["decoys-2"]
    starts = sum(1 for q in range(first, len(s)) if bamidx_gen.walk(s, q)[0])
    assert starts > 0.2 * (len(s) - first) and len(bamidx_gen.walk(s, first)[0]) == 7  # (a body has ONE alignment: a quarter)
    assert max(len(bamidx_gen.walk(s, q)[0]) for q in range(first, len(s))) > 10  # ... and decoys chain to decoys
    assert len(bamidx_gen.walk(*cases["stream-inside-a-record-1"])[0]) == 4


def test_library_walk_agrees_with_the_restatement():
    """fqg_bam_index_records itself (no GPU needed) against the ten lines every other comparison uses"""
    import ctypes as C

    import fastq_utils_amd as fq

    L = fq.abi.load()
    for name, stream, first in bamidx_gen.streams(128, 256):
        if name == "first-at-the-end" or name.endswith("from-inside"):  # (the two kinds that do not start behind the header)
            continue
        n, used = C.c_uint64(), C.c_uint64()
        want = bamidx_gen.walk(stream, first)
        offs = (C.c_uint64 * max(1, len(want[0])))()
        assert L.fqg_bam_index_records(stream, len(stream), offs, len(want[0]), C.byref(n), C.byref(used)) == 0, name
        assert (n.value, used.value, list(offs)[:n.value]) == (len(want[0]), want[1], want[0]), name
