"""The decoder core of the device inflater (fastq_utils_amd/csrc/fqg_inflate_core.h) on the CPU.

tests/cxx/inflate_model.cpp includes the header the kernel compiles and runs it as the kernel does - the payload staged
in windows, rounds of the one walking lane, tables filled and matches copied in between - with every buffer allocated to
its exact size.  Built three times (plain, undefined-behaviour sanitizer, address sanitizer: stand-alone programs, nothing
is preloaded), it inflates every file of tests/bgzfgen.py, the damaged ones included; verdicts, first refused block, first
CRC mismatch and the bytes of every good block must be zlib's, and the reason a hand-made damaged block is refused for
is the one bgzfgen.REASONS keeps.  The bounds of the core are established here, before a damaged payload is ever handed
to a GPU.  The same three programs read what the project's own compressor writes (tests/cxx/deflate_model.cpp, which is
the device compressor byte for byte: tests/test_gpu_deflate.py), framed as BGZF."""
import os
import re
import subprocess
import zlib

import pytest

from tests import bgzfgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "inflate_model.cpp")
BUILDS = {"plain": ["-O2"], "ubsan": ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"],
          "asan": ["-O1", "-g", "-fsanitize=address"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def model(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_model") / ("inflate_model_" + request.param))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + BUILDS[request.param] + ["-o", exe, SRC], check=True)
    return exe


def run(model, tmp_path, raw, stage=None):
    (tmp_path / "in").write_bytes(raw)
    p = subprocess.run([model, str(tmp_path / "in"), str(tmp_path / "out")] + ([str(stage)] if stage else []), capture_output=True,
                       text=True, timeout=120)
    return p


def check(model, tmp_path, name, raw, stage=None, reason=None):
    want = bgzfgen.verdict(raw)
    p = run(model, tmp_path, raw, stage)
    assert p.returncode == 0, (name, p.returncode, p.stdout[-300:], p.stderr[-2000:])
    blocks = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"block (\d+) status (\d+) crc (\d)", p.stdout)]
    m = re.search(r"blocks (\d+) out_bytes (\d+) raw_bytes (\d+) bad (-?\d+) crc (-?\d+)", p.stdout)
    n_blocks, out_bytes, raw_bytes, bad, crc = map(int, m.groups())
    assert (n_blocks, out_bytes, raw_bytes) == (want["n_blocks"], want["out_bytes"], want["raw_bytes"]), name
    assert [b[1] == 0 for b in blocks] == want["good"], name
    assert bad == (-1 if want["bad_block"] == bgzfgen.NONE else want["bad_block"]), name
    assert crc == (-1 if want["crc_block"] == bgzfgen.NONE else want["crc_block"]), name
    assert reason is None or blocks[bad][1] == reason, (name, blocks[bad], reason)
    out, at = (tmp_path / "out").read_bytes(), 0
    assert len(out) == out_bytes, name
    for text, (_, _, isize) in zip(want["texts"], bgzfgen.walk(raw)[0]):
        assert text is None or out[at:at + isize] == text, name
        at += isize
    return want


def test_well_formed_files(model, tmp_path):
    for name, raw in bgzfgen.well_formed().items():
        want = check(model, tmp_path, name, raw)
        assert want["bad_block"] == want["crc_block"] == bgzfgen.NONE, name


def test_small_staging_windows(model, tmp_path):
    # the smallest window the model takes: every file meets the window's end many times
    W = bgzfgen.well_formed()
    for name in ("fastq-l6", "noise-l0", "noise-huffman", "fastq-mem1", "bam-flushes", "period-by-hand", "65-blocks",
                 "stored-at-the-window-edge", "payload-alignment", "match-geometry"):
        check(model, tmp_path, name, W[name], stage=2048)


def test_many_small_blocks(model, tmp_path):
    check(model, tmp_path, "many", bgzfgen.many_blocks(1500))


def test_malformed_frames(model, tmp_path):
    for name, raw in bgzfgen.malformed_frames().items():
        assert bgzfgen.verdict(raw) is None, name
        p = run(model, tmp_path, raw)
        assert p.returncode == 3 and p.stdout == "frame refused\n", (name, p.stdout[-200:], p.stderr[-2000:])


def test_damaged_payloads(model, tmp_path):
    refused = accepted = 0
    for name, raw in bgzfgen.damaged().items():
        want = check(model, tmp_path, name, raw, reason=bgzfgen.reason(name))
        refused += want["bad_block"] != bgzfgen.NONE
        accepted += want["bad_block"] == bgzfgen.NONE
        assert bgzfgen.reason(name) is None or want["bad_block"] != bgzfgen.NONE, name
        for stage in (2048,):
            check(model, tmp_path, name, raw, stage, bgzfgen.reason(name))
    assert refused >= 10 and accepted >= 5, (refused, accepted)   # (a generator change must not quietly empty one side)
    assert set(bgzfgen.REASONS) <= set(bgzfgen.damaged())


def test_the_sweeps_are_what_they_say(model, tmp_path):
    D = bgzfgen.damaged()
    cuts, crcs = bgzfgen.sweeps()
    assert len(cuts) == 48 and len(crcs) == 10
    for name in cuts:
        assert bgzfgen.verdict(D[name])["bad_block"] == 1 and bgzfgen.reason(name) == 38, name
    for name, (raw, at) in bgzfgen.sizes_wrong_crc().items():
        want = bgzfgen.verdict(raw)
        assert (want["bad_block"], want["crc_block"]) == (bgzfgen.NONE, at) and D[name] == raw, name


@pytest.fixture(scope="module")
def own_files(tmp_path_factory):
    """name -> the BGZF file of what the project's compressor makes of the contents of tests/test_fastdeflate.py"""
    from tests.test_fastdeflate import contents
    tmp = tmp_path_factory.mktemp("deflate_model")
    exe = str(tmp / "deflate_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cxx", "deflate_model.cpp"), "-lz"], check=True)
    files = {}
    for name, data in contents():
        data = data[:2 * 65280 + 7]
        (tmp / "in").write_bytes(data)
        subprocess.run([exe, str(tmp / "in"), str(tmp / "out.gz")], check=True, capture_output=True, timeout=120)
        gz, blocks, texts = (tmp / "out.gz").read_bytes(), [], []
        while gz:   # cut into members; behind its ten header bytes a member is the BGZF block's payload and trailer
            d = zlib.decompressobj(31)
            texts.append(d.decompress(gz))
            assert d.eof
            size = len(gz) - len(d.unused_data)
            blocks.append(bgzfgen.block(gz[10:size - 8], len(texts[-1]), int.from_bytes(gz[size - 8:size - 4], "little")))
            gz = d.unused_data
        assert b"".join(texts) == data and len(blocks) == max(1, -(-len(data) // 65280))
        files[name] = b"".join(blocks) + bgzfgen.EOF
    return files


def test_blocks_of_the_projects_compressor(model, tmp_path, own_files):
    assert len(own_files) == 14
    for name, raw in own_files.items():
        want = check(model, tmp_path, name, raw)
        assert want["bad_block"] == want["crc_block"] == bgzfgen.NONE, name
        check(model, tmp_path, name, raw, stage=2048)
