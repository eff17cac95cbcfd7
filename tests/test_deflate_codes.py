"""The code construction of the device deflate compressor (fastq_utils_amd/csrc/fqg_deflate_codes.h) on the CPU:
tests/cxx/deflate_codes_check.cpp includes the header the kernel compiles and checks, on one-symbol, two-symbol, equal,
Fibonacci-weighted and 2 000 random tables of counts, that no length passes its limit (15 bits; 7 for the code-length
code), that the code is complete, that at least two symbols have a code, and that the run-length coded header decodes
back to the same lengths.  Built twice: plain, and with the undefined-behaviour sanitizer.

tests/cxx/deflate_model.cpp restates the kernel's decisions around the same header as one byte loop (the bytes the device
must write: tests/test_gpu_deflate.py compares them); here zlib inflates what it writes, member by member - the eight
plain texts, and every text of tests/deflgen.py, whose families must also be what they say: the model's report shows the
property each generator states."""
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


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """(the model under the undefined-behaviour sanitizer, the families of tests/deflgen.py, their check)"""
    from tests import deflgen
    model = deflgen.Model(tmp_path_factory.mktemp("deflate_model"), deflgen.UBSAN)
    return (model,) + deflgen.families(model)


def test_the_families_are_what_they_say(generated):
    _, fam, check = generated
    check()
    assert {"tie", "parse_geometry", "same_slot", "window", "wide_tokens", "member_cycle"} < set(fam)
    wide = fam["wide_tokens"].reports[0][0]
    print("wide tokens: widest %d bits, %d tokens with a third word (gzip), %d (BGZF)" % (wide["widest"], wide["three_word_gzip"], wide["three_word_bgzf"]))


def test_zlib_inflates_every_generated_text(generated):
    import zlib

    from tests import deflgen
    _, fam, _ = generated
    for name, f in fam.items():
        for k, (text, gz, reports) in enumerate(zip(f.texts, f.gz, f.reports)):
            members = deflgen.split_members(gz, reports)
            assert len(members) == max(1, -(-len(text) // deflgen.M)), (name, k)
            for i, m in enumerate(members):
                cut = text[i * deflgen.M:(i + 1) * deflgen.M]
                d = zlib.decompressobj(31)
                assert d.decompress(m) == cut and d.eof and not d.unused_data and len(m) <= len(cut) + 23, (name, k, i)
                assert reports[i]["n"] == len(cut)
                assert reports[i]["written"] == ("dynamic" if reports[i]["dyn_bytes"] <= reports[i]["stored_bytes"] else "stored")
            # the same members behind BGZF's header, as tests/test_gpu_bgzf.py expects them
            raw = f.bgzf(k)
            d = zlib.decompressobj(31)
            got = d.decompress(raw)
            while d.unused_data:
                rest, d = d.unused_data, zlib.decompressobj(31)
                got += d.decompress(rest)
            assert got == text and raw.endswith(deflgen.BGZF_EOF), (name, k)


def test_the_report_changes_nothing(generated, tmp_path):
    """the same bytes with and without --report, one text per process and many"""
    model, fam, _ = generated
    f = fam["parse_geometry"]
    assert model.run(f.texts, report=False)[0] == f.gz
    for k in (0, len(f.texts) - 1):
        (tmp_path / "in").write_bytes(f.texts[k])
        subprocess.run([model.exe, str(tmp_path / "in"), str(tmp_path / "out.gz")], check=True, capture_output=True, timeout=120)
        assert (tmp_path / "out.gz").read_bytes() == f.gz[k]
