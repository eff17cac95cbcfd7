"""fqg_deflate / fqg_text_deflate / fqg_deflate_output (gzip members compressed on the device) through abi.py.  Python's
zlib reads every member by itself: it must end where the next one starts, hold exactly its cut of the text (zlib checks
the CRC-32 and ISIZE of the trailer while it does; ISIZE is compared once more here), and be no larger than its text +
23 bytes.  The members of a text do not depend on where the text lies or on how it was cut into calls.

They are byte for byte what tests/cxx/deflate_model.cpp, the kernel's decisions in one byte loop, writes for the same
text: on eight plain texts, and on the families of tests/deflgen.py, each made to reach one thing the workgroup adds to
the model - every member size, both sides of stored | dynamic, matches at the edges of the parse's windows and steps,
hash slots that many positions of a step share, the window's edge, tokens that need a third word, every alignment of a
device source against every carry, and more members than workgroups, so that a workgroup's LDS goes from one member to
the next and the gather reads behind its first span of offsets."""
import ctypes as C
import random
import time
import zlib

import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import b2f_gen, deflgen, split_gen
from tests.test_fastdeflate import contents
from tests.test_pgzip import fastq_text

pytestmark = pytest.mark.gpu
A = fq.abi
M = A.GZ_MEMBER_TEXT
ERR_ARG = -3  # FQG_ERR_ARG, include/fqg.h


@pytest.fixture(scope="module")
def ctx():
    c = fq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def named():
    """the contents of tests/test_fastdeflate.py, cut to what a few members need"""
    keep = {"text": 3 * M + 7, "zeros": 3 * M + 7, "runs": 3 * M + 7, "two_symbols": 2 * M, "skewed": 2 * M, "noise": 2 * M + 100}
    return {name: data[:keep[name]] for name, data in contents() if name in keep}


@pytest.fixture(scope="module")
def fastq():
    return fastq_text(1500, 1)


@pytest.fixture(scope="module")
def model():
    """tests/cxx/deflate_model.cpp, built once (tests/test_gpu_bgzf.py shares it)"""
    return deflgen.shared()[0]


@pytest.fixture(scope="module")
def families():
    return deflgen.shared()[1]


def members_of(gz):
    """[(member bytes, its text)] of a run of gzip members, each inflated by itself"""
    out = []
    while gz:
        d = zlib.decompressobj(31)
        text = d.decompress(gz)
        assert d.eof, "a member that does not end"
        size = len(gz) - len(d.unused_data)
        out.append((gz[:size], text))
        gz = d.unused_data
    return out


def zlib_members(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """bytes zlib needs for the same cuts, as gzip members"""
    total = 0
    for o in range(0, max(len(data), 1), M):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
        total += len(c.compress(data[o:o + M]) + c.flush())
    return total


def check(ctx, label, data, **how):
    r = ctx.deflate(data, **how)
    assert r["text_bytes"] == len(data) and r["tail_bytes"] == 0 and r["tail"] == b"", label
    assert r["gz_bytes"] == len(r["members"]), label
    ms = members_of(r["members"])
    assert len(ms) == r["n_members"] == max(1, -(-len(data) // M)), (label, len(ms))
    for i, (raw, text) in enumerate(ms):
        assert text == data[i * M:(i + 1) * M], (label, i)
        assert int.from_bytes(raw[-4:], "little") == len(text), (label, i)
        assert raw[:4] == b"\x1f\x8b\x08\x00" and len(raw) <= len(text) + 23, (label, i, len(raw))
    z1 = zlib_members(data, 1)
    print("%-22s %8d -> %8d bytes, %.3f of the input, %.3f of zlib level 1" %
          (label, len(data), len(r["members"]), len(r["members"]) / max(1, len(data)), len(r["members"]) / z1))
    return r["members"]


@pytest.mark.parametrize("n", [0, 1, 7, M - 1, M, M + 1, 3 * M + 7], ids=lambda n: "bytes_%d" % n)
def test_sizes(ctx, fastq, n):
    check(ctx, "fastq[:%d]" % n, fastq[:n])


@pytest.mark.parametrize("name", ["text", "zeros", "runs"])
def test_matches_are_found_and_coded(ctx, named, name):
    gz = check(ctx, name, named[name])
    assert len(gz) < zlib_members(named[name], 1, zlib.Z_HUFFMAN_ONLY), name


@pytest.mark.parametrize("name", ["two_symbols", "skewed"])
def test_codes(ctx, named, name):
    gz = check(ctx, name, named[name])
    assert len(gz) < len(named[name])


def test_noise_is_stored(ctx, named):
    gz = check(ctx, "noise", named["noise"])
    assert len(gz) <= len(named["noise"]) + 23 * 3


def test_fastq_compresses(ctx, fastq):
    gz = check(ctx, "fastq_text(1500, 1)", fastq)
    assert len(gz) < 0.6 * len(fastq)


def test_window(ctx):
    r = random.Random(11)
    at = (r.randbytes(32768) * 2)[:M]
    gz = check(ctx, "period_32768", at)
    # 32768 bytes of noise cannot shrink; the 32512 behind them are matches of up to 258 bytes at five bytes at most each,
    # with a few literals between them where a later position took the hash slot
    assert len(gz) < 0.75 * M
    beyond = (r.randbytes(32769) * 2)[:M]
    check(ctx, "period_32769", beyond)  # (zlib refuses a distance beyond the window)


def structure(seed):
    """tests/test_fastdeflate.py's test_random_structures, at 200 kB at most"""
    r = random.Random(seed)
    parts = []
    for _ in range(r.randrange(1, 12)):
        kind = r.randrange(5)
        n = r.choice([1, 7, 100, 5000, 90000])
        if kind == 0:
            parts.append(r.randbytes(n))
        elif kind == 1:
            parts.append(bytes([r.randrange(256)]) * n)
        elif kind == 2:
            parts.append((r.randbytes(r.randrange(1, 40)) * (n // 3 + 1))[:n])
        elif kind == 3:
            parts.append(fastq_text(n // 300 + 1, seed)[:n])
        else:
            parts.append(b"".join(parts)[-n:])
    return b"".join(parts)[:200000]


@pytest.mark.parametrize("seed", range(12))
def test_random_structures(ctx, seed):
    check(ctx, "structure_%d" % seed, structure(seed))


def test_bytes_of_the_sequential_model(ctx, model, named, fastq):
    """tests/cxx/deflate_model.cpp makes the kernel's decisions in one byte loop: the same bytes"""
    r = random.Random(11)
    cases = (("fastq", fastq[:2 * M + 7]), ("text", named["text"][:M + 1]), ("runs", named["runs"][:M]),
             ("skewed", named["skewed"][:M]), ("noise", named["noise"][:M]), ("period_32768", (r.randbytes(32768) * 2)[:M]),
             ("seven", b"ACGTACG"), ("empty", b""))
    for (name, data), want in zip(cases, model.run([data for _, data in cases], report=False)[0]):
        assert ctx.deflate(data)["members"] == want, name


FAMILIES = ["sizes_" + c for c in deflgen.SIZE_CONTENTS] + ["tie", "parse_geometry", "same_slot", "window", "wide_tokens", "member_cycle"]


@pytest.mark.parametrize("name", FAMILIES)
def test_generated_texts_are_the_models_bytes(ctx, families, name):
    """every text of a family of tests/deflgen.py, one call from host memory each"""
    f = families[name]
    for k, text in enumerate(f.texts):
        r = ctx.deflate(text)
        assert r["n_members"] == 1 and r["members"] == f.gz[k], (name, k, len(text), f.reports[k][0]["written"])


def test_every_alignment_of_a_device_source_behind_every_carry(ctx, model):
    """the first 16-byte word staged holds the source's skew and the carry's end, the last one the skew and the member's
    end; the source has sixteen bytes and more of the tensor on either side"""
    import torch
    texts = deflgen.alignment_texts()
    want = dict(zip(texts, model.run(list(texts.values()), report=False)[0]))
    t = torch.zeros(M + 700 + 64, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    for (c, n), text in texts.items():
        src = torch.frombuffer(bytearray(text[c:]), dtype=torch.uint8).cuda()
        for s in range(16):
            t.fill_(0xA5)
            t[16 + s:16 + s + n - c] = src
            torch.cuda.synchronize()
            for again in range(1 + (n > M)):
                r = ctx.deflate(t.data_ptr() + 16 + s, carry=text[:c], nbytes=n - c)
                assert r["n_members"] == -(-n // M) and r["members"] == want[c, n], (c, n, s, again)


def test_more_members_than_workgroups_and_than_a_span_of_offsets(ctx, model, families):
    """the member cycle of tests/deflgen.py from host memory: every workgroup compresses a third member and more, each
    unlike the one before it in everything the workgroup keeps in LDS; k_deflate_gather reads the second span's sum"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_members = max(2049 + 2, 2 * cus + 3)
    assert n_members >= 2049 + 2 and n_members > 2 * cus + 2
    f = families["member_cycle"]
    text, order, last = deflgen.cycle_text(f.texts, n_members)
    want = b"".join(f.gz[k] for k in order) + model.run([last], report=False)[0][0]
    for again in range(2):
        t0 = time.perf_counter()
        r = ctx.deflate(text)
        print("%d members, %d bytes of text: %.2f s" % (n_members, len(text), time.perf_counter() - t0))
        assert r["n_members"] == n_members and r["text_bytes"] == len(text)
        assert r["members"] == want, again


def test_members_depend_on_the_text_alone(ctx, fastq):
    import torch
    data = (fastq * (3 * M // len(fastq) + 2))[:3 * M + 7]
    one_call = check(ctx, "one call, host", data)
    # device memory, at an address that is no multiple of 16
    t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    t[5:5 + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    r = ctx.deflate(t.data_ptr() + 5, nbytes=len(data))
    assert r["members"] == one_call
    # cut into calls: what did not fill a member comes back as text and goes into the next call
    cuts = [0, 1, M - 1, M + 1, 2 * M + 5, len(data)]
    got, carry = [], b""
    for a, b in zip(cuts, cuts[1:]):
        r = ctx.deflate(data[a:b], carry=carry, final=b == len(data))
        assert r["text_bytes"] == len(carry) + b - a and r["tail_bytes"] == len(r["tail"]) < M
        assert r["tail"] == data[b - len(r["tail"]):b]
        got.append(r["members"])
        carry = r["tail"]
    assert carry == b"" and b"".join(got) == one_call
    assert ctx.deflate(data)["members"] == one_call and ctx.deflate(data)["members"] == one_call


def test_text_of_a_store(ctx):
    image = b"".join(split_gen.pairs(3, 700))
    st = A.probe_first_record(image[:4096], True)
    ctx.validate(image, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY | A.VALIDATE_NO_STATS | A.VALIDATE_INDEX)
    fr = ctx.retain_frame()
    sizes, texts = ctx.records_split(fr, 0, fr.n_records, want_output=True)
    assert min(sizes) > M
    for w in (0, 1):
        got = ctx.text_deflate(A.TEXT_RECORDS, 1 + w, final=False)
        assert got["text_bytes"] == sizes[w] and got["tail"] == texts[w][len(texts[w]) - got["tail_bytes"]:]
        want = ctx.deflate(texts[w], final=False)
        assert (got["members"], got["tail"]) == (want["members"], want["tail"])
        assert ctx.records_split_output(w, sizes[w]) == texts[w]  # the producer's store is only read
        carried = ctx.text_deflate(A.TEXT_RECORDS, 1 + w, carry=b"@carried\n")
        assert b"".join(t for _, t in members_of(carried["members"])) == b"@carried\n" + texts[w]
    fr.release()
    rng = np.random.default_rng(4)
    stream = b2f_gen.stream([b2f_gen.fastq2bam_record(rng, i, paired=i % 3 != 0, sample=True, long_read=45 + i % 11) for i in range(300)])
    r = ctx.bam2fastq(stream)
    assert r["code"] == 0 and all(r["out_bytes"])
    for s in range(6):
        got = ctx.text_deflate(A.TEXT_BAM2FASTQ, s)
        assert got["members"] == ctx.deflate(r["streams"][s])["members"], s
        assert b"".join(t for _, t in members_of(got["members"])) == r["streams"][s]


def test_argument_errors(ctx):
    L = A.load()
    r = A.DeflateResult()
    big = bytes(M)
    assert L.fqg_deflate(ctx.h, big, M, b"x", 1, A.MEM_HOST, 1, C.byref(r)) == ERR_ARG
    assert L.fqg_text_deflate(ctx.h, A.TEXT_RECORDS, 1, big, M, 1, C.byref(r)) == ERR_ARG
    assert L.fqg_deflate(ctx.h, big, M - 1, b"x", 1, A.MEM_HOST, 1, C.byref(r)) == 0 and r.n_members == 1
    for store, stream in ((2, 0), (-1, 0), (A.TEXT_RECORDS, 3), (A.TEXT_RECORDS, -1), (A.TEXT_BAM2FASTQ, 6)):
        assert L.fqg_text_deflate(ctx.h, store, stream, None, 0, 1, C.byref(r)) == ERR_ARG, (store, stream)
    r = ctx.deflate(b"ACGT" * 100, final=False, want_output=False)
    assert (r["n_members"], r["gz_bytes"], r["tail_bytes"]) == (0, 0, 400)
    buf = C.create_string_buffer(512)
    # a call that is refused leaves the result of the one before it to be fetched
    r2 = A.DeflateResult()
    assert L.fqg_deflate(ctx.h, big, M, b"x", 1, A.MEM_HOST, 1, C.byref(r2)) == ERR_ARG
    assert L.fqg_text_deflate(ctx.h, 2, 0, None, 0, 1, C.byref(r2)) == ERR_ARG
    assert L.fqg_deflate_output(ctx.h, buf, 401) == ERR_ARG
    assert L.fqg_deflate_output(ctx.h, buf, 400) == 0 and buf.raw[:400] == b"ACGT" * 100
