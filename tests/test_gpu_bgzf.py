"""fqg_bgzf_deflate / fqg_text_bgzf_deflate (BGZF blocks compressed on the device), the FQG_TEXT_BAM_TAGS store and
fqg_deflate_output_begin / _wait, through abi.py.  The output is walked by BSIZE: every block has BGZF's fixed sixteen
header bytes and BSIZE = its length - 1, every block but the last holds FQG_GZ_MEMBER_TEXT bytes of text, a final call
ends in the 28-byte end-of-file block, and behind the eighteen header bytes a block is byte for byte the gzip member
fqg_deflate makes of the same text behind ITS ten - the compressor tests/cxx/deflate_model.cpp models.  The model's
member behind the eighteen header bytes, BSIZE set, is what a block must be: compared on the families of
tests/deflgen.py (what each reaches: tests/test_gpu_deflate.py), on every alignment of a device source behind every
carry, and on more blocks than workgroups from a device tensor."""
import ctypes as C
import gzip
import random
import time
import zlib

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import bam_tags_oracle as bto
from tests import bamgen, deflgen
from tests.test_gpu_bam_tags import make_stream
from tests.test_pgzip import fastq_text

pytestmark = pytest.mark.gpu
A = fq.abi
M = A.GZ_MEMBER_TEXT
ERR_ARG = -3  # FQG_ERR_ARG, include/fqg.h
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0])
EOF = HEAD + bytes([0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
LENGTHS = [0, 1, 3, M - 1, M, M + 1, 2 * M, 3 * M + 17]


@pytest.fixture(scope="module")
def ctx():
    c = fq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def contents():
    """name -> 4 * M bytes at least"""
    need = 4 * M
    rng = np.random.default_rng(5)
    recs, size = [], 0
    while size < need:
        name = b"STAGS_CELL=%s_UMI=%s_ETAGS_M%d" % (bamgen.barcode(rng, 16), bamgen.barcode(rng, 10), len(recs))
        recs.append(bamgen.record(name, bamgen.aux_z(b"XA", b"x" * int(rng.integers(0, 20))), seq_len=int(rng.integers(20, 90))))
        size += len(recs[-1])
    fastq = fastq_text(1500, 2)
    return {"fastq": (fastq * (need // len(fastq) + 1))[:need], "bam_records": b"".join(recs)[:need], "zeros": bytes(need),
            "noise": random.Random(3).randbytes(need)}


@pytest.fixture(scope="module")
def model():
    """tests/cxx/deflate_model.cpp, built once (tests/test_gpu_deflate.py shares it)"""
    return deflgen.shared()[0]


@pytest.fixture(scope="module")
def families():
    return deflgen.shared()[1]


def blocks_of(raw):
    """[(block bytes, its text)] of a run of BGZF blocks, walked by BSIZE; every block inflated by itself"""
    out = []
    while raw:
        assert len(raw) >= 28 and raw[:16] == HEAD, raw[:18].hex()
        size = int.from_bytes(raw[16:18], "little") + 1
        block = raw[:size]
        assert len(block) == size, "a block that runs beyond the output"
        d = zlib.decompressobj(-15)
        text = d.decompress(block[18:-8]) + d.flush()
        assert d.eof and not d.unused_data
        assert int.from_bytes(block[-8:-4], "little") == zlib.crc32(text) and int.from_bytes(block[-4:], "little") == len(text)
        out.append((block, text))
        raw = raw[size:]
    return out


def gzip_members_of(gz):
    out = []
    while gz:
        d = zlib.decompressobj(31)
        d.decompress(gz)
        assert d.eof
        out.append(gz[:len(gz) - len(d.unused_data)])
        gz = d.unused_data
    return out


def check(ctx, label, data, final, **how):
    r = ctx.bgzf_deflate(data, final=final, **how)
    text_bytes = (len(data) if isinstance(data, bytes) else how["nbytes"]) + len(how.get("carry", b""))
    n_data = -(-text_bytes // M) if final else text_bytes // M
    assert r["text_bytes"] == text_bytes and r["n_members"] == n_data and r["gz_bytes"] == len(r["members"]), label
    blocks = blocks_of(r["members"])
    if final:
        assert r["members"][-28:] == EOF and blocks[-1] == (EOF, b"") and r["tail"] == b"", label
        blocks.pop()
    else:
        assert r["tail_bytes"] == text_bytes % M, label
    assert len(blocks) == n_data, (label, len(blocks))
    assert all(len(t) == M for _, t in blocks[:-1]) and all(0 < len(t) <= M for _, t in blocks[-1:]), label
    assert all(len(b) <= len(t) + 31 and b != EOF for b, t in blocks), label
    return r, blocks


@pytest.mark.parametrize("final", [True, False], ids=["final", "not_final"])
@pytest.mark.parametrize("n", LENGTHS, ids=lambda n: "bytes_%d" % n)
@pytest.mark.parametrize("name", ["fastq", "bam_records", "zeros", "noise"])
def test_blocks(ctx, contents, name, n, final):
    data = contents[name][:n]
    r, blocks = check(ctx, "%s[:%d]" % (name, n), data, final)
    kept = n if final else n // M * M
    assert b"".join(t for _, t in blocks) == data[:kept] and r["tail"] == data[kept:]
    assert (gzip.decompress(r["members"]) if r["members"] else b"") == data[:kept]
    # behind the header a block is the gzip member of the same compressor (an empty text: gzip has one member, BGZF none)
    members = gzip_members_of(ctx.deflate(data, final=final)["members"]) if kept else []
    assert len(members) == len(blocks)
    for (block, text), member in zip(blocks, members):
        assert block[18:] == member[10:], (name, n, len(text))
    if name == "noise":
        assert all(len(b) == len(t) + 31 and b[18] == 1 for b, t in blocks)  # stored
    if name == "zeros":
        assert all(len(b) < 1000 for b, _ in blocks)


FAMILIES = ["sizes_" + c for c in deflgen.SIZE_CONTENTS] + ["tie", "parse_geometry", "same_slot", "window", "wide_tokens", "member_cycle"]


@pytest.mark.parametrize("name", FAMILIES)
def test_generated_texts_are_the_models_blocks(ctx, families, name):
    """every text of a family of tests/deflgen.py, one call from host memory each"""
    f = families[name]
    for k, text in enumerate(f.texts):
        r = ctx.bgzf_deflate(text)
        assert r["n_members"] == (len(text) > 0) and r["members"] == f.bgzf(k), (name, k, len(text), f.reports[k][0]["written"])


def test_every_alignment_of_a_device_source_behind_every_carry(ctx, model):
    import torch
    texts = deflgen.alignment_texts()
    want = {}
    for key, gz, reports in zip(texts, *model.run(list(texts.values()))):
        want[key] = deflgen.bgzf_of(deflgen.split_members(gz, reports))
    t = torch.zeros(M + 700 + 64, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    for (c, n), text in texts.items():
        src = torch.frombuffer(bytearray(text[c:]), dtype=torch.uint8).cuda()
        for s in range(16):
            t.fill_(0x5A)
            t[16 + s:16 + s + n - c] = src
            torch.cuda.synchronize()
            for again in range(1 + (n > M)):
                r = ctx.bgzf_deflate(t.data_ptr() + 16 + s, carry=text[:c], nbytes=n - c)
                assert r["n_members"] == -(-n // M) and r["members"] == want[c, n], (c, n, s, again)


def test_more_blocks_than_workgroups_and_than_a_span_of_offsets(ctx, model, families):
    """the member cycle of tests/deflgen.py from a device tensor (tests/test_gpu_deflate.py: the same from host memory)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_members = max(2049 + 2, 2 * cus + 3)
    assert n_members >= 2049 + 2 and n_members > 2 * cus + 2
    f = families["member_cycle"]
    text, order, last = deflgen.cycle_text(f.texts, n_members)
    blocks = [deflgen.bgzf_block(gz) for gz in f.gz]
    want = b"".join(blocks[k] for k in order) + deflgen.bgzf_of(model.run([last], report=False)[0])
    t = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    t[21:21 + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for again in range(2):
        t0 = time.perf_counter()
        r = ctx.bgzf_deflate(t.data_ptr() + 21, nbytes=len(text))
        print("%d blocks, %d bytes of text: %.2f s" % (n_members, len(text), time.perf_counter() - t0))
        assert r["n_members"] == n_members and r["text_bytes"] == len(text)
        assert r["members"] == want, again


def test_empty_text(ctx):
    r = ctx.bgzf_deflate(b"")
    assert (r["members"], r["n_members"], r["gz_bytes"], r["tail_bytes"]) == (EOF, 0, 28, 0)
    r = ctx.bgzf_deflate(b"", final=False)
    assert (r["members"], r["n_members"], r["gz_bytes"], r["tail_bytes"]) == (b"", 0, 0, 0)


@pytest.mark.parametrize("final", [True, False], ids=["final", "not_final"])
@pytest.mark.parametrize("carry", [0, 1, M - 1, M, M + 1, 2 * M + 100], ids=lambda n: "carry_%d" % n)
def test_host_carry_of_any_length_in_front_of_a_device_source(ctx, contents, carry, final):
    """members wholly inside the carry, the member on the seam, members of the source alone: one text"""
    import torch
    n_src = M + 777
    assert carry + n_src <= len(contents["fastq"])
    data = contents["fastq"][:carry + n_src]
    want, _ = check(ctx, "one call", data, final)
    src = data[carry:]
    t = torch.zeros(n_src + 64, dtype=torch.uint8, device="cuda")
    t[5:5 + n_src] = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()  # (an address that is no multiple of 16)
    torch.cuda.synchronize()
    got, _ = check(ctx, "carry + device", t.data_ptr() + 5, final, carry=data[:carry], nbytes=n_src)
    assert (got["members"], got["tail"]) == (want["members"], want["tail"])
    # ... and a carry with nothing behind it (what is left when a file is closed)
    alone = ctx.bgzf_deflate(b"", carry=data[:carry], final=final)
    whole = ctx.bgzf_deflate(data[:carry], final=final)
    assert (alone["members"], alone["tail"]) == (whole["members"], whole["tail"])


def test_a_chain_of_calls_is_one_call(ctx, contents):
    for name in ("fastq", "bam_records"):
        data = contents[name][:3 * M + 17]
        one_call = ctx.bgzf_deflate(data)["members"]
        cuts = [0, M + 5, M + 6, len(data)]
        got, carry = [], b""
        for a, b in zip(cuts, cuts[1:]):
            r = ctx.bgzf_deflate(data[a:b], carry=carry, final=b == len(data))
            assert r["tail"] == data[b - len(r["tail"]):b] and len(r["tail"]) < M
            got.append(r["members"])
            carry = r["tail"]
        assert carry == b"" and b"".join(got) == one_call
        assert ctx.bgzf_deflate(data)["members"] == one_call


def test_records_of_bam_add_tags(ctx):
    """FQG_TEXT_BAM_TAGS: the records where fqg_bam_add_tags left them, a header of two blocks as the carry"""
    L = A.load()
    stream, names = make_stream(np.random.default_rng(12), 2500, refs=3000)
    _, first = bto.parse_header(stream)
    header = stream[:first]
    assert len(header) > M
    r = ctx.bam_add_tags(stream, targets=names, want_output=False)
    assert r["code"] == 0 and r["out_bytes"] > M
    got = ctx.text_bgzf_deflate(A.TEXT_BAM_TAGS, 0, carry=header)
    plain = ctx.text_deflate(A.TEXT_BAM_TAGS, 0)  # the gzip frame reads the same store
    buf = C.create_string_buffer(r["out_bytes"])
    assert L.fqg_bam_add_tags_output(ctx.h, buf, r["out_bytes"]) == 0  # reading the store left it as it was
    records = buf.raw[:r["out_bytes"]]
    assert records == ctx.bam_add_tags(stream, targets=names)["records"]
    assert got["text_bytes"] == len(header) + len(records) and got["tail_bytes"] == 0
    assert got["members"] == ctx.bgzf_deflate(header + records)["members"]
    assert gzip.decompress(got["members"]) == header + records
    assert plain["members"] == ctx.deflate(records)["members"]
    not_final = ctx.text_bgzf_deflate(A.TEXT_BAM_TAGS, 0, carry=header, final=False)
    want = ctx.bgzf_deflate(header + records, final=False)
    assert (not_final["members"], not_final["tail"]) == (want["members"], want["tail"])


def test_output_begin_and_wait(ctx, contents):
    """the copies land in pinned memory (fqg_host_alloc), so they are asynchronous: begin returns while they run"""
    data = contents["fastq"][:2 * M + 300]
    want = ctx.bgzf_deflate(data, final=False)
    n = want["gz_bytes"] + want["tail_bytes"]
    ctx.bgzf_deflate(data, final=False, want_output=False)
    out = ctx.deflate_output_begin(n)
    ctx.deflate_output_wait()
    assert out.bytes() == want["members"] + want["tail"]
    out.free()
    # without a wait: the next deflate call writes the device buffer the copy reads, so it waits for the copy itself.
    # 32 MiB of noise are stored members, 32 MiB to copy: long enough for a call that did not wait to overwrite what
    # the copy has not read yet (the next call's members go to the start of the same buffer)
    noise = random.Random(9).randbytes(32 << 20)
    big = ctx.deflate(noise, final=False)
    n = big["gz_bytes"] + big["tail_bytes"]
    assert n > len(noise)
    ctx.deflate(noise, final=False, want_output=False)
    out = ctx.deflate_output_begin(n)
    other = ctx.bgzf_deflate(contents["zeros"][:M + 1])
    assert out.bytes() == big["members"] + big["tail"]
    out.free()
    assert gzip.decompress(other["members"]) == bytes(M + 1)
    ctx.deflate_output_wait()  # (nothing is pending: returns at once)
    L = A.load()
    assert L.fqg_deflate_output_begin(ctx.h, C.create_string_buffer(8), other["gz_bytes"] + 1) == ERR_ARG


def test_argument_errors(ctx):
    L = A.load()
    r = A.DeflateResult()
    big = bytes(M)
    keep = ctx.bgzf_deflate(b"ACGT" * 100, final=False, want_output=False)
    assert (keep["n_members"], keep["gz_bytes"], keep["tail_bytes"]) == (0, 0, 400)
    # a store that does not exist; the call that is refused leaves the result before it to be fetched
    for store, stream in ((3, 0), (-1, 0), (A.TEXT_BAM_TAGS, 1), (A.TEXT_BAM_TAGS, -1), (A.TEXT_RECORDS, 3), (A.TEXT_BAM2FASTQ, 6)):
        assert L.fqg_text_bgzf_deflate(ctx.h, store, stream, None, 0, 1, C.byref(r)) == ERR_ARG, (store, stream)
        assert L.fqg_text_deflate(ctx.h, store, stream, None, 0, 1, C.byref(r)) == ERR_ARG, (store, stream)
    # the gzip pair keeps refusing a carry of a member's text or more
    assert L.fqg_deflate(ctx.h, big, M, b"x", 1, A.MEM_HOST, 1, C.byref(r)) == ERR_ARG
    assert L.fqg_text_deflate(ctx.h, A.TEXT_RECORDS, 1, big, M, 1, C.byref(r)) == ERR_ARG
    buf = C.create_string_buffer(512)
    assert L.fqg_deflate_output(ctx.h, buf, 401) == ERR_ARG
    assert L.fqg_deflate_output(ctx.h, buf, 400) == 0 and buf.raw[:400] == b"ACGT" * 100
    # ... which BGZF takes
    assert L.fqg_bgzf_deflate(ctx.h, big, M, b"x", 1, A.MEM_HOST, 1, C.byref(r)) == 0 and r.n_members == 2
    # the records of fqg_bam_add_tags are no store before the context's first fqg_bam_add_tags
    with fq.Context(0) as fresh:
        assert L.fqg_text_bgzf_deflate(fresh.h, A.TEXT_BAM_TAGS, 0, None, 0, 1, C.byref(r)) == ERR_ARG
        fresh.bam_add_tags(bamgen.header(), want_output=False)  # (no alignments: an empty store)
        assert fresh.text_bgzf_deflate(A.TEXT_BAM_TAGS, 0, carry=bamgen.header())["members"] == \
            fresh.bgzf_deflate(bamgen.header())["members"]
