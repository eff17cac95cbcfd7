"""fqg_bgzf_inflate on the GPU: the files of tests/bgzfgen.py through Context.bgzf_inflate against zlib - every
well-formed file (bytes, counts, no finding), more blocks than the resident grid holds, the buffer reused, frames the
header walk refuses, damaged payloads (the verdict, the first refused block and the first CRC mismatch are zlib's),
windows of fqg_inflate_output, and the device stream handed to fqg_bam2fastq / fqg_bam_add_tags where it lies.

What the wavefront does around the decoder core - staging, the copies of a round's queue, the CRC stripes, the flush,
the first finding of either kind - has no CPU model: the files bgzfgen builds for it (match geometry, queue rounds, block
sizes, payload alignment, stored blocks and cuts at a staged window's edge, several findings in one file) are checked
here, as is what the project's own compressor (fqg_bgzf_deflate) writes.  Of a file with a refused block the stream in
front of that block is compared, and the reason where bgzfgen.REASONS keeps one.

The damaged payloads come here only behind tests/test_inflate_core.py, which runs the same decoder core over the same
files under the sanitizers on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import bgzfgen

pytestmark = pytest.mark.gpu
NONE = bgzfgen.NONE


@pytest.fixture(scope="module")
def ctx():
    import fastq_utils_amd as fq
    c = fq.Context(0)
    yield c
    c.close()


def check(ctx, name, raw):
    want = bgzfgen.verdict(raw)
    got = ctx.bgzf_inflate(raw)
    assert (got["n_blocks"], got["out_bytes"], got["raw_bytes"]) == (want["n_blocks"], want["out_bytes"], want["raw_bytes"]), name
    assert got["bad_block"] == want["bad_block"], (name, got)
    assert got["crc_block"] == want["crc_block"], (name, got)
    assert (got["code"] != 0) == (want["bad_block"] != NONE) and (got["code"] == 0 or 32 <= got["code"] <= 38), (name, got)
    if bgzfgen.reason(name) is not None:
        assert got["code"] == bgzfgen.reason(name), (name, got)
    if want["bad_block"] == NONE:
        assert got["data"] == b"".join(want["texts"]), name
    else:   # what stands in front of the first refused block is defined, up to the last byte of its neighbour
        front = b"".join(want["texts"][:want["bad_block"]])
        assert ctx.inflate_output(0, len(front)) == front, name
    return want, got


AROUND_THE_WALK = ("match-geometry", "queue-rounds", "sizes", "payload-alignment", "stored-at-the-window-edge")


def test_well_formed_files(ctx):
    for name, raw in bgzfgen.well_formed().items():
        if name not in AROUND_THE_WALK:
            want, _ = check(ctx, name, raw)
            assert want["bad_block"] == want["crc_block"] == NONE, name


@pytest.mark.parametrize("name", AROUND_THE_WALK)
def test_the_work_around_the_walk(ctx, name):
    want, _ = check(ctx, name, bgzfgen.well_formed()[name])
    assert want["bad_block"] == want["crc_block"] == NONE


def test_more_blocks_than_the_grid_holds(ctx):
    import torch
    # two workgroups of k_inflate_blocks per CU (its LDS: the static_assert beside kInfLds) are resident at once; with
    # more than twice that many blocks every workgroup is dealt a second and a third one
    resident = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * resident + 37
    want, _ = check(ctx, "many", bgzfgen.many_blocks(n))
    assert want["n_blocks"] == n + 1


def test_the_buffer_is_reused(ctx):
    W = bgzfgen.well_formed()
    for name in ("65-blocks", "65-blocks", "one-l6", "zeros-l9", "empty-l6", "nothing", "2-blocks"):
        check(ctx, name, W[name])


def test_malformed_frames(ctx):
    import fastq_utils_amd as fq
    W = bgzfgen.well_formed()
    want, _ = check(ctx, "2-blocks", W["2-blocks"])
    for name, raw in bgzfgen.malformed_frames().items():
        with pytest.raises(fq.abi.FqgError, match="error -3: fqg_bgzf_inflate: block"):
            ctx.bgzf_inflate(raw)
        assert ctx.inflate_output(0, want["out_bytes"]) == b"".join(want["texts"]), name   # the call before stays fetchable


def test_damaged_payloads(ctx):
    refused = accepted = 0
    cuts, crcs = bgzfgen.sweeps()
    for name, raw in bgzfgen.damaged().items():
        if name in cuts or name in crcs:   # (the two tests below)
            continue
        want, got = check(ctx, name, raw)
        refused += want["bad_block"] != NONE
        accepted += want["bad_block"] == NONE
    assert refused >= 10 and accepted >= 5, (refused, accepted)


def test_payloads_cut_at_the_window_edge(ctx):
    D = bgzfgen.damaged()
    cuts, _ = bgzfgen.sweeps()
    assert len(cuts) == 48
    for name in cuts:
        want, got = check(ctx, name, D[name])
        assert want["bad_block"] == got["bad_block"] == 1 and got["code"] == 38, (name, got)


def test_a_wrong_crc_at_every_path_of_the_stripes(ctx):
    files = bgzfgen.sizes_wrong_crc()
    assert len(files) == 10
    for name, (raw, at) in files.items():
        want, got = check(ctx, name, raw)   # (the data whole: no block is refused)
        assert (got["bad_block"], got["crc_block"], got["code"]) == (NONE, at, 0), (name, got)


def test_several_findings_in_one_file(ctx):
    D = bgzfgen.damaged()
    for name, bad, crc, code in (("several-findings", 5, 3, 32), ("several-findings-crc-behind", 5, 7, 36)):
        for again in range(3):   # (the order in which the workgroups report is not the same every time)
            _, got = check(ctx, name, D[name])
            assert (got["bad_block"], got["crc_block"], got["code"]) == (bad, crc, code), (name, got)


def test_output_windows(ctx):
    import fastq_utils_amd as fq
    want, got = check(ctx, "3 blocks", bgzfgen.well_formed()["65-blocks"])
    data, n = b"".join(want["texts"]), want["out_bytes"]
    for first, nbytes in ((0, 0), (0, 1), (1, 1), (1, n - 1), (5, 70001 % n), (n - 1, 1), (n, 0), (0, n)):
        assert ctx.inflate_output(first, nbytes) == data[first:first + nbytes], (first, nbytes)
    for first, nbytes in ((n, 1), (n + 1, 0), (0, n + 1), (2 ** 64 - 1, 2)):
        with pytest.raises(fq.abi.FqgError, match="error -3"):
            ctx.inflate_output(first, nbytes)


def bgzf_of(stream, piece=40000):
    return b"".join(bgzfgen.text_block(stream[k:k + piece], level=(1, 6)[(k // piece) & 1]) for k in range(0, len(stream), piece)) + bgzfgen.EOF


def offsets_of(stream):
    import fastq_utils_amd as fq
    buf = (C.c_char * len(stream)).from_buffer_copy(stream)
    offs, n, _ = fq.abi._bam_offsets(buf, len(stream))
    return [offs[i] for i in range(n)]


def test_the_device_stream_feeds_bam2fastq(ctx):
    from tests.test_gpu_bam2fastq import make_stream
    stream = make_stream(np.random.default_rng(41), 900, 0)
    want = ctx.bam2fastq(stream)
    offs = offsets_of(stream)
    got = ctx.bgzf_inflate(bgzf_of(stream))
    assert got["data"] == stream and ctx.inflate_device() % 16 == 0
    # (whole, and from the first record on: an address that is not 16-byte aligned)
    assert ctx.bam2fastq(ctx.inflate_device(), offsets=offs, nbytes=len(stream)) == want
    p0 = offs[0]
    assert p0 % 16
    assert ctx.bam2fastq(ctx.inflate_device() + p0, offsets=[o - p0 for o in offs], nbytes=len(stream) - p0) == want
    assert ctx.inflate_output(0, len(stream)) == stream   # the calls did not move or write it


def test_the_device_stream_feeds_bam_add_tags(ctx):
    from tests.test_gpu_bam_tags import make_stream, record_offsets
    stream, names = make_stream(np.random.default_rng(43), 1200, long_every=211)
    want = ctx.bam_add_tags(stream, tx_tag=True, targets=names)
    got = ctx.bgzf_inflate(bgzf_of(stream))
    assert got["data"] == stream
    dev = ctx.bam_add_tags(ctx.inflate_device(), tx_tag=True, targets=names, offsets=record_offsets(stream), nbytes=len(stream))
    assert dev == want and dev["code"] == 0
    assert ctx.inflate_output(0, len(stream)) == stream


# ---- the project's own compressor, read back --------------------------------------------------
def own_texts():
    from tests.test_fastdeflate import contents
    from tests.test_gpu_deflate import structure
    import fastq_utils_amd as fq
    M = fq.abi.GZ_MEMBER_TEXT
    return [(name, data[:2 * M + 7]) for name, data in contents()] + [("structure_%d" % seed, structure(seed)) for seed in range(12)]


def test_blocks_of_the_projects_compressor(ctx):
    """fqg_bgzf_deflate's code lengths, two-symbol codes and run-length coded headers, which zlib never writes"""
    import fastq_utils_amd as fq
    M = fq.abi.GZ_MEMBER_TEXT
    texts = own_texts()
    assert len(texts) == 26
    for name, data in texts:
        members = ctx.bgzf_deflate(data)["members"]
        got = ctx.bgzf_inflate(members)
        assert (got["n_blocks"], got["out_bytes"], got["raw_bytes"]) == (-(-len(data) // M) + 1, len(data), len(members)), name
        assert (got["bad_block"], got["crc_block"], got["code"]) == (NONE, NONE, 0), (name, got)
        assert got["data"] == data, name
        if len(data) > 2 * M:   # once more where it lies on the device, in windows over the blocks' borders
            got = ctx.bgzf_inflate(members, want_output=False)
            assert "data" not in got and ctx.inflate_device() and got["out_bytes"] == len(data)
            for first, nbytes in ((M - 5, 10), (2 * M - 17, len(data) - 2 * M + 17), (M - 1, M + 2)):
                assert ctx.inflate_output(first, nbytes) == data[first:first + nbytes], (name, first, nbytes)
