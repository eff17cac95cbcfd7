"""fqg_bgzf_inflate on the GPU: the files of tests/bgzfgen.py through Context.bgzf_inflate against zlib - every
well-formed file (bytes, counts, no finding), more blocks than the resident grid holds, the buffer reused, frames the
header walk refuses, damaged payloads (the verdict, the first refused block and the first CRC mismatch are zlib's),
windows of fqg_inflate_output, and the device stream handed to fqg_bam2fastq / fqg_bam_add_tags where it lies.

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
    if want["bad_block"] == NONE:
        assert got["data"] == b"".join(want["texts"]), name
    return want, got


def test_well_formed_files(ctx):
    for name, raw in bgzfgen.well_formed().items():
        want, _ = check(ctx, name, raw)
        assert want["bad_block"] == want["crc_block"] == NONE, name


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
    for name, raw in bgzfgen.damaged().items():
        want, got = check(ctx, name, raw)
        refused += want["bad_block"] != NONE
        accepted += want["bad_block"] == NONE
    assert refused >= 10 and accepted >= 5, (refused, accepted)


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
