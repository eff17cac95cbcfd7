"""fqg_bam_index_device: the record index of an inflated BAM stream made where the stream lies.

Every stream of tests/bamidx_gen.py (the shapes tests/test_bam_index_core.py runs through the CPU model) goes through the
kernels, at the default geometry and at segments of 64, 128 and 4096 bytes in windows of two and five segments, with the
default ring and with one so small that every record of 64 bytes or more is a hop: n_records, used and every offset are
those of the loop of fqg_bam_index_records started at first_record (bamidx_gen.walk, checked against the library in
test_bam_index_core.py).  The streams lie back to back in one device buffer, at every address offset 0 .. 15 in turn, with
other streams' bytes in front and behind.  Then the real files - every .bam under tests/golden, bamgen.config4 - and the
bulk calls fed from the index on the device (FQG_MEM_DEVICE_INDEXED) against the same calls with host offsets, and
fqg_bam_header_end on every prefix of three headers against fqg_bam_index_records' verdict."""
import struct

import random

import pytest

from tests import bamidx_gen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SMALL = [(seg, k * seg) for seg in (64, 128, 4096) for k in (2, 5)]
ERR_ARG = -3


@pytest.fixture(scope="module")
def ctx():
    import fastq_utils_amd as fq
    c = fq.Context(0)
    yield c
    c.close()


def geometry(monkeypatch, seg=None, window=None, ring=None):
    for name, v in (("FQGPU_BAMIDX_SEG", seg), ("FQGPU_BAMIDX_WINDOW", window), ("FQGPU_BAMIDX_RING", ring)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


class Resident:
    """the streams of `cases` back to back in one device buffer; stream k starts at address offset (k + shift) % 16"""

    def __init__(self, cases, shift=0):
        blob, self.at = bytearray(b"\x24\0\0\0" * 8), []   # (what lies around a stream looks like records too)
        for k, (_, s, _) in enumerate(cases):
            blob += b"\x20\0\0\0" * 4
            while len(blob) % 16 != (k + shift) % 16:
                blob += b"\x20"
            self.at.append(len(blob))
            blob += s
        blob += b"\x24\0\0\0" * 16
        self.t = torch.frombuffer(blob, dtype=torch.uint8).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]


def check_cases(ctx, cases, shift=0, tag=""):
    res = Resident(cases, shift)
    for k, (name, s, first) in enumerate(cases):
        want = bamidx_gen.walk(s, first)
        r = ctx.bam_index_device(res.ptr(k), len(s), first)
        assert (r["n_records"], r["used"]) == (len(want[0]), want[1]), (name, tag, r)
        assert ctx.bam_index_output(0, r["n_records"]) == want[0], (name, tag)


WANT = {}   # the cases of a geometry, made once


def cases_of(seg, window):
    if (seg, window) not in WANT:
        WANT[seg, window] = bamidx_gen.streams(seg, window)
    return WANT[seg, window]


def test_default_geometry(ctx, monkeypatch):
    geometry(monkeypatch)
    check_cases(ctx, cases_of(64, 128), 0, "default")
    check_cases(ctx, cases_of(4096, 20480), 5, "default")


@pytest.mark.parametrize("seg,window", SMALL)
@pytest.mark.parametrize("ring", (None, 128))
def test_small_segments_and_windows(ctx, monkeypatch, seg, window, ring):
    geometry(monkeypatch, seg, window, ring)
    check_cases(ctx, cases_of(seg, window), seg // 64 + window // seg, (seg, window, ring))


def test_every_address_offset(ctx, monkeypatch):
    cases = [c for c in cases_of(64, 128) if c[0].startswith(("decoys-", "seg-field-", "seg-stop-", "stream-inside", "cut-3", "minimal-7"))]
    assert len(cases) > 30
    for seg, window, ring in ((64, 128, 128), (None, None, None)):
        geometry(monkeypatch, seg, window, ring)
        for shift in range(16):
            check_cases(ctx, cases, shift, (seg, shift))


def test_output_ranges_and_a_second_call(ctx, monkeypatch):
    geometry(monkeypatch, 128, 256)
    cases = {c[0]: c for c in cases_of(128, 256)}
    a, b = cases["minimal-150"], cases["decoys-1"]
    res = Resident([a, b])
    r = ctx.bam_index_device(res.ptr(0), len(a[1]), a[2])
    want = bamidx_gen.walk(a[1], a[2])[0]
    assert r["n_records"] == 150 and ctx.bam_index_offsets() != 0
    for first, n in ((0, 150), (0, 0), (150, 0), (149, 1), (17, 60), (1, 1)):
        assert ctx.bam_index_output(first, n) == want[first:first + n]
    for first, n in ((0, 151), (151, 0), (150, 1), (2 ** 64 - 1, 2)):
        with pytest.raises(Exception):
            ctx.bam_index_output(first, n)
    r = ctx.bam_index_device(res.ptr(1), len(b[1]), b[2])   # a second call replaces the first
    want = bamidx_gen.walk(b[1], b[2])[0]
    assert r["n_records"] == len(want) == 7 and ctx.bam_index_output(0, 7) == want
    with pytest.raises(Exception):
        ctx.bam_index_output(0, 8)
    with pytest.raises(Exception):
        ctx.bam_index_device(res.ptr(1), len(b[1]), len(b[1]) + 1)   # first_record behind the stream
    ctx.release_scratch()
    assert ctx.bam_index_offsets() == 0
    with pytest.raises(Exception):
        ctx.bam_index_output(0, 0)


# ---- real files ---------------------------------------------------------------------------------
def header_end(stream):
    """where fqg_bam_index_records starts its record loop, or None for a stream it refuses"""
    return bamidx_gen.first_record(stream)


@pytest.fixture(scope="module")
def real_files():
    cases = bamidx_gen.real_files()
    wants = [bamidx_gen.walk(s, first) for _, s, first in cases]
    for (name, s, _), want in zip(cases, wants):   # (where the library's own walk takes the stream, it is the reference)
        lib = bamidx_gen.library_walk(s)
        assert lib is None or lib == want, name
    return cases, Resident(cases), wants


@pytest.mark.parametrize("seg,window", [(None, None)] + SMALL)
@pytest.mark.parametrize("ring", (None, 128))
def test_real_files(ctx, monkeypatch, real_files, seg, window, ring):
    """every golden stream, whole, at the default geometry and at every small one"""
    cases, res, wants = real_files
    geometry(monkeypatch, seg, window, ring)
    for k, ((name, s, first), want) in enumerate(zip(cases, wants)):
        r = ctx.bam_index_device(res.ptr(k), len(s), first)
        assert (r["n_records"], r["used"]) == (len(want[0]), want[1]), (name, r)
        assert ctx.bam_index_output(0, r["n_records"]) == want[0], name


def references(stream):
    p = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref, p = struct.unpack_from("<i", stream, p)[0], p + 4
    names = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, p)[0]
        names.append(stream[p + 4:p + 4 + l_name - 1])
        p += 8 + l_name
    return names


def outcome(call):
    """what a call returns, or the library's refusal (the same input must be refused the same way)"""
    try:
        return call()
    except Exception as e:   # noqa: BLE001
        return ("refused", str(e))


def test_bulk_calls_fed_from_the_index(ctx, monkeypatch, real_files):
    """fqg_bam_add_tags, fqg_bam2fastq and fqg_umi_count with FQG_MEM_DEVICE_INDEXED: the offsets of fqg_bam_index_offsets
    against host offsets, same stream on the device; bam2fastq also in pieces of 1 and 7 alignments (files of up to a
    hundred alignments: a piece is a call)"""
    cases, res, wants = real_files
    geometry(monkeypatch)
    n_calls = 0
    for k, ((name, s, first), (offs, used)) in enumerate(zip(cases, wants)):
        if header_end(s) is None or not offs:
            continue
        ptr, n = res.ptr(k) if res.ptr(k) % 16 == 0 else None, len(offs)
        if ptr is None:   # (the bulk calls copy a stream that is not at a 16-byte boundary: give them one that is)
            own = torch.frombuffer(bytearray(s + bytes(64)), dtype=torch.uint8).to(torch.device("cuda", 0))
            ptr = own.data_ptr()
        r = ctx.bam_index_device(ptr, len(s), first)
        assert r == {"n_records": n, "used": used}, name
        index = (ctx.bam_index_offsets(), n)
        refs = references(s)
        for kw in ({}, {"tenx": True}) + (({"tx_tag": True, "targets": refs},) if len(refs) <= 5000 else ()):
            a = outcome(lambda: ctx.bam_add_tags(ptr, nbytes=used, offsets=offs, **kw))
            b = outcome(lambda: ctx.bam_add_tags(ptr, nbytes=used, offsets_device=index, **kw))
            assert a == b, (name, kw)
            n_calls += 1
        a = outcome(lambda: ctx.umi_count(ptr, nbytes=len(s), offsets=offs))
        b = outcome(lambda: ctx.umi_count(ptr, nbytes=len(s), offsets_device=index))
        assert a == b, name
        for tenx in (False, True):
            for piece in (1, 7, n) if n <= 100 else (n,):
                for done in range(0, n, piece):
                    last = min(n, done + piece)
                    end = offs[last] if last < n else used
                    a = ctx.bam2fastq(ptr, tenx=tenx, nbytes=end, offsets=offs[done:last], first_alignment=done)
                    b = ctx.bam2fastq(ptr, tenx=tenx, nbytes=end, offsets_device=(index[0] + 8 * done, last - done), first_alignment=done)
                    assert a == b, (name, tenx, piece, done)
                    n_calls += 1
    assert n_calls > 300


# ---- the header walk over a prefix ----------------------------------------------------------------
def accepted(stream):
    """fqg_bam_index_records' verdict on the whole of `stream`"""
    import ctypes as C

    import fastq_utils_amd as fq
    n, used = C.c_uint64(), C.c_uint64()
    return fq.abi.load().fqg_bam_index_records(stream, len(stream), None, 0, C.byref(n), C.byref(used)) == 0


class HeaderEnd:
    """fqg_bam_header_end with its two result cells made once (the test calls it a million times)"""

    def __init__(self):
        import ctypes as C

        import fastq_utils_amd as fq
        self.fn, self.first, self.need = fq.abi.load().fqg_bam_header_end, C.c_uint64(), C.c_uint64()
        self.a, self.b = C.byref(self.first), C.byref(self.need)

    def __call__(self, prefix, total):
        rc = self.fn(prefix, len(prefix), total, self.a, self.b)
        return rc, self.first.value, self.need.value


@pytest.mark.parametrize("n_ref", (0, 3, 300))
def test_header_end_on_every_prefix(n_ref):
    import fastq_utils_amd as fq
    header_end_of = HeaderEnd()
    hdr = bamidx_gen.header(n_ref) if n_ref else bamidx_gen.HDR
    body = bamidx_gen.rec(36) + bamidx_gen.rec(50)
    full = hdr + body
    assert fq.abi._bam_offsets(full, len(full))[0][0] == len(hdr)
    rng = random.Random(n_ref)
    for total in range(len(full) + 1):
        stream = full[:total]
        want = (0, len(hdr)) if accepted(stream) else (ERR_ARG, 0)   # (every truncated header is a refusal)
        assert (want[0] == 0) == (total >= len(hdr)), total
        rc, first, need = header_end_of(stream, total)   # all of it at hand: a verdict, never a question
        assert (rc, first) == want, (total, rc, first, need)
        # from nothing, fetching exactly what is asked for - and from prefixes that end anywhere, inside a field too
        for start in (0, rng.randrange(total + 1)):
            have, steps = start, 0
            while True:
                rc, first, need = header_end_of(stream[:have], total)
                if rc != fq.abi.NEED_MORE:
                    break
                assert have < need <= total, (total, have, need)
                have, steps = need, steps + 1
            assert steps <= n_ref + 3 and (rc, first) == want, (total, start, have, steps)
    for have in range(len(full) + 1):   # every prefix of the whole stream: a question with a good answer, or the verdict
        rc, first, need = header_end_of(full[:have], len(full))
        assert (rc == fq.abi.NEED_MORE and have < need <= len(hdr)) or (rc, first) == (0, len(hdr)), (have, rc, first, need)
        # as BamInput fetches: at least what is asked for, usually more
        more = min(len(full), max(need, 2 * have)) if rc == fq.abi.NEED_MORE else have
        rc2, first2, need2 = header_end_of(full[:more], len(full))
        assert (rc2 == fq.abi.NEED_MORE and more < need2) or (rc2, first2) == (0, len(hdr)), (have, more)
    assert fq.abi.bam_header_end(full[:20], 10)[0] == ERR_ARG   # more at hand than the stream has
    q = 8 + struct.unpack_from("<i", full, 4)[0]   # where n_ref stands
    bad = [b"BAM\2" + full[4:], full[:4] + struct.pack("<i", -1) + full[8:], full[:q] + struct.pack("<i", -5) + full[q + 4:],
           full[:q] + struct.pack("<i", n_ref + 1) + full[q + 4:]]
    if n_ref:   # the last reference's name runs past the stream
        bad.append(full[:q + 4] + struct.pack("<i", len(full)) + full[q + 8:])
    for b in bad[:3] + bad[4:]:
        assert not accepted(b) and fq.abi.bam_header_end(b, len(b))[0] == ERR_ARG
    b = bad[3]   # one reference more than there is: whatever the library says of the records read as a reference
    assert (fq.abi.bam_header_end(b, len(b))[0] == 0) == accepted(b)
