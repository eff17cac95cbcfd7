"""Streams for the record index made on the device (fqg_bam_index_device, fastq_utils_amd/csrc/fqg_bam_index_core.h):
the smallest shapes at which the backward recurrence, the segment and window seams, the ring and the follower can
still go wrong.  Seeded; a case is (name, stream, first_record).  `walk` is the loop of fqg_bam_index_records started at
an arbitrary position - the reference of every comparison."""
import struct

import numpy as np

HDR = b"BAM\1" + struct.pack("<ii", 0, 0)  # l_text = 0, n_ref = 0: the records start at byte 12
FIRST = len(HDR)


def walk(b, first):
    """(offsets, used): fqg_bam_index_records' loop from `first`"""
    p, offs, n = first, [], len(b)
    while p + 4 <= n:
        block = int.from_bytes(b[p:p + 4], "little", signed=True)
        if block < 32 or p + 4 + block > n:
            break
        offs.append(p)
        p += 4 + block
    return offs, p


def header(n_ref, text=b"@HD\tVN:1.0\n"):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for i in range(n_ref):
        name = b"ref%d" % i + b"x" * (i % 7) + b"\0"
        h += struct.pack("<i", len(name)) + name + struct.pack("<i", 1000 + i)
    return h


def rec(size, body=None):
    """a record of `size` bytes in all (>= 36); body: what stands behind the block_size field, cut or zero-padded"""
    assert size >= 36
    body = (body or b"")[:size - 4]
    return struct.pack("<i", size - 4) + body + bytes(size - 4 - len(body))


def decoy_body(size, align, step=1, lo=32, hi=400):
    """little-endian values lo..hi back to back from byte `align` on: every position of that alignment starts a
    valid-looking chain (with step 4 one that stays on the alignment, decoy after decoy, to the end of the body)"""
    vals = np.arange(lo, hi + 1, step, dtype="<i4")
    reps = -(-size // (4 * vals.size)) + 1
    return (bytes(align) + np.tile(vals, reps).tobytes())[:size]


def put_block(stream, at, value):
    return stream[:at] + struct.pack("<i", value) + stream[at + 4:]


def basics():
    out = [("no-records", HDR, FIRST), ("one-record", HDR + rec(36), FIRST), ("first-at-the-end", HDR + rec(40), len(HDR) + 40),
           ("four-bytes-left", HDR + bytes(4), FIRST), ("three-bytes-left", HDR + bytes(3), FIRST),
           ("a-valid-field-and-nothing-else", HDR + struct.pack("<i", 32), FIRST)]
    for n in range(1, 201):
        out.append(("minimal-%d" % n, HDR + rec(36) * n, FIRST))
    rng = np.random.default_rng(7)
    sizes = [int(x) for x in rng.integers(36, 300, 9)]
    base = HDR + b"".join(rec(s, bytes(rng.integers(0, 256, s, dtype=np.uint8))) for s in sizes)
    offs, used = walk(base, FIRST)
    assert len(offs) == 9 and used == len(base)
    for k in (0, 1, 8):
        p = offs[k]
        for label, v in (("31", 31), ("0", 0), ("-1", -1), ("max", 0x7FFFFFFF), ("one-too-long", len(base) - p - 4 + 1)):
            out.append(("stop-%s-at-%d" % (label, k), put_block(base, p, v), FIRST))
    for cut in range(1, 41):
        out.append(("cut-%d" % cut, base[:len(base) - cut], FIRST))
    for n_ref in (3, 300):
        h = header(n_ref)
        out.append(("header-%d-refs" % n_ref, h + base[FIRST:], len(h)))
    return out


def geometry(u, tag):
    """the edges of a seam every `u` bytes (a segment's or a window's; seams lie at FIRST + j * u)"""
    out = []
    tail = rec(36) * 3 + rec(52) + rec(36)
    for d in range(4):  # a block_size field that starts d bytes before a seam
        out.append(("%s-field-%d-before-seam" % (tag, d), HDR + rec(2 * u - d) + tail, FIRST))
        if u - d >= 36:
            out.append(("%s-field-%d-before-first-seam" % (tag, d), HDR + rec(u - d) + tail, FIRST))
    for size in (u - 4, u, u + 4, 2 * u + 1, 5 * u):
        if size >= 36:
            out.append(("%s-records-of-%d" % (tag, size), HDR + rec(40) + rec(size) * 3 + tail, FIRST))
    for r in range(36):  # the chain enters a segment at every residue
        out.append(("%s-entry-at-%d" % (tag, r), HDR + rec(u + r) + rec(36) * (u // 36 + 2) + rec(u + 36 - r) + tail, FIRST))
    for land in (u, 2 * u - 1, 2 * u, 3 * u - 1):  # a stop exactly at a segment's first / last position
        for bad in (31, 0x7FFFFFFF):
            s = HDR + rec(land) + rec(36) * 4
            out.append(("%s-stop-at-%d-%d" % (tag, land, bad), put_block(s, FIRST + land, bad), FIRST))
        out.append(("%s-end-at-%d" % (tag, land), HDR + rec(land) + bytes(3), FIRST))
        out.append(("%s-end-exactly-at-%d" % (tag, land), HDR + rec(land), FIRST))
    out.append(("%s-spans-a-whole-unit" % tag, HDR + rec(u // 2 + 36) + rec(2 * u + 7) + tail, FIRST))
    out.append(("%s-three-units" % tag, HDR + (rec(36) + rec(61) + rec(47)) * (3 * u // 144 + 1), FIRST))
    return out


def decoys():
    out = []
    for align in range(4):
        s = HDR + b"".join(rec(36 + 4 * k + align + n, bytes(32) + decoy_body(4 * k + align + n, (align + n) % 4, 4 - 3 * (n % 2)))
                           for n, k in enumerate((40, 3, 170, 0, 1000, 9, 64)))
        out.append(("decoys-%d" % align, s, FIRST))
        out.append(("decoys-%d-cut" % align, s[:-17], FIRST))
        out.append(("decoys-%d-from-inside" % align, s, FIRST + 36 + align))  # a start that is no record of the file
    inner = HDR + rec(36) * 5 + rec(100) + rec(36)
    for pad in range(4):
        s = HDR + rec(36) + rec(36 + pad + len(inner) + 5, bytes(32 + pad) + inner) + rec(36 + pad) + rec(32 + 4 + len(inner), bytes(32) + inner)
        out.append(("stream-inside-a-record-%d" % pad, s, FIRST))
    return out


def streams(seg, window):
    """every case for segments of `seg` bytes in windows of `window`; the names are unique"""
    out = basics() + geometry(seg, "seg") + decoys()
    if window != seg:
        out += geometry(window, "win")
    assert len({c[0] for c in out}) == len(out)
    return out


def library_walk(stream):
    """fqg_bam_index_records on the whole of `stream` (host side, no GPU): (offsets, used), or None where it refuses"""
    import ctypes as C

    import fastq_utils_amd as fq
    L = fq.abi.load()
    n, used = C.c_uint64(), C.c_uint64()
    if L.fqg_bam_index_records(stream, len(stream), None, 0, C.byref(n), C.byref(used)) != 0:
        return None
    offs = (C.c_uint64 * max(1, n.value))()
    assert L.fqg_bam_index_records(stream, len(stream), offs, n.value, C.byref(n), C.byref(used)) == 0
    return list(offs)[:n.value], used.value


def first_record(stream):
    """where fqg_bam_index_records starts its loop over the records - its first offset, or `used` when it finds none;
    None for a stream it refuses"""
    w = library_walk(stream)
    return None if w is None else (w[0][0] if w[0] else w[1])


def real_files():
    """the inflated stream of every .bam under tests/golden and bamgen.config4 with 1 000 alignments, each from the
    first record fqg_bam_index_records finds (a stream it refuses: from byte 0)"""
    import glob
    import gzip
    import os

    from tests import bamgen
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = []
    for path in sorted(glob.glob(os.path.join(gold, "**", "*.bam"), recursive=True)):
        try:
            s = gzip.decompress(open(path, "rb").read())
        except (OSError, EOFError):   # (a file that is damaged as a gzip file has no stream)
            continue
        out.append((os.path.relpath(path, gold), s, first_record(s) or 0))
    rec, *_ = bamgen.config4(np.random.default_rng(4), n_cells=30, n_genes=200, n_triples=770)
    assert 900 <= rec.shape[0] <= 1100
    s = bamgen.header() + rec.tobytes()
    out.append(("config4", s, first_record(s)))
    assert len(out) >= 31
    return out


def pack(cases):
    """the file the model reads: per stream its length, the first record and the bytes"""
    return b"".join(struct.pack("<QQ", len(s), first) + s for _, s, first in cases)


def unpack(blob, n_cases):
    """what the model writes: per stream n, used and n offsets"""
    out, at = [], 0
    for _ in range(n_cases):
        n, used = struct.unpack_from("<QQ", blob, at)
        offs = list(struct.unpack_from("<%dQ" % n, blob, at + 16))
        out.append((offs, used))
        at += 16 + 8 * n
    assert at == len(blob)
    return out
