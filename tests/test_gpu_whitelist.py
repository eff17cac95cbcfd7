"""Whitelist membership of a barcode cut out of the reads (fqg_barcodes_whitelist; BASELINE configs[2]: "known_cells
whitelist") against the oracle's restatement of the reference: char2uint_64 (src/bam_umi_count.c:364-382) on the
barcode string, valid_barcode (:523-535) against what load_whitelist (:543-579) read from the file, and get_barcode's
bounds (src/fastq_pre_barcodes.c:232) for reads that are too short."""
import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import umi_oracle as uo

pytestmark = pytest.mark.gpu
ALPHA = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)


def make(rng, n, wl, size, offset):
    recs, want = [], []
    members = {uo.char2uint_64(w + b"\n") for w in wl}
    for i in range(n):
        ln = int(rng.integers(1, offset + size + 12))
        kind = rng.integers(0, 10)
        seq = bytearray(ALPHA[rng.integers(0, 4 if kind < 7 else 10, ln)].tobytes())
        if kind < 5 and ln >= offset + size:      # a whitelisted barcode (maybe in lower case, maybe with one error)
            w = bytearray(wl[int(rng.integers(0, len(wl)))])
            if kind == 1:
                w = bytearray(bytes(w).lower())
            if kind == 2:
                w[int(rng.integers(0, size))] = int(rng.choice(list(b"ACGTNX.")))
            seq[offset:offset + size] = w
        if kind == 9 and ln > offset:             # something that is no base inside the barcode: the packing stops there
            seq[offset + int(rng.integers(0, min(size, ln - offset)))] = int(rng.choice(list(b"X.-0 ")))
        q = (rng.integers(5, 40, ln) + 33).astype(np.uint8).tobytes()
        recs.append(b"@r%d 1:N:0:A\n%s\n+\n%s\n" % (i, bytes(seq), q))
        if offset + size > ln:
            want.append(0)
        else:
            want.append(1 if uo.char2uint_64(bytes(seq[offset:offset + size]) + b"\n") in members else 0)
    return b"".join(recs), np.array(want, dtype=np.uint8)


@pytest.mark.parametrize("size,offset", [(16, 0), (10, 16), (1, 0), (17, 3), (32, 0), (33, 5), (49, 1), (56, 0)])
def test_membership_matches_the_reference_semantics(size, offset):
    rng = np.random.default_rng(size * 100 + offset)
    wl = [ALPHA[rng.integers(0, 5, size)].tobytes() for _ in range(300)]
    wl_text = b"\n".join(wl) + b"\n\n" + wl[0] + b"\n"   # an empty line packs to 0 and is a member like any other; a repeat
    img, want = make(rng, 5000, wl, size, offset)
    want_zero_member = True  # "\n" -> 0 is in the table: a barcode that packs to 0 (first character from the end no base) is valid
    with fq.Context(0) as ctx:
        st = fq.abi.probe_first_record(img, False)
        r = ctx.validate(img, None, st, flags=fq.abi.VALIDATE_FRAME_ONLY)
        assert r["n_records"] == 5000
        frame = ctx.retain_frame()
        w = fq.abi.Whitelist.from_lines(ctx, wl_text)
        got = ctx.barcodes_whitelist(frame, w, offset, size, want_flags=True)
        # the oracle set holds 0 as well (the empty line): recompute `want` with it
        members = {uo.char2uint_64(x + b"\n") for x in wl} | {0}
        lines = img.split(b"\n")
        for i in range(5000):
            seq = lines[4 * i + 1]
            want[i] = 0 if offset + size > len(seq) else (1 if uo.char2uint_64(seq[offset:offset + size] + b"\n") in members else 0)
        assert want_zero_member and (got["valid"] == want).all(), np.nonzero(got["valid"] != want)[0][:10]
        assert got["n_valid"] == int(want.sum()) and got["n_records"] == 5000
        assert got["n_short"] == sum(1 for i in range(5000) if offset + size > len(lines[4 * i + 1]))
        # every other record, from the third on
        sub = ctx.barcodes_whitelist(frame, w, offset, size, n_records=2000, first_record=2, step=2, want_flags=True)
        assert (sub["valid"] == want[2:4002:2]).all()
        w.close()
        frame.release()


# The last record of a well-formed image whose barcode (one character at `offset`) has fewer than 8 bytes between its
# first byte and the image's end - 6 and 7: the kernels' fetch (wl_pack_at) takes such a word byte by byte
TAILS = {0: b"@r\nA\n+\nI\n", 1: b"@r\nCA\n+\nII\n"}


def ends_at_the_image_end(rng, n, wl, offset):
    """n records, the last of them TAILS[offset]"""
    return make(rng, n - 1, wl, 1, offset)[0] + TAILS[offset]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_a_barcode_in_the_last_bytes_of_the_image(n, offset):
    rng = np.random.default_rng(10 * n + offset)
    with fq.Context(0) as ctx:
        for wl in ([b"A"], [b"C"]):
            img = ends_at_the_image_end(rng, n, wl, offset)
            assert len(img) - (img.rindex(b"@r\n") + 3 + offset) == 6 + offset
            members = {uo.char2uint_64(x + b"\n") for x in wl}
            seqs = img.split(b"\n")[1::4]
            want = np.array([0 if offset + 1 > len(s) else int(uo.char2uint_64(s[offset:offset + 1] + b"\n") in members) for s in seqs],
                            dtype=np.uint8)
            assert len(seqs) == n and want[-1] == (wl == [b"A"])
            st = fq.abi.probe_first_record(img, False)
            assert ctx.validate(img, None, st, flags=fq.abi.VALIDATE_FRAME_ONLY)["n_records"] == n
            frame = ctx.retain_frame()
            w = fq.abi.Whitelist.from_lines(ctx, b"".join(x + b"\n" for x in wl))
            got = ctx.barcodes_whitelist(frame, w, offset, 1, want_flags=True)
            assert (got["valid"] == want).all(), np.nonzero(got["valid"] != want)[0][:10]
            assert (got["n_records"], got["n_valid"]) == (n, int(want.sum()))
            assert got["n_short"] == sum(1 for s in seqs if offset + 1 > len(s))
            assert ctx.barcodes_whitelist(frame, w, offset, 1)["n_valid"] == int(want.sum())   # ... without the bytes
            w.close()
            frame.release()


def test_the_reference_fixture_whitelist():
    """tests/golden/data_umi's known_cells file as load_whitelist reads it, against the oracle's packing"""
    import os
    from tests.util import GOLD
    path = os.path.join(GOLD, "data_umi", "known_cells.txt")
    if not os.path.exists(path):
        pytest.skip("fixture not present")
    text = open(path, "rb").read()
    cells = [ln for ln in text.split(b"\n") if ln]
    size = len(cells[0])
    rng = np.random.default_rng(1)
    recs = []
    for i in range(2000):
        bc = cells[i % len(cells)] if i % 3 else ALPHA[rng.integers(0, 4, size)].tobytes()
        recs.append(b"@x%d\n%s\n+\n%s\n" % (i, bc + b"ACGT", b"I" * (size + 4)))
    img = b"".join(recs)
    members = {uo.char2uint_64(c + b"\n") for c in cells}
    want = np.array([1 if uo.char2uint_64(img.split(b"\n")[4 * i + 1][:size] + b"\n") in members else 0 for i in range(2000)], dtype=np.uint8)
    with fq.Context(0) as ctx:
        st = fq.abi.probe_first_record(img, False)
        ctx.validate(img, None, st, flags=fq.abi.VALIDATE_FRAME_ONLY)
        frame = ctx.retain_frame()
        w = fq.abi.Whitelist.from_lines(ctx, text)
        got = ctx.barcodes_whitelist(frame, w, 0, size, want_flags=True)
        assert (got["valid"] == want).all() and got["n_valid"] == int(want.sum())
        w.close()
        frame.release()
