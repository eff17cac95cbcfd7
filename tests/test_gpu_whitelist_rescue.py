"""fqg_barcodes_whitelist_correct (k_bc_whitelist_correct) against tests/whitelist_rescue_oracle.py: status, value and
counters per record, at the sizes where the wavefront's neighbour pass changes shape (4 * size probes over 64 lanes:
idle lanes, exactly 64, two passes), at record counts around one wavefront, and on hand-made whitelists.  With
max_mismatch 0 the status is fqg_barcodes_whitelist's `valid`."""
import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import whitelist_rescue_oracle as wro
from tests.test_gpu_whitelist import ALPHA, ends_at_the_image_end, make

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def image(seqs):
    return b"".join(b"@r%d 1:N:0:A\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def check(ctx, img, lines, offset, size, modes=(0, 1), packed=None):
    """every record of img, and every other one from the third on, under both modes; returns the statuses (mode 1)"""
    seqs = img.split(b"\n")[1::4]
    n = len(seqs)
    st = fq.abi.probe_first_record(img, False)
    r = ctx.validate(img, None, st, flags=fq.abi.VALIDATE_FRAME_ONLY)
    assert r["n_records"] == n
    frame = ctx.retain_frame()
    W = wro.members(lines) if packed is None else set(packed)
    w = fq.abi.Whitelist.from_lines(ctx, b"".join(ln + b"\n" for ln in lines)) if packed is None else fq.abi.Whitelist(ctx, packed)
    last = None
    try:
        for mm in modes:
            want = [wro.classify_read(s, offset, size, W, mm) for s in seqs]
            want_st = np.array([a for a, _ in want], dtype=np.uint8)
            want_v = np.array([b for _, b in want], dtype=np.uint64)
            got = ctx.barcodes_whitelist_correct(frame, w, offset, size, mm, want_status=True, want_cells=True)
            bad = np.nonzero((got["status"] != want_st) | (got["cells"] != want_v))[0]
            assert bad.size == 0, (mm, bad[:10], got["status"][bad[:10]], want_st[bad[:10]], [seqs[i] for i in bad[:3]])
            assert {k: got[k] for k in ("n_records", "n_exact", "n_rescued", "n_ambiguous", "n_short")} == wro.counts(want_st.tolist())
            if mm == 0:   # the exact kernel's answer, quirks included
                valid = ctx.barcodes_whitelist(frame, w, offset, size, want_flags=True)
                assert ((got["status"] == wro.EXACT) == (valid["valid"] == 1)).all()
                assert (got["n_exact"], got["n_short"]) == (valid["n_valid"], valid["n_short"])
            if n >= 6:    # every other record, from the third on
                m = (n - 2 + 1) // 2
                sub = ctx.barcodes_whitelist_correct(frame, w, offset, size, mm, n_records=m, first_record=2, step=2,
                                                     want_status=True, want_cells=True)
                assert (sub["status"] == want_st[2:2 + 2 * m:2]).all() and (sub["cells"] == want_v[2:2 + 2 * m:2]).all()
                assert {k: sub[k] for k in ("n_records", "n_exact", "n_rescued", "n_ambiguous", "n_short")} == wro.counts(want_st[2:2 + 2 * m:2].tolist())
            last = want_st
        # either array may be left out
        only = ctx.barcodes_whitelist_correct(frame, w, offset, size, modes[-1], want_status=True)
        assert (only["status"] == last).all() and "cells" not in only
        none = ctx.barcodes_whitelist_correct(frame, w, offset, size, modes[-1])
        assert none["n_exact"] == int((last == wro.EXACT).sum())
    finally:
        w.close()
        frame.release()
    return last


def whitelist_of(rng, size, n=300):
    return [ALPHA[rng.integers(0, 5, size)].tobytes() for _ in range(n)]


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("size", [1, 2, 15, 16, 17, 19])
def test_sizes_around_the_neighbour_pass(size, offset):
    rng = np.random.default_rng(size * 100 + offset)
    wl = whitelist_of(rng, size, 1 if size == 1 else 3 if size == 2 else 300)
    img, _ = make(rng, 5000, wl, size, offset)
    with fq.Context(0) as ctx:
        st = check(ctx, img, wl + [b"", wl[0]], offset, size)   # an empty line (0 is a member) and a repeat
    assert {wro.EXACT, wro.RESCUED} <= set(st.tolist())
    assert wro.SHORT in set(st.tolist()) or offset + size == 1   # (no read is shorter than one base)
    if size >= 15:
        assert wro.MISS in set(st.tolist())


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_record_counts_around_one_wavefront(n):
    rng = np.random.default_rng(n)
    wl = whitelist_of(rng, 16)
    img, _ = make(rng, n, wl, 16, 0)
    with fq.Context(0) as ctx:
        check(ctx, img, wl, 0, 16)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_a_barcode_in_the_last_bytes_of_the_image(n, offset):
    """the last record's barcode is fetched byte by byte (tests/test_gpu_whitelist.py: TAILS): a member, and an `A`
    beside the only member `C`; both modes, and max_mismatch 0 against fqg_barcodes_whitelist (check)"""
    rng = np.random.default_rng(10 * n + offset)
    with fq.Context(0) as ctx:
        for wl, last in (([b"A"], wro.EXACT), ([b"C"], wro.RESCUED)):
            img = ends_at_the_image_end(rng, n, wl, offset)
            assert check(ctx, img, wl, offset, 1, modes=(0,))[-1] == (wro.EXACT if last == wro.EXACT else wro.MISS)
            assert check(ctx, img, wl, offset, 1)[-1] == last


@pytest.mark.parametrize("size", [20, 56])
def test_beyond_19_characters_there_is_no_rescue_and_exact_is_unchanged(size):
    rng = np.random.default_rng(size)
    wl = whitelist_of(rng, size)
    img, _ = make(rng, 5000, wl, size, 0)
    with fq.Context(0) as ctx:
        check(ctx, img, wl + [b""], 0, size, modes=(0,))
        if size == 20:
            st = fq.abi.probe_first_record(img, False)
            ctx.validate(img, None, st, flags=fq.abi.VALIDATE_FRAME_ONLY)
            frame = ctx.retain_frame()
            w = fq.abi.Whitelist.from_lines(ctx, b"\n".join(wl) + b"\n")
            with pytest.raises(fq.abi.FqgError):
                ctx.barcodes_whitelist_correct(frame, w, 0, 20, 1)
            with pytest.raises(fq.abi.FqgError):
                ctx.barcodes_whitelist_correct(frame, w, 0, 16, 2)
            assert ctx.barcodes_whitelist_correct(frame, w, 0, 19, 1)["n_records"] == 5000
            w.close()
            frame.release()


def one_error(rng, w):
    b = bytearray(w)
    p = int(rng.integers(0, len(b)))
    b[p] = int(rng.choice([c for c in b"ACGT" if c != b[p]]))
    return bytes(b)


@pytest.mark.parametrize("kind", ["all_miss", "all_hit", "miss_in_lane_0", "miss_in_lane_63"])
def test_wavefronts_of_one_kind(kind):
    rng = np.random.default_rng(5)
    wl = sorted(set(whitelist_of(rng, 16, 200)))
    hits = [wl[int(rng.integers(0, len(wl)))] + b"ACGT" for _ in range(192)]
    if kind == "all_miss":     # rescued, and far from everything, in turns
        seqs = [(one_error(rng, h[:16]) if i % 2 else ALPHA[rng.integers(0, 4, 16)].tobytes()) + b"AC" for i, h in enumerate(hits)]
    elif kind == "all_hit":
        seqs = hits
    else:                      # the second wavefront of the first workgroup has one miss, in its first / last lane
        seqs = list(hits)
        at = 64 if kind == "miss_in_lane_0" else 127
        seqs[at] = one_error(rng, seqs[at][:16]) + b"ACGT"
    with fq.Context(0) as ctx:
        st = check(ctx, image(seqs), wl, 0, 16)
    if kind == "all_hit":
        assert (st == wro.EXACT).all()
    elif kind == "all_miss":
        assert (st != wro.EXACT).all() and (st[1::2] != wro.MISS).all()
    else:
        assert int((st != wro.EXACT).sum()) == 1 and st[64 if kind == "miss_in_lane_0" else 127] in (wro.RESCUED, wro.AMBIGUOUS)


HAND = {
    # name: (whitelist lines, size, reads, statuses with max_mismatch 1)
    "one_entry": ([b"ACGTACGT"], 8, [b"ACGTACGT", b"ACGTACGA", b"TCGTACGT", b"TCGTACGA", b"acgtacgn"],
                  [wro.EXACT, wro.RESCUED, wro.RESCUED, wro.MISS, wro.RESCUED]),
    "two_at_distance_2_and_a_read_between": ([b"AAAAAA", b"AACCAA"], 6, [b"AACAAA", b"AAACAA", b"AAAAAC"],
                                             [wro.AMBIGUOUS, wro.AMBIGUOUS, wro.RESCUED]),
    "two_at_distance_1_and_a_read_on_one": ([b"GGGGGG", b"GGGTGG"], 6, [b"GGGGGG", b"GGGTGG", b"GGGAGG"],
                                            [wro.EXACT, wro.EXACT, wro.AMBIGUOUS]),
    "an_entry_that_holds_n": ([b"ACNTAC"], 6, [b"ACNTAC", b"ACGTAC", b"acntaa", b"ACGTAA"],
                              [wro.EXACT, wro.RESCUED, wro.RESCUED, wro.MISS]),
    "a_read_with_n_beside_an_entry": ([b"ACGTAC"], 6, [b"ACGNAC", b"NCGTAC", b"ACGTAN", b"NCGTAN"],
                                      [wro.RESCUED, wro.RESCUED, wro.RESCUED, wro.MISS]),
    "an_empty_line_and_a_last_byte_that_is_no_base": ([b"ACGTAC", b""], 6, [b"ACGTAX", b"ACGTA.", b"ACXTAC", b"XCGTAC", b"ACGTAC"],
                                                      [wro.EXACT, wro.EXACT, wro.MISS, wro.MISS, wro.EXACT]),
    "the_same_entry_twice": ([b"CCCCCCCC", b"CCCCCCCC"], 8, [b"CCCCCCCC", b"CCCCACCC", b"CCCCAACC"],
                             [wro.EXACT, wro.RESCUED, wro.MISS]),
    "entries_of_another_length": ([b"ACGTA", b"ACGTACG", b"CGTAC"], 6, [b"ACGTAC", b"ACGTAA", b"CCGTAC", b"ACGTAX"],
                                  [wro.MISS, wro.MISS, wro.MISS, wro.MISS]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_whitelists(name):
    lines, size, reads, want = HAND[name]
    for offset in (0, 2):
        seqs = [b"TG"[:offset] + r + b"T" for r in reads] + [b"TG"[:offset] + reads[0][:size - 1]]   # and one too short
        with fq.Context(0) as ctx:
            st = check(ctx, image(seqs), lines, offset, size)
        assert st.tolist() == want + [wro.SHORT], (name, st.tolist())


def wl_hash(x):
    """the table's finaliser (wl_hash, fqg_barcode_kernels.hip)"""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x


def test_probe_chains_that_wrap_around_the_table():
    """Entries whose home is the table's LAST slot (1024 slots for up to 256 entries): the chain of the second one on
    wraps to slot 0, and so does every probe that looks for them - the exact look-up of a read that is one of them, the
    rescue probes of a read beside one of them, and a miss that starts there."""
    rng = np.random.default_rng(99)
    mask = 1023
    at_last = []
    while len(at_last) < 9:
        s = ALPHA[rng.integers(0, 4, 16)].tobytes()
        if wl_hash(wro.pack(s)) & mask == mask:
            at_last.append(s)
    wl, strangers = at_last[:6], at_last[6:]       # six members in slots 1023, 0, 1, 2, 3, 4; three misses that start at 1023
    filler = [ALPHA[rng.integers(0, 4, 16)].tobytes() for _ in range(100)]
    reads = list(wl) + strangers
    for w in wl:                                    # all 64 neighbours of every member (N excluded: 48) - rescued through the wrap
        for p in range(16):
            for c in b"ACGT":
                if c != w[p]:
                    reads.append(w[:p] + bytes([c]) + w[p + 1:])
    reads += filler[:20]
    with fq.Context(0) as ctx:
        st = check(ctx, image([r + b"AC" for r in reads]), wl + filler, 0, 16)
    assert (st[:6] == wro.EXACT).all() and (st[6:9] != wro.EXACT).all()
    assert (st[9:9 + 6 * 48] == wro.RESCUED).sum() >= 6 * 48 - 8   # (a neighbour may sit beside a filler entry as well)
