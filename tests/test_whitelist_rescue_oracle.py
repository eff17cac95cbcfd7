"""tests/whitelist_rescue_oracle.py (packed integers, digit arithmetic) against an independent formulation: brute-force
Hamming distance on the strings.  Base-only barcodes and whitelists, so that the two formulations speak about the same
thing: for such strings of one length, P is injective up to case, and 'one digit replaced by another of 1..5' is 'one
character replaced by another base'."""
import numpy as np
import pytest

from tests import whitelist_rescue_oracle as wro

UPPER = np.frombuffer(b"ACGTN", dtype=np.uint8)


def hamming(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a.upper(), b.upper()))


def by_strings(s: bytes, wl, max_mismatch):
    """wl: distinct upper-case base strings of len(s)"""
    near = [w for w in wl if hamming(s, w) <= 1]
    exact = [w for w in near if hamming(s, w) == 0]
    if exact:
        return wro.EXACT, wro.pack(exact[0])
    if max_mismatch == 1 and len(near) == 1:
        return wro.RESCUED, wro.pack(near[0])
    if max_mismatch == 1 and len(near) >= 2:
        return wro.AMBIGUOUS, 0
    return wro.MISS, 0


def draw(rng, size, n):
    return sorted({UPPER[rng.integers(0, 5, size)].tobytes() for _ in range(n)})


@pytest.mark.parametrize("size", [1, 2, 16, 19])
@pytest.mark.parametrize("max_mismatch", [0, 1])
def test_digits_agree_with_hamming_distance_on_strings(size, max_mismatch):
    rng = np.random.default_rng(size)
    wl = draw(rng, size, {1: 2, 2: 6}.get(size, 200))
    # neighbours of neighbours, so that reads between two members (ambiguous) exist at every size
    for w in list(wl[:40]) if size > 2 else []:
        b = bytearray(w)
        for _ in range(2):
            b[int(rng.integers(0, size))] = int(rng.choice(list(b"ACGTN")))
        wl.append(bytes(b))
    wl = sorted(set(wl))
    W = wro.members(wl)
    seen = set()
    for i in range(3000):
        s = bytearray(wl[int(rng.integers(0, len(wl)))] if i % 4 else UPPER[rng.integers(0, 5, size)].tobytes())
        for _ in range(int(rng.integers(0, 3))):   # 0, 1 or 2 substitutions; N on either side
            s[int(rng.integers(0, size))] = int(rng.choice(list(b"ACGTN")))
        s = bytes(s) if i % 3 else bytes(s).lower()
        got = wro.classify(s, W, max_mismatch)
        assert got == by_strings(s, wl, max_mismatch), (s, got)
        seen.add(got[0])
    if size > 2:   # (with one or two characters nearly everything is a neighbour of something)
        assert seen == ({wro.EXACT, wro.MISS} if max_mismatch == 0 else {wro.EXACT, wro.RESCUED, wro.AMBIGUOUS, wro.MISS}), seen


def test_an_exact_hit_is_never_examined_for_neighbours():
    W = wro.members([b"ACGT", b"ACGA", b"ACGC"])
    assert wro.classify(b"ACGT", W, 1) == (wro.EXACT, wro.pack(b"ACGT"))   # two members at distance 1: still exact
    assert wro.classify(b"ACGG", W, 1) == (wro.AMBIGUOUS, 0)
    assert wro.classify(b"ACGG", W, 0) == (wro.MISS, 0)
    assert wro.classify(b"TCGT", W, 1) == (wro.RESCUED, wro.pack(b"ACGT"))


def test_the_member_that_packs_to_zero():
    W = wro.members([b"ACGT", b""])          # an empty line of the file: 0 is a member
    assert 0 in W
    assert wro.classify(b"ACGX", W, 1) == (wro.EXACT, 0)     # the last byte is no base: packs to 0, exact by the quirk
    assert wro.classify(b"ACXT", W, 1) == (wro.MISS, 0)      # packs to 4 ("T"), no member; a non-base byte: no rescue
    assert wro.classify(b"ACGX", wro.members([b"ACGT"]), 1) == (wro.MISS, 0)
    # a member of another length is never a candidate: "CGA" and "ACGAA" are not one substitution away from "ACGA"
    assert wro.classify(b"ACGA", wro.members([b"CGA", b"ACGAA"]), 1) == (wro.MISS, 0)


def test_reads_too_short_have_no_barcode():
    W = wro.members([b"ACGT"])
    assert wro.classify_read(b"GGACGT", 2, 4, W, 1) == (wro.EXACT, wro.pack(b"ACGT"))
    assert wro.classify_read(b"GGACG", 2, 4, W, 1) == (wro.SHORT, 0)
    assert wro.counts([wro.EXACT, wro.SHORT, wro.MISS, wro.RESCUED, wro.RESCUED]) == {
        "n_records": 5, "n_exact": 1, "n_rescued": 2, "n_ambiguous": 0, "n_short": 1}
