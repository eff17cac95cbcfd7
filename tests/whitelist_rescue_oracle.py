"""Whitelist rescue (fqg_barcodes_whitelist_correct, include/fqg.h) restated on packed integers.

s: the barcode string; P: char2uint_64 (oracle/umi_oracle.py; base 10, A C G T N in either case -> 1..5, from the end of
the string, stopping at the first other byte, modulo 2^64); W: the set of packed whitelist values.

  EXACT      P(s) in W (a string that packs to 0 is a member if 0 is); the value is P(s)
  RESCUED    not exact, max_mismatch == 1, every byte of s a base, exactly one k in W that is P(s) with one decimal
             digit replaced by another digit of 1..5; the value is k
  AMBIGUOUS  as above with two or more such k; no value
  MISS       everything else; no value
  SHORT      no barcode (the read is too short for offset + size)

An exact hit is never examined for neighbours."""
from oracle import umi_oracle as uo

MISS, EXACT, RESCUED, AMBIGUOUS, SHORT = 0, 1, 2, 3, 4
BASES = frozenset(b"ACGTNacgtn")
MAX_RESCUE_SIZE = 19  # digits that cannot wrap in 64 bits


def pack(s: bytes) -> int:
    return uo.char2uint_64(s + b"\n")


def members(lines) -> set:
    """W of a whitelist file's lines (an empty line packs to 0 and is a member like any other)"""
    return {pack(ln) for ln in lines}


def candidates(v: int, n: int, W) -> list:
    """the members that are v (n digits of 1..5) with one digit replaced by another of 1..5"""
    out = []
    for p in range(n):
        d = (v // 10 ** p) % 10
        for o in range(1, 6):
            if o != d:
                k = v + (o - d) * 10 ** p
                if k in W:
                    out.append(k)
    return out


def classify(s: bytes, W, max_mismatch: int):
    """(status, value) of a barcode string that is long enough"""
    assert max_mismatch in (0, 1) and (max_mismatch == 0 or len(s) <= MAX_RESCUE_SIZE)
    v = pack(s)
    if v in W:
        return EXACT, v
    if max_mismatch == 1 and s and all(c in BASES for c in s):
        c = candidates(v, len(s), W)
        if len(c) == 1:
            return RESCUED, c[0]
        if len(c) >= 2:
            return AMBIGUOUS, 0
    return MISS, 0


def classify_read(seq: bytes, offset: int, size: int, W, max_mismatch: int):
    """the `size` bytes at `offset` of a sequence line (get_barcode's bounds: a line too short has no barcode)"""
    if offset + size > len(seq):
        return SHORT, 0
    return classify(seq[offset:offset + size], W, max_mismatch)


def counts(statuses) -> dict:
    st = list(statuses)
    return {"n_records": len(st), "n_exact": st.count(EXACT), "n_rescued": st.count(RESCUED),
            "n_ambiguous": st.count(AMBIGUOUS), "n_short": st.count(SHORT)}


def census_filter(pairs, W, max_mismatch: int):
    """A plain census's (cell string, packed UMI) pairs -> what a census with the whitelist keeps, and its info counts.
    `pairs` holds the cell VALUE as the census packs it (bytes; b"" for a missing cell: cell 0)."""
    kept, info = [], {"exact": 0, "rescued": 0, "ambiguous": 0, "dropped": 0}
    for cell, umi in pairs:
        st, v = classify(cell, W, max_mismatch)
        if st == EXACT:
            info["exact"] += 1
        elif st == RESCUED:
            info["rescued"] += 1
        else:
            info["dropped"] += 1
            info["ambiguous"] += st == AMBIGUOUS
        if st in (EXACT, RESCUED):
            kept.append((v, umi))
    return kept, info
