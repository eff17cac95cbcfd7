"""The kernels of fqg_filter_kernels.hip at their own edges: seeded families of images for fqg_records_filter (both
modes) and of lists for fqg_records_gather, what each call must give, and the check.  Shared by
tests/test_filter_cases.py (no GPU: the generators show the properties they claim, the expectations are the oracle's)
and tests/test_gpu_filter_kernels.py (the families in its own process at the default tile size, and as
`python -m tests.filter_cases GROUP` under another FQGPU_BC_LDS or FQGPU_TILE_WAVES - the library reads both once).

No reference binary, no golden file.  What a filter call must give comes from oracle/filter_oracle.py record by
record: trim_record for the trim, the N rule of filter_n (len(seq) * max_n // 100 with the '\\n' counted, max_n clamped
to 100), _cstr for images with NUL bytes.  What a gather must give is the listed records joined.

Left out: a line that BEGINS with NUL (the host loop ends the file there, fq_filter_run.h), and with it the record that
has no quality line at all (a last record whose empty quality line has no newline is three lines: a truncated file).
Included although the reference is undefined there: a quality line shorter than the poly-T head that is cut off - the
kernel and the oracle both print an empty quality.

Stale output: the text area of a context is reused from call to call.  Every compared call comes behind a gather of
ONE record of 2 MiB of '~' (a byte no case holds, and two newlines: at byte 2 and at the end), so a kernel that fails
to write a byte finds '~' there and not the right byte of an earlier call.

The fit rule of a tile stands twice in the kernels (k_rf_tile_flags, bc_span_plan) and a third time here
(direct_tiles): `n <= in_cap and ((skew + n + 15) >> 4) * 16 + 32 <= in_cap`, skew = the span's start modulo 16 (the
image is 16-byte aligned on the device).  Every call on an image without NUL bytes must report exactly that many direct
tiles through fqg_records_filter_info, with T, in_cap and out_cap as tile_for gives them.  The third term of the
kernel's flag, `sum + 32 > out_cap`, cannot hold for a filter WHERE out_cap >= in_cap: a record's output is never longer
than its input (a trimmed quality gains a '\\n' only where the sequence lost at least one base), so a span that fits has
sum + 32 <= n + 32 <= in_cap.  That holds for the tile_edge images at all three budgets (9168 / 15408, 1536 / 2560,
10272 / 55264 bytes; the check asserts it from the reported values, and that the output term changes no flag there).
It does not hold everywhere: bc_tile_for only keeps in_cap <= budget - 1024, and at FQGPU_BC_LDS=4096 the tile_mix images
with a long record have T = 1, in_cap 2320, out_cap 1776 - a kept record of 1745 to 2288 bytes is direct by its
output alone.  So the expected count of every other family carries the third term, from the oracle's output lengths.
"""
import functools
import itertools
import json
import os
import sys

import numpy as np

from oracle import filter_oracle as fo

FILTER_N, FILTER_POLY_AT = 1, 2
DEFAULT_BUDGET = 24576  # bytes of LDS per wavefront (fqg_records_filter's call of bc_tile_for)
ERR_ARG = "libfqgpu error -3:"
POISON = b"@~\n" + b"~" * (2 << 20) + b"\n+\n~\n"
# quality bytes: neither N nor n (a neighbour of the sequence line that must not count), nor the '~' of the stale text
QA = bytes(c for c in range(33, 126) if c not in (78, 110))


def qual(n, phase=0):
    """n quality bytes, neighbours distinct (a shift shows)"""
    return bytes(QA[(phase + i) % len(QA)] for i in range(n))


def bases(n, phase=0):
    return (b"ACGT" * (n // 4 + 2))[phase % 4:phase % 4 + n]


def rec(h, s, q, plus=b"+"):
    return h + b"\n" + s + b"\n" + plus + b"\n" + q + b"\n"


def lines_of(image):
    parts = image.split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def records_of(image):
    """the records as four lines each, every line with its '\\n' (the file's last line may have none)"""
    ln = lines_of(image)
    assert len(ln) % 4 == 0 and ln, len(ln)
    return [tuple(ln[i:i + 4]) for i in range(0, len(ln), 4)]


def budget_of(env=os.environ):
    v = int(env.get("FQGPU_BC_LDS") or 0)
    return v if 4096 <= v <= 65536 else DEFAULT_BUDGET


def tile_for(nbytes, n_records, budget):
    """bc_tile_for (fqg_barcode_abi.inc) for one FASTQ input that is printed as FASTQ -> (T, in_cap, out_cap)"""
    r = nbytes / n_records
    t = (budget - (48.0 + 96.0)) / (1.06 * (r + (r + 100)) + 1.0)
    T = int(max(1.0, min(t, 64.0)))
    in_cap = (int(1.06 * r * T + 48.0 + 48.0) + 15) & ~15
    if in_cap + 1024 > budget:
        in_cap = (budget // 2) & ~15
    return T, in_cap, (budget - in_cap) & ~15


def fits(skew, nbytes, in_cap):
    return nbytes <= in_cap and ((skew + nbytes + 15) >> 4) * 16 + 32 <= in_cap


def direct_tiles(records, first, n, T, in_cap, out_cap=None, out_lens=None):
    """the fit rule, per tile of records [first, first + n): 1 = the span does not fit the tile's input area - or, with
    out_cap and the output bytes of every record of the range, its output does not fit the output area"""
    at = [0]
    for r in records:
        at.append(at[-1] + sum(map(len, r)))
    out = []
    for k0 in range(first, first + n, T):
        k1 = min(k0 + T, first + n)
        fit = fits(at[k0] % 16, at[k1] - at[k0], in_cap)
        if fit and out_cap is not None:
            fit = sum(out_lens[k0 - first:k1 - first]) + 32 <= out_cap
        out.append(0 if fit else 1)
    return out


# ---- what a call must give -------------------------------------------------------------------------------------------
def expect_filter(records, mode, max_n=0, min_poly=10, min_len=10):
    out, lens, trimmed, discarded = [], [], 0, 0
    for r in records:
        h1, seq, h2, q = (fo._cstr(x) for x in r)
        if mode == FILTER_N:
            body = seq.split(b"\n")[0]
            keep = body.count(b"N") + body.count(b"n") <= len(seq) * min(max_n, 100) // 100
            piece = h1 + seq + h2 + q
        else:
            nseq, nq, read_len, was = fo.trim_record(seq, q, min_poly)
            trimmed += 1 if was else 0
            keep = read_len >= (min_len & 0xFFFFFFFFFFFFFFFF)
            piece = h1 + nseq + h2 + (nq if nq is not None else b"")  # (None: Lq < matched2, see the module's text)
        discarded += 0 if keep else 1
        lens.append(len(piece) if keep else 0)
        if keep:
            out.append(piece)
    text = b"".join(out)
    return {"text": text, "lens": lens, "n_records": len(records), "n_kept": len(records) - discarded, "n_trimmed": trimmed,
            "n_discarded": discarded, "out_bytes": len(text)}


def expect_gather(records, order, nul=False):
    if nul:  # (what gzputs writes of a line is the C string)
        return b"".join(b"".join(fo._cstr(x) for x in records[int(k)]) for k in order)
    return b"".join(b"".join(records[int(k)]) for k in order)


def call(mode, first=0, n=None, **kw):
    return dict({"mode": mode, "first": first, "n": n}, **kw)


def N(max_n, **kw):
    return call(FILTER_N, max_n=max_n, **kw)


def P(min_poly, min_len, **kw):
    return call(FILTER_POLY_AT, min_poly=min_poly, min_len=min_len, **kw)


def params_of(c):
    return {k: c[k] for k in ("max_n", "min_poly", "min_len") if k in c}


def fcase(name, image, calls, **kw):
    return dict({"kind": "filter", "name": name, "image": image, "calls": calls}, **kw)


def gcase(name, image, lists, nul=False):
    return {"kind": "gather", "name": name, "image": image, "lists": lists, "nul": nul}


def want_of(case, c):
    recs = records_of(case["image"])
    n = len(recs) - c["first"] if c["n"] is None else c["n"]
    return expect_filter(recs[c["first"]:c["first"] + n], c["mode"], **params_of(c))


class Img:
    """records appended one by one; `at` = the offset the next record starts at"""

    def __init__(self):
        self.parts, self.at = [], 0

    def add(self, h, s, q, plus=b"+"):
        self.parts.append(rec(h, s, q, plus))
        self.at += len(self.parts[-1])
        return len(self.parts) - 1

    def header_to(self, residue, tail):
        """a header line after which the sequence line starts at `residue` modulo 16"""
        pad = (residue - (self.at + 1 + len(tail) + 1)) % 16
        h = b"@" + b"h" * pad + tail
        assert (self.at + len(h) + 1) % 16 == residue
        return h

    def image(self):
        return b"".join(self.parts)


# ---- FILTER_N --------------------------------------------------------------------------------------------------------
N_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def n_positions(pre, L):
    """first byte, last byte, and each side of every 16-byte boundary of the pieces (they lie on the image's own
    alignment; the 32-byte halves of a lane and the 256 bytes of a round of eight lanes are multiples of them)"""
    return sorted({0, L - 1} | {p + d for p in range(1, L) if (pre + p) % 16 == 0 for d in (-1, 0)}) if L else []


@functools.lru_cache(None)
def n_alignment(budget=DEFAULT_BUDGET):
    a, b = Img(), Img()
    seen = set()
    for pre in range(16):
        for L in sorted(set(N_LENGTHS) | {x - pre for x in (16, 32, 256) if x - pre > 0}):
            # (a) no N in the sequence, N and n all around it
            a.add(a.header_to(pre, b"NnNnNnNnNnNnNnNn"), bases(L, pre + L), (b"Nn" * 300)[pre % 2:pre % 2 + max(L, 13)], plus=b"+")
            seen.add((pre, L))
            # (b) clean neighbours, one N or n
            for j, p in enumerate(n_positions(pre, L)):
                s = bytearray(bases(L, p))
                s[p:p + 1] = b"Nn"[(j + pre) % 2:(j + pre) % 2 + 1]
                b.add(b.header_to(pre, b"ok_header_0123"), bytes(s), qual(min(L, 20), p))
    assert len(seen) >= 16 * len(N_LENGTHS)
    ca = fcase("n_alignment_poisoned_neighbours", a.image(), [N(0)])
    cb = fcase("n_alignment_one_n", b.image(), [N(0)])
    wa, wb = want_of(ca, ca["calls"][0]), want_of(cb, cb["calls"][0])
    assert wa["n_discarded"] == 0 and wb["n_kept"] == 0 and wb["n_records"] > 1000
    return [ca, cb]


N_THRESHOLDS = (1, 5, 33, 50, 99, 100, 250)


@functools.lru_cache(None)
def n_threshold(budget=DEFAULT_BUDGET):
    rng = np.random.default_rng(20261020)
    out = []
    for max_n in N_THRESHOLDS:
        im, both = Img(), set()
        for L in range(1, 301):
            allowed = (L + 1) * min(max_n, 100) // 100  # read_len counts the '\n'
            for extra in (0, 1):
                cnt = min(allowed, L) + extra  # (at 100 % the '\n' allows one N more than there are bases)
                if cnt > L:
                    continue
                s = bytearray(bases(L, L))
                style = len(im.parts) % 3
                for p in rng.choice(L, cnt, replace=False):
                    s[p] = (78, 110, 78 if p % 2 else 110)[style]
                im.add(b"@t%d_%d" % (L, extra), bytes(s), qual(L, L))
                both.add(extra)
        assert both == ({0, 1} if max_n < 100 else {0}), (max_n, both)
        c = fcase("n_threshold_%d" % max_n, im.image(), [N(max_n)])
        w = want_of(c, c["calls"][0])
        assert w["n_discarded"] == sum(1 for L in range(1, 301) if (L + 1) * min(max_n, 100) // 100 + 1 <= L) * (max_n < 100)
        out.append(c)
    return out


N_GROUPS = (1, 7, 8, 9, 63, 64, 65, 255, 257, 2051)


@functools.lru_cache(None)
def n_groups(budget=DEFAULT_BUDGET):
    out = []
    for n in N_GROUPS:
        im = Img()
        for i in range(n):  # discard and keep alternate (one wavefront takes eight records, the clamped lanes read the last)
            s = bytearray(bases(5 + i % 23, i))
            if i % 2 == 0:
                s[i % len(s)] = 78
            im.add(b"@g%d" % i, bytes(s), qual(len(s), i))
        c = fcase("n_groups_%d" % n, im.image(), [N(0)])
        assert want_of(c, c["calls"][0])["n_discarded"] == (n + 1) // 2
        out.append(c)
    # one long record among short ones, its only N in its last byte: the ballot loop runs on for one group alone
    im = Img()
    for i in range(40):
        L = 5000 if i == 19 else 30
        s = bytearray(bases(L, i))
        if i == 19:
            s[4999] = 78
        im.add(b"@l%d" % i, bytes(s), qual(L, i))
    c = fcase("n_groups_one_long_record", im.image(), [N(0), N(1)])
    assert want_of(c, c["calls"][0])["n_discarded"] == 1 and want_of(c, c["calls"][1])["n_discarded"] == 0
    return out + [c]


# ---- records of the tile, range and NUL families: reads with N, poly-A tails and poly-T heads ---------------------
def read_of(rng, i, L):
    s = bytearray(np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, L, p=[0.245, 0.245, 0.245, 0.245, 0.02])].tobytes())
    if i % 5 == 0:
        s[max(0, L - 12):] = b"A" * min(L, 12)
    elif i % 7 == 0:
        s[:9] = b"T" * min(L, 9)
    return bytes(s)


RANGES = ((0, 2051), (1, 8), (5, 3), (2046, 5), (2047, 4), (2051, 0), (64, 1987), (5, 3))
RANGES_REFUSED = ((0, 2052), (2051, 1), (2052, 0), (10, 2 ** 63), (1, 2 ** 64 - 1))


@functools.lru_cache(None)
def ranges(budget=DEFAULT_BUDGET):
    rng = np.random.default_rng(7)
    im = Img()
    for i in range(2051):
        L = int(rng.integers(1, 121))
        im.add(b"@r%d" % i, read_of(rng, i, L), qual(L, i))
    calls = [f(first=a, n=n) for a, n in RANGES for f in (lambda **kw: N(3, **kw), lambda **kw: P(6, 20, **kw))]
    c = fcase("ranges", im.image(), calls, refused=RANGES_REFUSED)
    w = [want_of(c, x) for x in calls]
    assert all(0 < x["n_discarded"] < x["n_records"] for x in w[:2]) and 0 < w[1]["n_trimmed"]
    return [c]


# ---- FILTER_POLY_AT --------------------------------------------------------------------------------------------------
POLY_SETTINGS = ((1, 0), (2, 1), (3, 3), (5, 10), (0, 4), (-1, 0), (3, -1))
POLY_PINNED = {"n_trimmed": (7775, 5439, 3569, 1235, 0), "n_discarded": (0, 0, 2466, 9331, 43)}


@functools.lru_cache(None)
def poly_exhaustive(budget=DEFAULT_BUDGET):
    out = []
    for name, alphabet, longest in (("ATNCan", b"ATNCan", 5), ("TtNnG", b"TtNnG", 4)):
        parts = []
        for L in range(longest + 1):
            for t in itertools.product(alphabet, repeat=L):
                parts.append(rec(b"@e", bytes(t), qual(L, len(parts))))
        out.append(fcase("poly_exhaustive_" + name, b"".join(parts), [P(a, b) for a, b in POLY_SETTINGS]))
    assert len(records_of(out[0]["image"])) == 9331 and len(out[0]["image"]) == 154897
    return out


def poly_branches(seq, q, min_poly):
    """which branches of rf_decide a record takes (seq and q with their '\\n')"""
    L, Lq = len(seq), len(q)
    m1 = 0
    while L - 2 - m1 >= 0 and seq[L - 2 - m1:L - 1 - m1] in (b"N", b"A", b"n", b"a"):
        m1 += 1
    if m1 >= min_poly:
        keep = L - 1 - m1
        return {"keep<Lq" if keep < Lq else "keep==Lq" if keep == Lq else "keep>Lq"}
    m2 = 0
    while m2 < L and seq[m2:m2 + 1] in (b"N", b"T", b"n", b"t"):
        m2 += 1
    if m2 >= min_poly:
        return {"Lq<matched2" if Lq < m2 else "Lq<=L" if Lq <= L else "Lq>L" if Lq - (L - m2 + 1) > 0 else "Lq>L,empty"}
    return {"untrimmed"}


POLY_QL_SEQS = (b"TTTTACGTAAAA", b"TTTTACGTAC", b"ACGTAAAA", b"AAAA", b"TTTT")
POLY_QL_BRANCHES = {"keep<Lq", "keep==Lq", "keep>Lq", "Lq<matched2", "Lq<=L", "Lq>L"}


@functools.lru_cache(None)
def poly_quality_lengths(budget=DEFAULT_BUDGET):
    im, seen, singles = Img(), set(), []
    for si, s in enumerate(POLY_QL_SEQS):
        for ql in range(len(s) + 1 + 8 + 1):  # 0 .. L + 8, L = the sequence with its '\n'
            im.add(b"@q%d_%d" % (si, ql), s, qual(ql, 7 * si + ql))
            seen |= poly_branches(s + b"\n", qual(ql) + b"\n", 4)
            if ql:  # (without a quality line the record has three lines: see the module's text)
                singles.append((si, ql))
                seen |= poly_branches(s + b"\n", qual(ql), 4)
    assert POLY_QL_BRANCHES <= seen, seen
    out = [fcase("poly_quality_lengths", im.image(), [P(4, 0), P(4, 6)])]
    # each once more as the file's last record, without a final newline (behind a few complete records)
    front = im.parts[3] + im.parts[40] + im.parts[17]
    for si, ql in singles:
        last = rec(b"@last%d_%d" % (si, ql), POLY_QL_SEQS[si], qual(ql, si + ql))[:-1]
        out.append(fcase("poly_quality_lengths_last_%d_%d" % (si, ql), front + last, [P(4, 0)]))
    return out


@functools.lru_cache(None)
def poly_runs(budget=DEFAULT_BUDGET):
    mp = 5
    im = Img()
    core = lambda n, i: (b"CGGCCG" * (n // 6 + 2))[i % 6:i % 6 + n]
    # runs of min_poly - 1, min_poly, min_poly + 1 at either end and at both (the A end wins)
    for t in (0, mp - 1, mp, mp + 1):
        for a in (0, mp - 1, mp, mp + 1):
            for A_, T_ in ((b"A", b"T"), (b"a", b"t"), (b"N", b"n")):
                s = T_ * t + core(17, t + a) + A_ * a
                im.add(b"@run_t%d_a%d" % (t, a), s, qual(len(s), t * 7 + a))
    # all A, all T
    for n in (1, 2, 63, 64, 1000, 9000):
        for ch in (b"A", b"T"):
            im.add(b"@all%s%d" % (ch, n), ch * n, qual(n, n))
    # read_len exactly min_len and one less, after an A trim, after a T trim and untrimmed (min_len 20: 19 and 18 bases + '\n')
    for keep in (19, 18):
        im.add(b"@len_a%d" % keep, core(keep, 1) + b"A" * 7, qual(keep + 7, keep))
        im.add(b"@len_t%d" % keep, b"T" * 6 + core(keep, 2), qual(keep + 6, keep))
        im.add(b"@len_u%d" % keep, core(keep, 3), qual(keep, keep))
    calls = [P(mp, 20), P(mp, 1), P(mp, 0), P(1, 0), P(64, 1), P(65, 2), P(mp, 19)]
    c = fcase("poly_runs", im.image(), calls, some_direct=True)  # (the reads of 9 000 bases: the direct path)
    w20, w19 = want_of(c, calls[0]), want_of(c, calls[6])
    recs = records_of(c["image"])
    names = [r[0] for r in recs]
    gone = lambda w: {names[i] for i, n in enumerate(w["lens"]) if n == 0}
    assert {b"@len_a18\n", b"@len_t18\n", b"@len_u18\n"} <= gone(w20) and not {b"@len_a19\n", b"@len_t19\n", b"@len_u19\n"} & gone(w20)
    assert not {b"@len_a18\n", b"@len_t18\n", b"@len_u18\n"} & gone(w19)
    for t in (0, mp - 1, mp, mp + 1):
        for a in (0, mp - 1, mp, mp + 1):
            s = [r for r in recs if r[0] == b"@run_t%d_a%d\n" % (t, a)][0]
            ns, _, _, was = fo.trim_record(s[1], s[3], mp)
            assert was == (a >= mp or t >= mp) and (a < mp or ns.startswith(s[1][:t + 17])) and (a >= mp or t < mp or ns == s[1][t:])
    return [c]


def with_nuls(parts, where):
    """parts: records as bytes; where: (record, line, offset inside the line) -> a NUL byte there"""
    parts = list(parts)
    for k, line, at in where:
        ln = parts[k].split(b"\n")
        assert 0 < at < len(ln[line])  # (never a line's first byte)
        ln[line] = ln[line][:at] + b"\0" + ln[line][at + 1:]
        parts[k] = b"\n".join(ln)
    return parts


@functools.lru_cache(None)
def nul_images(budget=DEFAULT_BUDGET):
    rng = np.random.default_rng(11)
    im = Img()
    for i in range(150):
        L = int(rng.integers(30, 90))
        im.add(b"@nul_%d text" % i, read_of(rng, i, L), qual(L, i))
    # header, sequence (also inside the A run of records 10 and 75, and in front of it), quality
    in_run = lambda k: len(im.parts[k].split(b"\n")[1]) - 5
    assert all(im.parts[k].split(b"\n")[1].endswith(b"A" * 12) for k in (10, 20, 75))
    where = ((3, 0, 4), (10, 1, in_run(10)), (11, 3, 9), (20, 1, 3), (40, 0, 7), (75, 1, in_run(75)), (76, 3, 1), (118, 3, 20), (149, 0, 2),
             (149, 1, 10))
    image = b"".join(with_nuls(im.parts, where))
    assert image.count(b"\0") == len(where) and len(fo._lines4(image)[0]) == 150
    return [fcase("nul_images", image, [N(3), N(0), P(6, 20), P(3, 0)], nul=True)]


# ---- tiles -------------------------------------------------------------------------------------------------------------
TILE_CALLS = (N(3), P(6, 8))


def sized_read(rng, i, size, tag=b"e"):
    """a record of exactly `size` bytes (>= 14)"""
    s = (size - 12) // 2
    return rec(b"@" + tag + b"%05d" % i + b"x" * ((size - 12) % 2), read_of(rng, i, s), qual(s, i))


@functools.lru_cache(None)
def tile_edge(budget=DEFAULT_BUDGET):
    """48 images of the same size and record count: tile 1 grows byte by byte across the edge of the input area through
    one longer record, tile 4 shrinks by as much"""
    R, tiles = 150, 6
    T, in_cap, _ = tile_for(R, 1, budget)
    n = tiles * T
    grow = next(d for d in range(in_cap) if not fits((R * T) % 16, R * T + d, in_cap))  # tile 1 starts at byte R * T
    out, sweep = [], []
    for v in range(48):
        d = max(0, grow - 24) + v
        rng = np.random.default_rng(3)
        sizes = [R] * n
        sizes[T + T // 2] += d
        for j in range(T):
            sizes[4 * T + j] -= d // T + (1 if j < d % T else 0)
        assert sum(sizes) == R * n and min(sizes) >= 14
        image = b"".join(sized_read(rng, i, sz) for i, sz in enumerate(sizes))
        assert tile_for(len(image), n, budget)[:2] == (T, in_cap)  # (nbytes / n_records has not moved)
        sweep.append(sum(direct_tiles(records_of(image), 0, n, T, in_cap)))
        out.append(fcase("tile_edge_%d" % d, image, list(TILE_CALLS), tile=(T, in_cap), out_ge_in=True))
    assert set(sweep) == {0, 1} and sweep == sorted(sweep), sweep
    return out


def tiled_image(seed, budget, k, d, direct, lens=(1, 600), big_len=None):
    """k * T + d records of random lengths; the tiles listed in `direct` (negative: from the end) hold one record that
    is long enough to push its tile over the input area (big_len: that long).  T depends on the mean record size and
    so on the image: built until it stands (None: it does not)."""
    m0 = lens[0] + lens[1] + 10  # mean bytes of a record
    T = 32
    for _ in range(12):
        n = k * T + d
        if n < 1:
            return None
        tiles = (n + T - 1) // T
        big_at = {min((t % tiles) * T + min(1, T - 1), n - 1) for t in direct}
        rng = np.random.default_rng(seed)
        parts = []
        for i in range(n):
            L = int(rng.integers(lens[0], lens[1] + 1))
            pad = int(rng.integers(0, 8))
            if i in big_at:
                L = big_len or int(2 * (0.06 * T * m0 + m0 + 96)) + 400
            parts.append(rec(b"@m%d" % i + b"x" * pad, read_of(rng, i, L), qual(L, i)))
        image = b"".join(parts)
        T2, in_cap, _ = tile_for(len(image), n, budget)
        if T2 == T:
            return image, T, in_cap
        T = T2
    return None


def tiled_image_where(seed, budget, k, d, direct, holds, lens=(1, 600), big_len=None):
    """the first seed from `seed` on whose image has direct tiles where holds(flags) wants them (a tile of random
    lengths may miss the input area without a long record: the area is 1.06 mean tiles)"""
    for s in range(seed, seed + 400):
        made = tiled_image(s, budget, k, d, direct, lens, big_len)
        if made:
            recs = records_of(made[0])
            flags = direct_tiles(recs, 0, len(recs), made[1], made[2])
            if len(recs) == k * made[1] + d and holds(flags):
                return made + (flags,)
    raise AssertionError("no image for %r" % ((budget, k, d, direct),))


def tile_residues(case):
    """(span starts of the tiles modulo 16, per call the output offsets of the tiles modulo 16)"""
    recs = records_of(case["image"])
    T = case["tile"][0]
    at = list(itertools.accumulate([0] + [sum(map(len, r)) for r in recs]))
    starts = {at[k] % 16 for k in range(0, len(recs), T)}
    outs = []
    for c in case["calls"]:
        o = list(itertools.accumulate([0] + want_of(case, c)["lens"]))
        outs.append({o[k] % 16 for k in range(0, len(recs), T)})
    return starts, outs


def has_run(flags, pattern):
    return any(tuple(flags[i:i + len(pattern)]) == pattern for i in range(len(flags)))


# name, k, d (k * T + d records), tiles with a long record, what the flags of the tiles must show
TILE_MIX = (("first", 5, 0, (0,), lambda f: f[0] and not f[1]),
            ("last", 5, 0, (-1,), lambda f: f[-1] and not f[-2]),
            ("last_of_kT_plus_1", 5, 1, (-1,), lambda f: f[-1] and not f[-2]),
            ("two_in_a_row", 6, -1, (2, 3), lambda f: has_run(f, (0, 1, 1, 0))),
            ("between_staged", 5, 1, (1, 3), lambda f: has_run(f, (0, 1, 0, 1, 0))),
            ("all", 3, 0, (0, 1, 2), all),
            ("kT", 12, 0, (), lambda f: not f[0] and not f[-1]),
            ("kT_minus_1", 12, -1, (), lambda f: not f[0] and not f[-1]),
            ("kT_plus_1", 12, 1, (), lambda f: not f[0] and not f[-1]))


def output_edge(budget):
    """records of about 2 000 bytes among some of 1 600: at a budget of 4 096 bytes T is 1 and the output area is
    smaller than the input area, so a long record that is kept fits as input and not as output - the
    third term of the tile flag alone sends its tile the direct way.  At the other budgets: one more image."""
    rng = np.random.default_rng(77)
    parts = [rec(b"@o%d" % i, read_of(rng, i, L), qual(L, i)) for i in range(40) for L in [800 if i % 4 == 3 else 1000 - i % 9]]
    c = fcase("tile_mix_output_edge", b"".join(parts), list(TILE_CALLS))
    T, in_cap, out_cap = tile_for(len(c["image"]), 40, budget)
    c["tile"] = (T, in_cap)
    if budget == 4096:
        recs = records_of(c["image"])
        for x in c["calls"]:
            a, b = direct_tiles(recs, 0, 40, T, in_cap), direct_tiles(recs, 0, 40, T, in_cap, out_cap, want_of(c, x)["lens"])
            assert T == 1 and out_cap < in_cap and sum(a) < sum(b) < 40, (T, in_cap, out_cap, a, b)
    return c


@functools.lru_cache(None)
def tile_mix(budget=DEFAULT_BUDGET):
    for base in range(8):  # (until the tiles' starts in the image and in the output show every residue)
        out = []
        starts, outs = set(), [set() for _ in TILE_CALLS]
        for j, (name, k, d, direct, holds) in enumerate(TILE_MIX):
            big_len = budget // 2 if name in ("all", "last_of_kT_plus_1") else None
            image, T, in_cap, flags = tiled_image_where(1000 * j + 100000 * base, budget, k, d, direct, holds, big_len=big_len)
            c = fcase("tile_mix_" + name, image, list(TILE_CALLS), tile=(T, in_cap))
            s, o = tile_residues(c)
            starts |= s
            for a, b in zip(outs, o):
                a |= b
            out.append(c)
        if starts == set(range(16)) and all(o == set(range(16)) for o in outs):
            return out + [output_edge(budget)]
    raise AssertionError((starts, outs))


def waves_of(env=os.environ):
    return int(env.get("FQGPU_TILE_WAVES") or 0)


@functools.lru_cache(None)
def tile_walk(budget=DEFAULT_BUDGET, waves=2):
    """with FQGPU_TILE_WAVES = waves the grid of k_rf_emit_tile is `waves`: a wavefront walks 1 to 5 tiles"""
    out = []
    for j, tiles in enumerate((waves, waves + 1, 2 * waves, 2 * waves + 1, 3 * waves + 1, 5 * waves)):
        direct = tuple(sorted({t for t in (1, tiles - 2, tiles // 2) if 0 < t < tiles - 1}))[:2 if tiles < 8 else 3]
        holds = lambda f, tiles=tiles: len(f) == tiles and (tiles < 3 or (0 < sum(f) < tiles and not f[0] and not f[-1]))
        image, T, in_cap, flags = tiled_image_where(1000 * (10 * waves + j), budget, tiles, -1, direct, holds, lens=(20, 200))
        out.append(fcase("tile_walk_%d_tiles" % tiles, image, list(TILE_CALLS), tile=(T, in_cap), grid=min(waves, tiles), tiles=tiles))
    assert out[-1]["tiles"] >= 4 * out[-1]["grid"]
    return out


# ---- gather ----------------------------------------------------------------------------------------------------------
def sized_record(i, size):
    """a record of exactly `size` bytes (>= 9) whose bytes depend on i"""
    s = (size - 7 + 1) // 2
    r = rec(b"@g", bases(s, i), qual(size - 7 - s, 5 * i))
    assert len(r) == size
    return r


SPAN_M = (1, 2, 63, 64, 65, 128, 129)
SPAN_BYTES = (10, 15, 16, 17, 1023, 1024, 1025, 3087, 3088, 3089, 4096, 4097, 8197, 70000)  # (10: the smallest record)
SMALLEST = 10


@functools.lru_cache(None)
def span(budget=DEFAULT_BUDGET):
    """every list: 64 records in falling order (the run's place in the output is arbitrary), then a run of neighbours"""
    parts, at = [], [0]

    def add(size):
        parts.append(sized_record(len(parts), size))
        at.append(at[-1] + size)
        return len(parts) - 1

    for _ in range(63):
        add(20)
    for x in range(16):
        add(SMALLEST + x)  # records 63 .. 78: one of them heads a list and sets the run's residue in the output
    blocks = []
    for m in SPAN_M:
        for B in SPAN_BYTES:
            if B < SMALLEST * m:
                continue
            add(SMALLEST + (len(blocks) * 7 - at[-1] - SMALLEST) % 16)  # the run's residue in the image
            sizes = [SMALLEST] * m
            sizes[m // 2] = B - SMALLEST * (m - 1)
            first = [add(sz) for sz in sizes][0]
            blocks.append((m, B, first))
    m, B = 64, 4097
    first = [add(sz) for sz in [SMALLEST] * 32 + [B - SMALLEST * 63] + [SMALLEST] * 31][0]
    blocks.append((m, B, first))  # ... and the run that ends in the file's last record, which has no newline
    image = b"".join(parts)[:-1]
    lists, src, dst = [], set(), set()
    for j, (m, B, first) in enumerate(blocks):
        head = [63 + j % 16] + list(range(62, -1, -1))
        lists.append(("run_%d_records_%d_bytes%s" % (m, B, "_unterminated" if j == len(blocks) - 1 else ""), head + list(range(first, first + m))))
        src.add(at[first] % 16)
        dst.add(sum(at[k + 1] - at[k] for k in head) % 16)
    assert src == set(range(16)) and dst == set(range(16)), (src, dst)
    run = next(first for m, B, first in blocks if (m, B) == (64, 1024))  # (inside the image: far from its end)
    lists.append(("broken_between_lanes_0_and_1", [5] + list(range(run, run + 63))))
    lists.append(("broken_between_the_last_two", list(range(run, run + 63)) + [6]))
    return [gcase("span", image, lists)]


PIECE_SIZES = (10, 15, 16, 17, 1023, 1024, 1025, 2048, 2049, 20000)


@functools.lru_cache(None)
def pieces(budget=DEFAULT_BUDGET):
    rng = np.random.default_rng(23)
    sizes = list(PIECE_SIZES) * 3 + [17]
    image = b"".join(sized_record(i, sz) for i, sz in enumerate(sizes))[:-1]
    last = len(sizes) - 1
    small = [i for i, sz in enumerate(sizes[:-1]) if sz <= 1024]
    large = [i for i, sz in enumerate(sizes[:-1]) if sz > 1024]
    lists = []
    for c in list(range(1, 10)) + [64]:  # the same record again and again
        for r in (3, 5, 6):
            lists.append(("record_%d_bytes_%d_times" % (sizes[r], c), [r] * c))
    for j, c in enumerate(list(range(1, 10)) + [63, 64, 65, 2051]):
        ls = [int(x) for x in rng.choice(small, c)]
        lists.append(("small_%d" % c, ls))  # four records at once
        one = list(ls)
        one[int(rng.integers(0, c))] = large[j % len(large)]
        lists.append(("one_large_%d" % c, one))  # the whole wavefront takes the loop for long records
    lists.append(("all_sizes_permuted", [int(x) for x in rng.permutation(last + 1)]))
    lists.append(("unterminated_last_in_the_middle", [0, last, 14, 4, last, 1]))
    lists.append(("unterminated_last_among_large", [large[0], last, 4]))
    return [gcase("pieces", image, lists)]


@functools.lru_cache(None)
def gather_nul(budget=DEFAULT_BUDGET):
    image = nul_images()[0]["image"]
    n = len(records_of(image))
    return [gcase("gather_nul", image, [("identity", list(range(n))), ("permutation", [int(x) for x in np.random.default_rng(2).permutation(n)])], nul=True)]


FAMILIES = {"n_alignment": n_alignment, "n_threshold": n_threshold, "n_groups": n_groups, "ranges": ranges,
            "poly_exhaustive": poly_exhaustive, "poly_quality_lengths": poly_quality_lengths, "poly_runs": poly_runs,
            "nul_images": nul_images, "tile_edge": tile_edge, "tile_mix": tile_mix, "tile_walk": tile_walk,
            "span": span, "pieces": pieces, "nul": gather_nul}
GROUPS = {"tiles": ("tile_edge", "tile_mix"), "walk": ("tile_walk",), "all": tuple(f for f in FAMILIES if f != "tile_walk")}


def cases_of(family, env=os.environ):
    if family == "tile_walk":
        return tile_walk(budget_of(env), waves_of(env) or 2)
    return FAMILIES[family](budget_of(env))


# ---- the check -------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self):
        import fastq_utils_amd as fq
        self.fq, self.A = fq, fq.abi
        self.ctx = fq.Context(0)
        self.budget, self.waves = budget_of(), waves_of()
        self.poison = self.frame_of(POISON)

    def close(self):
        self.poison.release()
        self.ctx.close()

    def frame_of(self, image):
        """as the programs make it (fq_filter_run.h)"""
        st = self.A.probe_first_record(image[:4096], True)
        r = self.ctx.validate(image, None, st, final=True, flags=self.A.VALIDATE_FRAME_ONLY)
        assert r["code"] == 0, r
        return self.ctx.retain_frame()

    def stale(self):
        nb, _ = self.ctx.records_gather(self.poison, np.zeros(1, dtype=np.uint64))
        assert nb == len(POISON)

    def check(self, case):
        """-> what is wrong, a list"""
        assert b"~" not in case["image"]
        fr = self.frame_of(case["image"])
        try:
            return (self.check_filter if case["kind"] == "filter" else self.check_gather)(case, fr)
        finally:
            fr.release()

    def check_filter(self, case, fr):
        bad = []
        recs = records_of(case["image"])
        if fr.n_records != len(recs):
            return ["%s: %d records framed, %d expected" % (case["name"], fr.n_records, len(recs))]
        for c in case["calls"]:
            n = len(recs) - c["first"] if c["n"] is None else c["n"]
            label = "%s %r" % (case["name"], {k: v for k, v in c.items() if v is not None})
            want = want_of(case, c)
            assert want["out_bytes"] < len(POISON)
            self.stale()
            kw = {{"max_n": "max_n_percent", "min_poly": "min_poly_at_len"}.get(k, k): v for k, v in params_of(c).items()}
            r = self.ctx.records_filter(fr, n, c["mode"], first_record=c["first"], **kw)
            info = self.ctx.records_filter_info()
            got = self.ctx.records_filter_output(r["out_bytes"])
            for k in ("n_records", "n_kept", "n_trimmed", "n_discarded", "out_bytes"):
                if r[k] != want[k]:
                    bad.append("%s: %s %d, expected %d" % (label, k, r[k], want[k]))
            if got != want["text"]:
                at = next((i for i, (a, b) in enumerate(zip(got, want["text"])) if a != b), min(len(got), len(want["text"])))
                bad.append("%s: %d bytes against %d expected, first difference at byte %d" % (label, len(got), len(want["text"]), at))
            bad += ["%s: %s" % (label, m) for m in self.info_wrong(case, c, recs, n, want, info)]
        for first, n in case.get("refused", ()):
            for mode in (FILTER_N, FILTER_POLY_AT):
                try:
                    self.ctx.records_filter(fr, n, mode, first_record=first)
                    bad.append("%s: no FQG_ERR_ARG for records %d, +%d" % (case["name"], first, n))
                except self.A.FqgError as e:
                    if ERR_ARG not in str(e):
                        raise
        return bad

    def info_wrong(self, case, c, recs, n, want, info):
        if n == 0:
            return [] if not any(info.values()) else ["info %r after a call without records" % info]
        T, in_cap, out_cap = tile_for(len(case["image"]), len(recs), self.budget)
        bad = []
        if (info["T"], info["in_cap"], info["out_cap"]) != (T, in_cap, out_cap):
            bad.append("info %r, expected T %d in_cap %d out_cap %d" % (info, T, in_cap, out_cap))
        if case.get("out_ge_in") and info["out_cap"] < info["in_cap"]:
            bad.append("info %r: the output area is smaller than the input area" % info)
        if "tile" in case and case["tile"] != (T, in_cap):
            bad.append("the case was made for T, in_cap %r" % (case["tile"],))
        flags = direct_tiles(recs, c["first"], n, T, in_cap, out_cap, want["lens"])
        if case.get("out_ge_in") and flags != direct_tiles(recs, c["first"], n, T, in_cap):
            bad.append("the output edge is reached")
        big = len(flags) if case.get("nul") else sum(flags)
        if info["tiles"] != len(flags) or info["big_tiles"] != big:
            bad.append("info %r, expected %d tiles, %d of them direct" % (info, len(flags), big))
        if case.get("some_direct") and not 0 < big < len(flags):
            bad.append("%d of %d tiles direct" % (big, len(flags)))
        if self.waves and want["out_bytes"] and info["grid"] != min(self.waves, len(flags)):
            bad.append("grid %d under FQGPU_TILE_WAVES=%d, %d tiles" % (info["grid"], self.waves, len(flags)))
        if not self.waves and want["out_bytes"] and not 0 < info["grid"] <= len(flags):
            bad.append("grid %d, %d tiles" % (info["grid"], len(flags)))
        if "grid" in case and self.waves and case["tiles"] != len(flags):
            bad.append("%d tiles, the case was made for %d" % (len(flags), case["tiles"]))
        return bad

    def check_gather(self, case, fr):
        bad = []
        recs = records_of(case["image"])
        if fr.n_records != len(recs):
            return ["%s: %d records framed, %d expected" % (case["name"], fr.n_records, len(recs))]
        for label, order in case["lists"]:
            want = expect_gather(recs, order, case["nul"])
            assert len(want) < len(POISON)
            self.stale()
            nb, got = self.ctx.records_gather(fr, np.asarray(order, dtype=np.uint64), want_output=True)
            if nb != len(want) or got != want:
                at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                bad.append("%s %s: %d bytes against %d expected, first difference at byte %d" % (case["name"], label, nb, len(want), at))
        return bad


def run_families(names, runner=None):
    """-> (number of cases, what is wrong)"""
    own = runner is None
    runner = runner or Runner()
    n, bad = 0, []
    try:
        for fam in names:
            for case in cases_of(fam):
                n += 1
                bad += runner.check(case)
    finally:
        if own:
            runner.close()
    return n, bad


def main(argv):
    group = argv[1]
    n, bad = run_families(GROUPS.get(group, (group,)))
    print(json.dumps({"group": group, "env": {k: os.environ.get(k) for k in ("FQGPU_BC_LDS", "FQGPU_TILE_WAVES")}, "cases": n,
                      "failed": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
