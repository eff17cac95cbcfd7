"""Texts for the device deflate compressor (k_deflate_members, fastq_utils_amd/csrc/fqg_deflate_kernels.hip), each family
made to reach one thing the workgroup adds on top of tests/cxx/deflate_model.cpp, and each with a property that the model's
--report must show: property(family, reports) raises if the family is not what it says.  tests/test_deflate_codes.py
checks the properties (and zlib's reading of the model's bytes) without a GPU; tests/test_gpu_deflate.py and
tests/test_gpu_bgzf.py compare the device's bytes with the model's on the same texts.

Every generator is seeded: the texts are the same bytes on every machine.  Where a generator has to search (the ties, the
planted matches a later position may take the hash slot of, the window's planted copies) it asks the model, a bounded
number of times."""
import json
import os
import random
import struct
import subprocess
import tempfile

from tests.test_pgzip import fastq_text

M = 65280
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UBSAN = ["-fsanitize=undefined", "-fno-sanitize-recover=all"]


class Model:
    """tests/cxx/deflate_model.cpp, built into `workdir`; run(texts) -> ([gzip members of each text], [[report of each
    member] of each text]), all texts in one process"""

    def __init__(self, workdir, flags=()):
        self.dir = str(workdir)
        self.exe = os.path.join(self.dir, "deflate_model")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", self.exe,
                        os.path.join(ROOT, "tests", "cxx", "deflate_model.cpp"), "-lz"], check=True)
        self.runs = 0

    def run(self, texts, report=True):
        self.runs += 1
        src, dst, rep = (os.path.join(self.dir, "%s.%d" % (name, self.runs)) for name in ("in", "out", "report"))
        with open(src, "wb") as f:
            for t in texts:
                f.write(struct.pack("<I", len(t)))
                f.write(t)
        subprocess.run([self.exe, src, dst, "--records"] + (["--report", rep] if report else []), check=True, capture_output=True, timeout=600)
        with open(dst, "rb") as f:
            raw = f.read()
        out, at = [], 0
        while at < len(raw):
            size, = struct.unpack_from("<I", raw, at)
            out.append(raw[at + 4:at + 4 + size])
            at += 4 + size
        assert len(out) == len(texts) and at == len(raw)
        reports = [[] for _ in texts]
        if report:
            with open(rep) as f:
                for line in f:
                    r = json.loads(line)
                    assert r["member"] == len(reports[r["text"]])
                    reports[r["text"]].append(r)
            os.unlink(rep)
        os.unlink(src)
        os.unlink(dst)
        return out, reports


def noise(seed, n):
    return random.Random(seed).randbytes(n)


# ---------------------------------------------------------------------------------------------------------------- sizes

def size_values():
    """0..600 without a gap; the multiples of 255 (a CRC stripe) and 256 (a step) up to 2048 and their neighbours; the
    sizes below a full member at which the last stripe, the last step, the last wavefront and the last word change"""
    ns = set(range(601))
    for unit in (255, 256):
        for k in range(unit, 2049, unit):
            ns.update((k - 1, k, k + 1))
    ns.update((M - 257, M - 256, M - 255, M - 65, M - 64, M - 63, M - 62, M - 4, M - 3, M - 2, M - 1, M))
    return sorted(ns)


SIZE_CONTENTS = ("noise", "one_byte", "fastq", "period_5")


def sizes(content):
    """[text of every size_values()] of one content.  Property (over the four contents together): members of 64 bytes and
    less are written both stored and dynamic; every n mod 64 and every n mod 256 occurs with a dynamic block."""
    whole = {"noise": noise(21, M), "one_byte": b"A" * M, "fastq": fastq_text(700, 7)[:M], "period_5": (b"GATTC" * (M // 5 + 1))[:M]}[content]
    assert len(whole) == M
    return [whole[:n] for n in size_values()]


def sizes_property(reports_by_content):
    small, mod64, mod256 = set(), set(), set()
    for reports in reports_by_content.values():
        for (r,) in reports:
            if r["n"] <= 64:
                small.add(r["written"])
            if r["written"] == "dynamic":
                mod64.add(r["n"] % 64)
                mod256.add(r["n"] % 256)
    assert small == {"stored", "dynamic"}, small
    assert mod64 == set(range(64)) and mod256 == set(range(256))


# ------------------------------------------------------------------------------------------------------------------ tie

TIE_SIZES = (40, 300, 2000, M)


def tie(model, budget=160):
    """[(n, a, dyn_bytes - stored_bytes, text)]: members noise[:a] + filler whose dynamic block is one byte smaller than
    the stored one, as large, and one byte larger - the two sides of `dyn_bytes <= stored_bytes` and the tie itself.  The
    block grows with a (a byte of noise costs eight bits and more, the filler next to nothing), so the search bisects on a
    and then reads a window of neighbours; `budget` bounds the model runs.  Property: all three differences occur at two
    values of n at least."""
    found = []
    for n in TIE_SIZES:
        body = noise(100 + n, n)
        for filler in (b"A", b"AC", b"ACGTT"):
            def text(a):
                return body[:a] + (filler * (n // len(filler) + 1))[:n - a]

            def diff(r):
                return r[0]["dyn_bytes"] - r[0]["stored_bytes"]

            lo, hi = 0, n  # (taken for granted: the filler alone is a dynamic block, the noise alone a stored one)
            while hi - lo > 24 and budget > 0:
                mid = (lo + hi) // 2
                budget -= 1
                if diff(model.run([text(mid)])[1][0]) < 0:
                    lo = mid
                else:
                    hi = mid
            window = list(range(max(0, lo - 24), min(n, hi + 24) + 1))
            if budget <= 0:
                break
            budget -= 1
            got = {}
            for a, r in zip(window, model.run([text(a) for a in window])[1]):
                got.setdefault(diff(r), a)
            if all(d in got for d in (-1, 0, 1)):
                found.extend((n, got[d], d, text(got[d])) for d in (-1, 0, 1))
                break
    return found


def tie_property(cases, reports):
    seen = {}
    for (n, _, d, _), (r,) in zip(cases, reports):
        assert r["dyn_bytes"] - r["stored_bytes"] == d and r["n"] == n
        assert r["written"] == ("dynamic" if d <= 0 else "stored")
        seen.setdefault(n, set()).add(d)
    assert sum(s == {-1, 0, 1} for s in seen.values()) >= 2, seen


# ------------------------------------------------------------------------------------------------------- parse geometry

GEO_STARTS = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255)
GEO_LENGTHS = (4, 5, 6, 63, 64, 65, 192, 193, 255, 256, 257, 258)
GEO_CELL = 1280  # five steps: the source in the first, the copy in the third and, at most, two bytes of the fifth


def _differ(t, a, b):
    if t[a] == t[b]:
        t[a] ^= 1


def _plant(t, p, length, dist):
    """bytes [p, p + length) become a copy from `dist` back that is that long and no longer, and starts at p, not before"""
    _differ(t, p - 1, p - 1 - dist)
    for i in range(length):
        t[p + i] = t[p - dist + i]
    if p + length < len(t):
        _differ(t, p + length, p + length - dist)


def _geo_cell(seed, start, length):
    """a cell of noise with one copy: at `start` of the cell's third step, from 257 + start back - a step earlier than the
    copy's own, as a candidate must be, and near enough for a match of four bytes (512)"""
    t = bytearray(noise(seed, GEO_CELL))
    _plant(t, 512 + start, length, 257 + start)
    return t


def _chunks(seq, n):
    return [seq[k:k + n] for k in range(0, len(seq), n)]


def _geo_end(seed):
    """a copy of 40 bytes from 300 back whose last byte is the member's last; the member cut 36 and 37 bytes earlier"""
    t = bytearray(noise(3100 + seed, 2000 + 40))
    _plant(t, 2000, 40, 300)
    return [(bytes(t[:len(t) - cut]), want) for cut, want in ((0, [(2000, 40, 300)]), (36, [(2000, 4, 300)]), (37, []))]


def _geo_twins(seed):
    """two copies back to back, from 434 and from 754 back"""
    t = bytearray(noise(3200 + seed, 4096))
    t[1034:1054], t[1054:1084] = t[600:620], t[300:330]
    for a, b in ((599, 1033), (620, 1054), (299, 1053), (330, 1084)):
        _differ(t, a, b)
    return [(bytes(t), [(1034, 20, 434), (1054, 30, 754)])]


def _geo_inside(seed):
    """X (40 bytes) at 300; X[10:] + Z (70 bytes) at 800; X + Z at 1500: from 1510 a copy of 100 bytes lies at 800, but the
    parse has taken 40 bytes from 300 at 1500 and goes on behind them"""
    t = bytearray(noise(3300 + seed, 4096))
    x, z = bytes(t[300:340]), noise(3400 + seed, 70)
    t[800:900] = x[10:] + z
    t[1500:1610] = x + z
    for a, b in ((340, 1540), (1499, 299), (1610, 900)):
        _differ(t, a, b)
    return [(bytes(t), [(1500, 40, 1200), (1540, 70, 710)])]


def parse_geometry(model, rounds=24):
    """(texts, planted): planted[i] = [(position, length, distance)] that the parse of member i must take.

    Three members of noise in cells of 1280 bytes, each cell with one copy for a pair of GEO_STARTS x GEO_LENGTHS: the
    copy starts at that lane of a step (63 | 64, 127 | 128, 191 | 192: the parse goes to its next ballot window; 255 | 0:
    `next` goes to the next step) and its length carries the parse over that many windows and steps.  A later position
    with the same hash takes a planted source's slot now and then: such a cell gets other noise until the model's
    report shows the copy taken as planted.  Then five short members: a copy that ends at the member's end; the same cut
    to four bytes and to three (no match: p + 4 > n); two copies back to back; and a copy with a longer candidate
    inside it, which a greedy parse must not see."""
    pairs = [(s, l) for s in GEO_STARTS for l in GEO_LENGTHS]
    per_member = M // GEO_CELL
    seeds = {k: 1000 * k for k in range(len(pairs))}
    for _ in range(rounds):
        texts, planted = [], []
        for first in range(0, len(pairs), per_member):
            t, want = bytearray(), []
            for k in range(first, min(first + per_member, len(pairs))):
                want.append((len(t) + 512 + pairs[k][0], pairs[k][1], 257 + pairs[k][0]))
                t += _geo_cell(seeds[k], *pairs[k])
            texts.append(bytes(t + noise(77 + first, M - len(t))))
            planted.append(want)
        lost = 0
        for i, (r,) in enumerate(model.run(texts)[1]):
            taken = set(map(tuple, r["taken"]))
            for j, w in enumerate(planted[i]):
                if w not in taken:
                    seeds[i * per_member + j] += 1
                    lost += 1
        if not lost:
            break
    else:
        raise AssertionError("planted copies keep losing their hash slots")
    for special in (_geo_end, _geo_twins, _geo_inside):
        tries = [special(seed) for seed in range(16)]
        for made, reports in zip(tries, _chunks(model.run([t for made in tries for t, _ in made])[1], len(tries[0]))):
            if all(w in map(tuple, r["taken"]) for (_, want), (r,) in zip(made, reports) for w in want):
                texts.extend(t for t, _ in made)
                planted.extend(want for _, want in made)
                break
        else:
            raise AssertionError("no seed keeps the hash slots of %s" % special.__name__)
    return texts, planted


def parse_geometry_property(texts, planted, reports):
    pairs = set()
    for want, (r,) in zip(planted, reports):
        taken = list(map(tuple, r["taken"]))
        for w in want:
            assert w in taken, w
        pairs.update((p % 256, l) for p, l, _ in want)
    assert pairs >= {(s, l) for s in GEO_STARTS for l in GEO_LENGTHS}
    end, cut4, cut3, twins, inside = reports[-5:]
    assert tuple(end[0]["taken"][-1]) == (2000, 40, 300) and end[0]["n"] == 2040
    assert tuple(cut4[0]["taken"][-1]) == (2000, 4, 300) and cut4[0]["n"] == 2004
    assert all(p + l <= 2000 for p, l, _ in cut3[0]["taken"]) and cut3[0]["n"] == 2003
    assert not any(1500 < p < 1540 for p, _, _ in inside[0]["taken"])


# ------------------------------------------------------------------------------------------------------------ same slot

SLOT_PERIODS = (2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 255, 256, 257, 300)


def same_slot():
    """[text of 4099 bytes of every period]: the unit's bytes are distinct (noise above 256), so a step's 256 words share
    `period` hash slots and atomicMax decides 256 / period times per slot which position stays.  The second half of
    every text is a run of the unit's first byte and nine of another, where the candidate at distance 1 stands against the table's at equal
    length and wins (`l1 >= len`).  Property: every match of the first half is at a
    multiple of the period, the run's last match is at distance 1, and the matches cover nine tenths of the text."""
    out = []
    for period in SLOT_PERIODS:
        r = random.Random(500 + period)
        unit = bytes(r.sample(range(256), period)) if period <= 256 else r.randbytes(period)
        half = (unit * (2050 // period + 1))[:2050]
        out.append(half + unit[:1] * 2040 + bytes([unit[0] ^ 0x55]) * 9)
    return out


def same_slot_property(reports):
    for period, (r,) in zip(SLOT_PERIODS, reports):
        covered = 0
        for p, l, d in r["taken"]:
            covered += l
            if p + l <= 2050:
                assert d % period == 0, (period, p, l, d)
        assert covered >= 0.9 * (r["n"] - min(period, 300) - 300), (period, covered)
        # in the run a candidate of the table reaches 258 bytes and is taken as it is; the run's last match is shorter,
        # both candidates end with the run, and the one at distance 1 is written
        p, l, d = [m for m in r["taken"] if m[0] + m[1] == 2050 + 2040][0]
        assert l < 258 and d == 1, (period, p, l, d)


# --------------------------------------------------------------------------------------------------------------- window

def window(model, tries=96):
    """[texts]: noise of period 32767, 32768 and 32769, a full member each, and one member of noise with a copy of 50 bytes
    from 32768 back and another from 32769 back.  Between a source and its copy 32768 positions are inserted, two per
    hash slot: the planted source keeps its slot in one text out of seven, so `tries` seeds are tried in one run of the
    model.  Property: the report has a match at distance 32768 - in the periodic text and the planted one - and
    none beyond it anywhere."""
    texts = [(noise(40 + k, period) * 2)[:M] for k, period in enumerate((32767, 32768, 32769))]
    cands = []
    for seed in range(tries):
        t = bytearray(noise(600 + seed, M))
        _plant(t, 40000, 50, 32768)
        _plant(t, 50000, 50, 32769)
        cands.append(bytes(t))
    for t, (r,) in zip(cands, model.run(cands)[1]):
        if [40000, 50, 32768] in r["taken"]:
            return texts + [t]
    raise AssertionError("no seed keeps the hash slot of the copy at distance 32768")


def window_property(reports):
    far = [max((d for _, _, d in r["taken"]), default=0) for (r,) in reports]
    assert far[1] == 32768 and far[3] == 32768 and max(far) == 32768, far
    assert far[0] == 32767 and [40000, 50, 32768] in reports[3][0]["taken"]
    assert not any(p == 50000 for p, _, _ in reports[3][0]["taken"])


# ---------------------------------------------------------------------------------------------------------- wide tokens

WIDE_LETTERS = 6           # byte values 0..5: the filler in front of the wide tokens; the noise of this text has none of them
WIDE_LETTER_COUNTS = (512, 256, 128, 64, 32, 16)  # code lengths a bit apart each: what the filler can shift a token by
WIDE_GROUP = 10            # letters in front of every wide token
WIDE_FRONT = 32768 + 512
# (length symbol - 257, distance symbol, how many): the rarest lengths meet the rarest distances
WIDE_PAIRS = ((27, 29, 1), (26, 28, 1), (25, 27, 2), (24, 26, 3), (23, 25, 5), (22, 24, 8))
# (distance symbol, copies of six bytes): every count is above the sum of all counts two and more places before it, by
# the share of copies that lose their hash slot at that distance and two more - so the tree stays a chain
WIDE_NEAR = ((23, 18), (22, 27), (21, 46), (20, 74), (19, 121), (18, 197), (17, 318), (16, 518))


def _dist_class(sym):
    e = (sym - 2) >> 1
    low = ((2 + (sym & 1)) << e) + 1
    return low, low + (1 << e) - 1


def _len_class(sym):  # sym - 257 in 8..27
    e = (sym - 4) >> 2
    low = ((4 + (sym & 3)) << e) + 3
    return low, low + (1 << e) - 1


class _Wide:
    """the layout of wide_tokens(): everything but the letters of the groups and the sources of the wide copies is fixed"""

    def __init__(self):
        r = random.Random(4242)
        self.r = r
        self.front = bytes(r.choices(range(WIDE_LETTERS, 256), k=WIDE_FRONT))
        self.tokens = []  # [position, length, distance]
        p = WIDE_FRONT
        for len_sym, dist_sym, count in WIDE_PAIRS:
            for _ in range(count):
                low, high = _len_class(len_sym)
                p += 2 * WIDE_GROUP
                self.tokens.append([p, (low + high) // 2, 0, dist_sym])
                p += self.tokens[-1][1]
        self.near_at = -(-(p + 1) // 14) * 14  # (one byte of noise at least behind the last wide copy)
        self.used = []  # sources of the wide copies
        for k in range(len(self.tokens)):
            self.source(k)
        pool = []
        for letter, count in enumerate(WIDE_LETTER_COUNTS):
            pool += [letter] * count
        r.shuffle(pool)
        self.groups = [[pool.pop() for _ in range(WIDE_GROUP)] for _ in self.tokens]
        self.pool = sorted(pool)
        self.fill = bytes(r.choices(range(WIDE_LETTERS, 256), k=M))  # the noise of everything behind the front

    def source(self, k):
        """another source for wide copy k: in the front's noise, apart from the other copies' sources"""
        p, length, _, dist_sym = self.tokens[k]
        low, high = _dist_class(dist_sym)
        while True:
            dist = self.r.randint(low, min(high, p - 8))
            src = p - dist
            if src + length + 8 < self.near_at - 4200 and all(src + length + 8 < a or b + 8 < src for a, b in self.used):
                self.used.append((src, src + length))
                self.tokens[k][2] = dist
                return

    def text(self):
        t = bytearray(self.front)
        fill = iter(self.fill)
        for (p, length, dist, _), group in zip(self.tokens, self.groups):
            for letter in group:  # (a byte of noise behind every letter: no four bytes of filler occur twice)
                t += bytes((letter, next(fill)))
            assert len(t) == p
            t += t[p - dist:p - dist + length]
        while len(t) < self.near_at:
            t.append(next(fill))
        # copies of six bytes, one every fourteen, each from the noise between two earlier ones: class by class as many as
        # WIDE_NEAR says, as far as a source that no other copy has used lies in reach
        r = random.Random(4343)
        left = dict(WIDE_NEAR)
        taken_gaps = set()
        j = 0
        while sum(left.values()) and len(t) + 14 + 4 * len(self.pool) + 64 < M:
            p = len(t)
            done = False
            for sym in r.sample(list(left), len(left)) if r.random() < 0.5 else sorted(left, key=lambda s: -left[s]):
                if not left[sym]:
                    continue
                low, high = _dist_class(sym)
                ks = [k for k in range(j - (high + 7) // 14, j - (low + 7) // 14 + 1)
                      if k not in taken_gaps and low <= 14 * (j - k) - 7 <= high
                      and (k >= 0 or self.near_at + 14 * k + 7 + 8 < WIDE_FRONT)]
                if ks:
                    k = r.choice(ks)
                    taken_gaps.add(k)
                    src = self.near_at + 14 * k + 7
                    t += t[src:src + 6]
                    left[sym] -= 1
                    done = True
                    break
            if not done:
                t += bytes(next(fill) for _ in range(6))
            for _ in range(8):
                t.append(next(fill))
            if done and t[p + 6] == t[src + 6]:
                t[p + 6] = t[p + 6] % 250 + WIDE_LETTERS  # (noise still, and another byte)
            j += 1
        for letter in self.pool:
            t.append(letter)
            t += bytes(next(fill) for _ in range(3))
        while len(t) < M:
            t.append(next(fill))
        return bytes(t[:M])


def wide_tokens(model, rounds=80):
    """One full member whose widest tokens need the third word of gz_or_bits (a token of 34 bits and more that begins late
    enough in its 32-bit word), sixteen times and more.

    A token is widest where a rare length symbol and a rare distance symbol meet and both carry many extra bits: 15 + 5
    bits for a length of 131..257 whose symbol has the longest code, 15 + 13 for a distance of 16385..32768 whose symbol
    has the longest, 48 in all.  Positions of one step cannot be candidates for one another, so distances above 256 build
    the distance tree: the fourteen classes 257..384, ..., 24577..32768 with Fibonacci-weighted counts (1, 1, 2, 3, 5,
    8, 13, ... 377), the farthest the rarest, give it thirteen levels.  The twenty copies of the six rarest classes (eleven
    to thirteen extra bits) are the wide tokens: their lengths are the six longest length symbols (four and five extra
    bits) with the same counts, which, below 244 values of noise and six filler letters, sink to the 15th level of the
    literal/length tree.  All other copies are six bytes long.

    Few tokens can be wide - a long code is a rare symbol - so every one of them is put where it needs the third word:
    ten filler letters stand in front of each wide copy, their code lengths a bit apart each, and with the model's report
    of every token's first bit the letters are exchanged with a pool at the member's end (the histograms stay as they
    are) until the token begins in the last bits of its word.  A wide copy's source lies up to 32768 positions back, two
    per hash slot: a copy that lost its slot gets another source.  -> (text, report)

    Reached: see wide_tokens_property and docs/host_gzip.md.  48 bits would take two more distance symbols below
    the fourteen (distances below 257 reach a copy only across a step's edge, or as distance 1 in a run)."""
    w = _Wide()
    for _ in range(rounds):
        text = w.text()
        (report,), = model.run([text])[1]
        at = {tuple(m): b for m, b in zip(report["taken"], report["taken_at"])}
        lost = [k for k, (p, length, dist, _) in enumerate(w.tokens) if (p, length, dist) not in at]
        for k in lost:
            w.source(k)
        if lost:
            continue
        if report["three_word_gzip"] >= 16:
            return text, report
        # the letters of every group anew: `shift` is what the groups so far have added to every later token's first bit
        ll = report["lit_len"][:WIDE_LETTERS]
        pool = [w.pool.count(letter) for letter in range(WIDE_LETTERS)]
        shift = 0
        for k, (p, length, dist, _) in enumerate(w.tokens):
            first, width = at[(p, length, dist)]
            have = [w.groups[k].count(letter) for letter in range(WIDE_LETTERS)]
            old = sum(n * b for n, b in zip(have, ll))
            best = None
            for combo in _compositions(WIDE_GROUP, WIDE_LETTERS):
                if any(c > h + q for c, h, q in zip(combo, have, pool)):
                    continue
                new = sum(n * b for n, b in zip(combo, ll))
                if ((80 + first + shift + new - old) & 31) + width > 64:
                    cost = sum(max(0, c - h) / (1 + q) for c, h, q in zip(combo, have, pool))
                    if best is None or cost < best[0]:
                        best = (cost, combo, new)
            if best is None:
                continue
            _, combo, new = best
            pool = [q + h - c for q, h, c in zip(pool, have, combo)]
            w.groups[k] = [letter for letter in range(WIDE_LETTERS) for _ in range(combo[letter])]
            shift += new - old
        w.pool = [letter for letter in range(WIDE_LETTERS) for _ in range(pool[letter])]
    raise AssertionError("the wide tokens do not come to rest")


def _compositions(total, parts):
    if parts == 1:
        yield (total,)
        return
    for first in range(total + 1):
        for rest in _compositions(total - first, parts - 1):
            yield (first,) + rest


def wide_tokens_property(report):
    assert report["written"] == "dynamic"
    assert report["widest"] > 34, report["widest"]
    assert report["three_word_gzip"] >= 16 and report["three_word_bgzf"] >= 16, (report["three_word_gzip"], report["three_word_bgzf"])
    assert report["max_ll"] == 15, report["max_ll"]


# --------------------------------------------------------------------------------------------------------- member cycle

def no_match_text():
    """M bytes in which no four bytes occur twice and whose bytes are far from equally frequent: '@' and a counter of three
    letters, 16320 times.  Every position is a literal: ntok = M + 1, 256 rounds of the bit scan."""
    digits = bytes(range(0x41, 0x41 + 26))
    out = bytearray()
    for k in range(M // 4):
        out += bytes([0x40, digits[k // 676], digits[k // 26 % 26], digits[k % 26]])
    return bytes(out)


def member_cycle(model):
    """seven full members, neighbours unlike each other in everything a workgroup keeps in LDS from one member to the next:
    histograms, token count, hash table, the image (stored | dynamic, long | short)"""
    r = random.Random(808)
    two = bytes(r.choice(b"AB") for _ in range(M))
    cycle = [fastq_text(700, 9)[:M], noise(809, M), bytes(M), wide_tokens(model)[0], no_match_text(), two, (noise(810, 32768) * 2)[:M]]
    assert all(len(t) == M for t in cycle)
    return cycle


def member_cycle_property(reports):
    fastq, stored, zeros, wide, literal, two, periodic = (r for (r,) in reports)
    assert stored["written"] == "stored" and all(r["written"] == "dynamic" for r in (fastq, zeros, wide, literal, two, periodic))
    assert literal["matches"] == 0 and literal["ntok"] == M + 1
    assert zeros["ntok"] < 300 and zeros["dyn_bytes"] < 400
    assert max(d for _, _, d in periodic["taken"]) == 32768
    wide_tokens_property(wide)
    ntok = [r["ntok"] for r in (fastq, stored, zeros, wide, literal, two, periodic)]
    assert all(abs(a - b) > 1000 for a, b in zip(ntok, ntok[1:] + ntok[:1])), ntok


def cycle_text(cycle, n_members):
    """the cycle repeated to n_members members, the last one cut to 777 bytes; -> (text, index of every member in the
    cycle, the cut last member's text)"""
    order = [k % 7 for k in range(n_members - 1)]
    last = cycle[(n_members - 1) % 7][:777]
    reps, rest = divmod(n_members - 1, 7)
    return b"".join(cycle) * reps + b"".join(cycle[:rest]) + last, order, last


# ------------------------------------------------------------------------------------------- the families and the model

BGZF_HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0])
BGZF_EOF = BGZF_HEAD + bytes([0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def split_members(gz, reports):
    """the model's bytes for one text, member by member: the report says how long each block is"""
    out, at = [], 0
    for r in reports:
        size = 10 + (r["dyn_bytes"] if r["written"] == "dynamic" else r["stored_bytes"]) + 8
        out.append(gz[at:at + size])
        at += size
    assert at == len(gz)
    return out


def bgzf_of(members, empty=False):
    """what fqg_bgzf_deflate(final) must write for the text the model made these gzip members of: every member behind
    BGZF's eighteen header bytes instead of gzip's ten, BSIZE = the block's bytes - 1, and the end-of-file block (an empty
    text is one gzip member and no BGZF block at all)"""
    return (b"" if empty else b"".join(bgzf_block(m) for m in members)) + BGZF_EOF


def bgzf_block(member):
    return BGZF_HEAD + (len(member) + 8 - 1).to_bytes(2, "little") + member[10:]


class Family:
    def __init__(self, model, texts):
        self.texts = texts
        self.gz, self.reports = model.run(texts)

    def bgzf(self, k):
        return bgzf_of(split_members(self.gz[k], self.reports[k]), empty=not self.texts[k])


def families(model):
    """(name -> Family, check): every family above with the model's bytes and reports; check() raises if one of them is
    not what its generator says"""
    tie_cases = tie(model)
    geo_texts, planted = parse_geometry(model)
    wide_text, _ = wide_tokens(model)
    cycle = member_cycle(model)
    fam = {"sizes_" + c: Family(model, sizes(c)) for c in SIZE_CONTENTS}
    fam.update(tie=Family(model, [c[3] for c in tie_cases]), parse_geometry=Family(model, geo_texts), same_slot=Family(model, same_slot()),
               window=Family(model, window(model)), wide_tokens=Family(model, [wide_text]), member_cycle=Family(model, cycle))

    def check():
        sizes_property({c: fam["sizes_" + c].reports for c in SIZE_CONTENTS})
        tie_property(tie_cases, fam["tie"].reports)
        parse_geometry_property(geo_texts, planted, fam["parse_geometry"].reports)
        same_slot_property(fam["same_slot"].reports)
        window_property(fam["window"].reports)
        wide_tokens_property(fam["wide_tokens"].reports[0][0])
        member_cycle_property(fam["member_cycle"].reports)
    return fam, check


_SHARED = []


def shared():
    """(model, name -> Family) for the GPU tests: the model built and the families made once per process"""
    if not _SHARED:
        keep = tempfile.TemporaryDirectory(prefix="deflgen_")
        model = Model(keep.name)
        _SHARED.extend((keep, model, families(model)[0]))
    return _SHARED[1], _SHARED[2]


def alignment_texts():
    """{(carry bytes, text bytes): text} of tests' alignment cases: FASTQ, so the blocks are dynamic"""
    whole = fastq_text(900, 12)
    return {(c, n): whole[:n] for c in (0, 1, 3, 15, 16, 17, 255) for n in (700, M + 700)}
