"""A plain model of the read-name keys and of the read-name table (no GPU, no product code in here).

Written from the documented definitions, not from the register code:
  - the canonical name: fastq_get_readname (reference src/fastq.c:488-512) on the C string of the header line, with the
    quirks the comments of canon_name (fqg_index_kernels.hip) cite;
  - the hash: fqg_device.h - seed(n), ONE 32 x 32 multiply-add per 8-byte word that holds a name byte, name_fin;
  - the 23 check bits: mix_hash2 / fin_hash2 over the full words and then the partial (possibly empty) last word;
  - the table: open addressing, linear probing, one `tag : 24 | record : 40` word per slot.
Everything is Python integers and bytes; numpy only where many candidates are hashed at once."""
import struct

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
MAX_LABEL = 1000            # FQG_MAX_LABEL_LENGTH: gzgets hands out at most MAX_LABEL - 1 bytes of a header line, '\n' included
NAME_INLINE = 56            # kNameInline
NAME_REC_TEXT = 60          # kNameRecText
DIGEST_TEXT = 64            # kDigestText
HDR_BYTES = 128             # kHdrBytes
CHUNK = 4096                # kChunkBytes
NAME_DEFAULT, NAME_CASAVA18, NAME_INTEGER = 0, 1, 2
NO_MATCH, MATCH_WRONG_HEADER = M64, M64 - 1
E_WRONG_HEADER, E_DUP_NAME, E_UNPAIRED = 2, 3, 13
STYLES = ("casava", "slash", "int", "nosuffix")
FMT_OF = {"casava": NAME_CASAVA18, "slash": NAME_DEFAULT, "int": NAME_INTEGER, "nosuffix": NAME_INTEGER}
# (style, is_pe): the five ways a name is cut out of a header (is_pe only matters to `slash`)
MODES = (("casava", True), ("slash", True), ("slash", False), ("int", True), ("nosuffix", True))


# ---- the canonical name ---------------------------------------------------------------------------------------------
def canonical(header_line, has_nl, fmt, is_pe, may_have_nul=True):
    """header_line: the bytes of the line without its '\\n' (the '@' included).  -> (n, acct, at_sign): the length of
    the canonical name (it starts at byte 1 of the line and may run into the '\\n'), the `len` the reference hands to
    new_indexentry (src/fastq.c:609), and whether the line starts with '@' (src/fastq.c:448)."""
    cstr = len(header_line) + (1 if has_nl else 0)          # strlen(hdr): the C string counts the '\n'
    if may_have_nul:
        z = header_line.find(b"\0")
        if z >= 0:
            cstr = z
    L = cstr - 1 if cstr > 0 else 0                         # strlen(&hdr[1])
    at_sign = header_line[:1] == b"@"
    if fmt == NAME_CASAVA18:
        text = (header_line + (b"\n" if has_nl else b""))[1:1 + L]
        sp = text.find(b" ")
        if sp < 0:
            sp = L                                          # no blank: the name keeps the '\n'
        if sp >= 2 and text[sp - 2:sp - 1] == b"/":         # (rn[len - 2] is only a name byte with sp >= 2)
            sp -= 2
        return sp, sp, at_sign
    l = L
    if fmt == NAME_DEFAULT and is_pe:
        l -= 1
    acct = l if l > 0 else 0
    return (l - 1 if l >= 1 else L), acct, at_sign           # rn[len - 1] = '\0' only lands in the name with len >= 1


def canonical_name(header_line, has_nl, fmt, is_pe, may_have_nul=True):
    n = canonical(header_line, has_nl, fmt, is_pe, may_have_nul)[0]
    return (header_line + (b"\n" if has_nl else b""))[1:1 + n]


# ---- the hashes -----------------------------------------------------------------------------------------------------
def name_mul(k):
    return ((0x9E3779B97F4A7C15 + k * 0xD1B54A32D192ED03) & M64) | 1


def _words(name):
    """the 8-byte little-endian words of the name, zero bytes behind it: only words that hold a name byte"""
    pad = name + b"\0" * (-len(name) % 8)
    return list(struct.unpack("<%dQ" % (len(pad) // 8), pad))


def name_fin(h):
    hi = h >> 32
    t = (h & M32) ^ hi
    p = t * 0xD6E8FEB9
    q = hi * 0x85EBCA6B
    return p ^ (((q << 32) | (q >> 32)) & M64)


def hash64(name):
    h = 0x2545F4914F6CDD1D + len(name)
    for k, w in enumerate(_words(name)):
        m = name_mul(k)
        h += (((w & M32) + (m & M32)) & M32) * (((w >> 32) + (m >> 32)) & M32)
    return name_fin(h & M64)


def hash2(name):
    """the second hash: every FULL word, then the partial last word - an empty one when the length is a multiple of 8"""
    g = (0x9E3779B97F4A7C15 + len(name)) & M64
    ws = _words(name)
    if len(name) % 8 == 0:
        ws.append(0)
    for w in ws:
        g = ((g ^ w) * 0xC2B2AE3D27D4EB4F) & M64
        g ^= g >> 31
    g = (g * 0x94D049BB133111EB) & M64
    return g ^ (g >> 29)


def check23(name):
    """bits 40..62 of the index word that travels with a fingerprint"""
    return hash2(name) & ((1 << 23) - 1)


def fingerprint(name):
    """the fingerprint that travels: the hash, kept clear of the two values the table reserves"""
    return min(hash64(name), M64 - 2)


def owner(fp, n_owners):
    return ((fp >> 32) * n_owners) >> 32


def name_record(name, at_sign=True):
    """NameRec (fqg_index_kernels.hip), as the index keeps it and fqg_frame_name_records writes it: the length (bit 63:
    the header does not start with '@'), then the first 56 name bytes, zero padded"""
    return struct.pack("<Q", len(name) | (0 if at_sign else 1 << 63)) + name[:NAME_INLINE].ljust(NAME_INLINE, b"\0")


def travel_record(name):
    """the name record that travels beside a fingerprint: the first 56 name bytes, zero padded, then the length"""
    return name[:NAME_INLINE].ljust(NAME_INLINE, b"\0") + struct.pack("<Q", len(name))


# ---- names with a chosen hash ----------------------------------------------------------------------------------------
def zero_half(k, high):
    """the four bytes that make word k's product zero whatever the word's other half holds: lo + A_k = 0 (mod 2^32) in
    the low half, or hi + B_k = 0 in the high half"""
    m = name_mul(k)
    return struct.pack("<I", (-(m >> 32 if high else m & M32)) & M32)


def twins(k, length=8, word=0, high=False, prefix=None, free=None):
    """k different names of `length` bytes with ONE 64-bit hash.  By default they start with the bytes that zero word
    0's product (EB 83 B5 80) and differ in the word's high half; high=True: they END in 47 86 C8 61 and differ in the
    low half.  word chooses another full word of the name: the names agree everywhere but in the OTHER half of that
    word, which the zero product hides.  Word 5, high half (49 13 3E 49 at bytes 44..47) is the one choice among the
    first eight words whose bytes are all below 0x80.  free: the byte values the four differing places are drawn from;
    prefix: the bytes of the name everywhere else."""
    assert 8 * word + 8 <= length, "the chosen word must be a full word of the name"
    free = free if free is not None else bytes(range(0x30, 0x3A)) + bytes(range(0x41, 0x5B)) + bytes(range(0x61, 0x7B))
    base = bytearray(prefix if prefix is not None else bytes(0x61 + (i * 7) % 26 for i in range(length)))
    assert len(base) == length
    z = zero_half(word, high)
    fixed_at, free_at = (8 * word + 4, 8 * word) if high else (8 * word, 8 * word + 4)
    base[fixed_at:fixed_at + 4] = z
    out = []
    for i in range(k):
        v, four = i, []
        for _ in range(4):
            four.append(free[v % len(free)])
            v //= len(free)
        assert v == 0, "more twins asked for than the free bytes give"
        nm = bytearray(base)
        nm[free_at:free_at + 4] = bytes(four)
        out.append(bytes(nm))
    return out


def with_home(slot_set, mask, count, style="casava", stem=b"h", limit=2000000):
    """{slot: [count names]} for every slot of slot_set: names (canonical) whose home slot hash & mask is that slot,
    found by trying suffixes.  style "int": digits only."""
    want = {s: [] for s in slot_set}
    open_ = len(want)
    for i in range(limit):
        nm = (b"%d" % (10 ** 9 + i)) if style == "int" else stem + b"%07d" % i
        s = hash64(nm) & mask
        if s in want and len(want[s]) < count:
            want[s].append(nm)
            if len(want[s]) == count:
                open_ -= 1
                if not open_:
                    return want
    raise AssertionError("with_home: not enough candidates")


# ---- headers and images ---------------------------------------------------------------------------------------------
def header_for(name, style, is_pe=True, mate=1, comment=b""):
    """a header line (without '\\n') whose canonical name under (style, is_pe) is `name`"""
    if style == "casava":
        return b"@" + name + b" %d:N:0:AC" % mate + comment
    if style == "slash" and is_pe:
        return b"@" + name + b"%d" % mate          # (the reference drops the last byte in front of the '\n': "x/1" -> "x/")
    return b"@" + name


def lead_header(style, mate=1):
    """the header of an image's first record: it fixes the read-name format the way the reference detects it"""
    return {"casava": b"@LEAD:0:0 %d:N:0:AC" % mate, "slash": b"@lead.0/%d" % mate, "int": b"@4000000000",
            "nosuffix": b"@lead_0_x"}[style]


BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def record(header_line, rng, ln=40):
    s = BASES[rng.integers(0, 4, ln)].tobytes()
    q = (rng.integers(5, 40, ln) + 33).astype(np.uint8).tobytes()
    return header_line + b"\n" + s + b"\n+\n" + q + b"\n"


def image(header_lines, seed=1, ln=40, final_newline=True):
    rng = np.random.default_rng(seed)
    img = b"".join(record(h, rng, ln) for h in header_lines)
    return img if final_newline else img[:-1]


def generated_names(style, count, first=0, stem=b"pad"):
    """canonical names that no ladder name is (they start with `stem`, ladder names never do)"""
    if style == "int":
        return [b"%d" % (7 * 10 ** 11 + first + i) for i in range(count)]
    return [stem + b":%d:%d" % ((first + i) % 89, first + i) for i in range(count)]


# ---- the ladder -----------------------------------------------------------------------------------------------------
NAME_LENGTHS = ([0, 1, 2, 7, 8, 9, 15, 16, 17, 47, 48, 49, 55, 56, 57, 59, 60, 61, 63, 64, 65] + list(range(119, 131)) + [300])
LINE_LENGTHS = [15, 16, 17, 31, 32, 33, 125, 126, 127, 128]          # hdr_load fetches 16-byte pieces; kHdrBytes - 1
BLANK_AT = list(range(1, 19)) + [23, 24, 25, 26] + list(range(55, 67)) + [126, 127]
LONGEST_LINES = [MAX_LABEL - 3, MAX_LABEL - 2]                       # a line of MAX_LABEL - 2 bytes + '\n' is the longest gzgets returns whole


def _filler(style, serial, n):
    alpha = b"0123456789" if style == "int" else b"bcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    out, s = [], serial
    for _ in range(3):
        out.append(alpha[s % len(alpha)])
        s //= len(alpha)
    out += [alpha[(serial + 5 * i) % len(alpha)] for i in range(max(0, n - 3))]
    return bytes(out[:n])


def ladder(style, is_pe=True):
    """[(header line without '\\n', note)]: the header lines at whose lengths and blanks the ways to a key can differ.
    Names of one ladder are different wherever their length leaves room for it (distinct() drops the rest)."""
    out, serial = [], [0]
    over = 1 if (style == "slash" and is_pe) else 0   # text bytes behind the canonical name

    def fresh(n):
        serial[0] += 1
        return _filler(style, serial[0], n)

    if style != "casava":
        for n in NAME_LENGTHS:
            if n + over:                                    # (a name of no bytes is the header "@": degenerate() has it)
                out.append((header_for(fresh(n), style, is_pe), "name of %d" % n))
        for ll in LINE_LENGTHS + LONGEST_LINES:
            out.append((header_for(fresh(ll - 1 - over), style, is_pe), "line of %d" % ll))
    else:
        for n in NAME_LENGTHS:
            out.append((header_for(fresh(n), style), "name of %d" % n))
        for ll in LINE_LENGTHS + LONGEST_LINES:
            h = header_for(fresh(5), style)
            out.append((h + b"C" * (ll - len(h)), "line of %d" % ll))
        for p in BLANK_AT:                                  # the first blank at line byte p: a name of p - 1 bytes
            out.append((header_for(fresh(p - 1), style), "blank at %d" % p))
            for mate in (1, 2):
                if p >= 3:                                  # ".../1" in front of the blank: the '/' at line byte p - 2
                    out.append((b"@" + fresh(p - 3) + b"/%d 1:N:0:AC" % mate, "/%d in front of the blank at %d" % (mate, p)))
        for n in (10, 58, 62, 126, 200):                    # no blank at all: the name runs into the '\n'
            out.append((b"@" + fresh(n), "no blank, text of %d" % n))
        out.append((b"@/1 1:N:0:AC", "x/1 with sp = 2"))
        out.append((b"@q/1 1:N:0:AC", "x/1 with sp = 3"))
        out.append((b"@" + fresh(12) + b"  1:N:0:AC", "two blanks"))
        out.append((b"@" + fresh(6) + b" " + fresh(6) + b" 1:N:0:AC", "a blank inside, one behind"))
        out.append((b"@ 1:N:0:AC", "a blank as the first name byte"))
        out.append((b"@" + fresh(20) + b"/1/2 1:N:0:AC", "two suffixes"))
        out.append((b"@" + fresh(20) + b"/ 1:N:0:AC", "a '/' right in front of the blank"))
    out += [(b"@a", "short"), (b"@/1", "short"), (b"@1", "short")]
    return out


def degenerate(style):
    """header lines no validated file holds, but a frame may (FQG_VALIDATE_FRAME_ONLY): "@" alone - the reference asks
    for a longer one - and a header that does not start with '@'"""
    return [(b"@", "the '@' alone"), (b"X" + header_for(b"noat", style)[1:], "no '@'")]


def distinct(entries, fmt, is_pe, taken=()):
    """the entries whose canonical names are new (the earlier one stays)"""
    seen, keep = set(taken), []
    for h, note in entries:
        nm = canonical_name(h, True, fmt, is_pe)
        if nm not in seen:
            seen.add(nm)
            keep.append((h, note))
    return keep


def holdable(header_line, fmt, is_pe, digests):
    """can a capture record (64 bytes: 60 text bytes behind the '@') or a digest (four lanes x 16 bytes = 64 name
    bytes) of a header whose line end was seen give the name?  From the layouts documented in fqg_device.h."""
    L = len(header_line)                      # bytes behind the '@', the '\n' counted: strlen(&hdr[1])
    n = canonical(header_line, True, fmt, is_pe)[0]
    if L >= MAX_LABEL:
        return False
    if digests:
        if n > DIGEST_TEXT:
            return False
        return fmt != NAME_CASAVA18 or b" " in header_line[1:1 + DIGEST_TEXT + 1]
    if fmt == NAME_CASAVA18:
        sp = header_line[1:].find(b" ")
        return 0 <= sp < min(L, NAME_REC_TEXT)
    return L <= NAME_REC_TEXT


# ---- the table ------------------------------------------------------------------------------------------------------
class TableModel:
    """Serial linear probing into `capacity` slots of tag | record words.  insert(): one more frame of names - per record
    the canonical name, or None for a header without '@'; accts: per record what the reference accounts for the name.
    The finding of a frame follows the first-repeat rule of the serial loop (src/fastq.c:396-439), while the table
    itself holds - as the device leaves it when the caller goes on - every name once, at its smallest record.
    part_log: also note the records whose probe ran past the end of their part of 2^part_log slots (the spill set)."""

    def __init__(self, capacity, part_log=None):
        self.capacity, self.mask, self.part_log = capacity, capacity - 1, part_log
        self.names = []
        self.slots = [None] * capacity
        self.holder = {}          # name -> the record that holds it
        self.first_dup = self.first_wrong = None   # of the first frame (global records: the same thing there)
        self.findings = []        # per frame (code, record of the frame)
        self.index_bytes = 0
        self.spilled = []
        self.claims = {}          # holder record -> the smallest asker that took it
        self.n_askers = 0

    def insert(self, names, accts=None):
        base = len(self.names)
        accts = list(accts) if accts is not None else [len(x) if x is not None else 0 for x in names]
        dup = wrong = None
        for r, nm in enumerate(names):
            self.names.append(nm)
            if nm is None:
                wrong = r if wrong is None else wrong
                continue
            if nm in self.holder:
                dup = r if dup is None else dup
                continue
            self.holder[nm] = base + r
            self.index_bytes += accts[r]
            h = hash64(nm)
            at = h & self.mask
            if self.part_log is not None:
                end = ((at >> self.part_log) + 1) << self.part_log
                while at < end and self.slots[at] is not None:
                    at += 1
                if at == end:
                    self.spilled.append(base + r)
                    at = h & self.mask
            while self.slots[at] is not None:
                at = (at + 1) & self.mask
            self.slots[at] = ((h >> 40) << 40) | (base + r)
        if not base:
            self.first_dup, self.first_wrong = dup, wrong
        if wrong is not None and (dup is None or wrong < dup):
            f = (E_WRONG_HEADER, wrong)
        else:
            f = (E_DUP_NAME, dup) if dup is not None else (0, 0)
        self.findings.append(f)
        return f

    @property
    def n_entries(self):
        return len(self.holder)

    @property
    def index_mem(self):
        """sizeof(hashtable) + per entry sizeof(INDEX_ENTRY) + len + 1 + sizeof(hashnode) (src/fastq.c:609)"""
        return 8 + self.n_entries * (16 + 1 + 24) + self.index_bytes

    def finding(self):
        """(code, record) of the first insert: the earlier of the first header without '@' and the first repeated name"""
        return self.findings[0]

    def slot_of(self, name):
        """where linear probing finds the name (None: it is not in the table); the probes it took"""
        h = hash64(name)
        at, probes = h & self.mask, 0
        while self.slots[at] is not None and probes <= self.mask:
            if self.slots[at] >> 40 == h >> 40 and self.names[self.slots[at] & ((1 << 40) - 1)] == name:
                return at, probes
            at, probes = (at + 1) & self.mask, probes + 1
        return None, probes

    def match_delete(self, asked):
        """the file-2 loop (src/fastq_info.c:333-356: look the name up, delete the entry) over one more frame of askers:
        -> (code, record of the frame, per asker the record whose entry it took / NO_MATCH / MATCH_WRONG_HEADER).  The
        loop stops at the first asker without a partner; the device goes on, and every later asker is answered as the
        loop would have answered it had it gone on."""
        out, wrong, missing = [], None, None
        for r, nm in enumerate(asked):
            if nm is None:
                out.append(MATCH_WRONG_HEADER)
                wrong = r if wrong is None else wrong
                continue
            g = self.holder.get(nm)
            if g is None or g in self.claims:
                out.append(NO_MATCH)
                missing = r if missing is None else missing
            else:
                self.claims[g] = self.n_askers + r
                out.append(g)
        self.n_askers += len(asked)
        if wrong is not None and (missing is None or wrong < missing):
            return E_WRONG_HEADER, wrong, out
        return (E_UNPAIRED, missing, out) if missing is not None else (0, 0, out)

    def entries_left(self):
        return self.n_entries - len(self.claims)

    def alive(self):
        """per inserted record: 1 when the table holds its entry and nobody has taken it"""
        a = [0] * len(self.names)
        for g in self.holder.values():
            a[g] = 0 if g in self.claims else 1
        return a


def table_model(names, capacity, accts=None, part_log=None):
    m = TableModel(capacity, part_log)
    m.insert(names, accts)
    return m


# ---- the owner side: runs of equal fingerprints ----------------------------------------------------------------------
FP_FILE2 = 1 << 63
FP_CHECK_MASK = ((1 << 23) - 1) << 40
FP_INDEX_MASK = (1 << 40) - 1


def runs_of(fps):
    """[(first, end)] of the runs of equal values in the sorted order, and the stable order itself"""
    order = sorted(range(len(fps)), key=lambda i: fps[i])
    runs, i = [], 0
    while i < len(order):
        e = i
        while e < len(order) and fps[order[e]] == fps[order[i]]:
            e += 1
        runs.append((i, e))
        i = e
    return order, runs


def candidates_model(fps, idxs):
    """k_fp_runs: per run of two or more, (smallest index, every other index) - the check bits are no part of it"""
    order, runs = runs_of(fps)
    out = []
    for i, e in runs:
        if e - i < 2:
            continue
        v = [idxs[order[k]] & ~FP_CHECK_MASK & M64 for k in range(i, e)]
        mn = min(v)
        out += [(mn, x) for x in v if x != mn]
    return sorted(out)


def pair_runs_model(fps, idxs, names=None):
    """the comment above k_fp_pair_runs: per run of h holders and a askers - (1, 1) with equal check bits (and, with
    names, equal name records of names that fit a record) a pair; (h, 0) left over; (0, a) unpaired, the smallest index
    among them the candidate for first_unpaired; anything else exported as (run id = the run's first place in the sorted
    order, index without the check bits).  names: per entry its travel_record()."""
    order, runs = runs_of(fps)
    s = {"matched": 0, "leftover": 0, "unpaired": 0, "first_unpaired": None, "n_complex": 0}
    ent = []
    for i, e in runs:
        v = [idxs[order[k]] for k in range(i, e)]
        hold = [k for k in range(i, e) if not idxs[order[k]] & FP_FILE2]
        ask = [k for k in range(i, e) if idxs[order[k]] & FP_FILE2]
        pair = len(hold) == 1 and len(ask) == 1 and (idxs[order[hold[0]]] & FP_CHECK_MASK) == (idxs[order[ask[0]]] & FP_CHECK_MASK)
        by_index = False
        if pair and names is not None:
            nh, na = names[order[hold[0]]], names[order[ask[0]]]
            by_index = nh != na or struct.unpack("<Q", nh[56:])[0] > NAME_INLINE or struct.unpack("<Q", na[56:])[0] > NAME_INLINE
            pair = not by_index
        if pair:
            s["matched"] += 1
        elif not by_index and not ask:
            s["leftover"] += len(hold)
        elif not by_index and not hold:
            s["unpaired"] += len(ask)
            m = min(x & FP_INDEX_MASK for x in v)
            s["first_unpaired"] = m if s["first_unpaired"] is None else min(m, s["first_unpaired"])
        else:
            s["n_complex"] += e - i
            ent += [(i, x & ~FP_CHECK_MASK & M64) for x in v]
    return s, sorted(ent)
