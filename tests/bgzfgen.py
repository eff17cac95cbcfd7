"""BGZF files for the inflate tests (tests/test_inflate_core.py, tests/test_gpu_inflate.py): header, BSIZE, CRC-32 and
ISIZE are written here, so that a file may hold what bgzip never writes - hand-made deflate blocks, damaged payloads,
wrong frames - and zlib's verdict on every block, which is what the inflater under test must say.

A payload comes from zlib (`deflate`: level, strategy, memLevel, flushes in mid-text) or from the two bit writers
(`fixed_block`, `dynamic_block`: tokens under codes the caller chooses)."""
import functools
import random
import struct
import zlib

EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
NONE = 2 ** 64 - 1
Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE = 4, 2, 3


# ---- payloads ---------------------------------------------------------------------------------
def deflate(data, level=6, strategy=0, mem=8, flushes=()):
    """raw deflate of data; flushes: (offset, zlib flush mode) pairs in ascending order"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += c.compress(data[at:off]) + c.flush(mode)
        at = off
    return out + c.compress(data[at:]) + c.flush()


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):          # as deflate packs fields: least significant bit first
        self.v |= value << self.n
        self.n += nbits

    def code(self, value, nbits):         # a Huffman code: most significant bit first
        self.put(int(format(value, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def put_tokens(b, tokens, lit, dist):
    """tokens: an int (a literal byte or a raw literal/length symbol), or (length, distance), or ("raw", lsym, lextra_bits,
    lextra, dsym, dextra_bits, dextra)"""
    for t in tokens:
        if isinstance(t, int):
            b.code(*lit[t])
        elif t[0] == "raw":
            _, ls, lb, lx, ds, db, dx = t
            b.code(*lit[ls])
            b.put(lx, lb)
            b.code(*dist[ds])
            b.put(dx, db)
        else:
            length, d = t
            ls = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
            ds = max(k for k in range(30) if DIST_BASE[k] <= d)
            b.code(*lit[257 + ls])
            b.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
            b.code(*dist[ds])
            b.put(d - DIST_BASE[ds], DIST_EXTRA[ds])


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def fixed_block(tokens, final=True, bits=None, eob=True):
    b = bits or Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LIT, FIXED_DIST)
    if eob:
        b.code(*FIXED_LIT[256])
    return b


def dynamic_block(tokens, lit_lens, dist_lens, final=True, bits=None, hlit=None, hdist=None, cl_lens=None, cl_syms=None):
    """a dynamic block whose header spells every length out (no repeat codes) under a code-length code of sixteen 4-bit
    codes - or under cl_lens, with the run-length symbols cl_syms in place of the plain lengths"""
    b = bits or Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
    b.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
    b.put(15, 4)
    cl = cl_lens or ([4] * 16 + [0, 0, 0])
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.put(cl[s], 3)
    clc = canonical(cl)
    for s in (cl_syms if cl_syms is not None else list(lit_lens) + list(dist_lens)):
        if isinstance(s, tuple):   # (symbol, extra bits, extra value)
            b.code(*clc[s[0]])
            b.put(s[2], s[1])
        else:
            b.code(*clc[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    put_tokens(b, tokens, lit, dist)
    if 256 in lit:
        b.code(*lit[256])
    return b


def stored_block(data, final=True, bits=None, nlen=None):
    b = bits or Bits()
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    for x in data:
        b.put(x, 8)
    return b


# ---- frames -----------------------------------------------------------------------------------
def block(payload, isize, crc, extra=b"", bsize=None):
    """one BGZF block around a payload; extra: subfields in front of BC"""
    xlen = len(extra) + 6
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536, total
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra + b"BC" +
            struct.pack("<HH", 2, (total - 1) if bsize is None else bsize) + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize))


def text_block(data, payload=None, extra=b"", **kw):
    return block(deflate(data, **kw) if payload is None else payload, len(data), zlib.crc32(data), extra)


# ---- the oracle -------------------------------------------------------------------------------
def walk(raw):
    """the blocks of a file by the rules of bgzf_inflate_parallel: [(payload, crc, isize)] and the bytes they take, or
    None for a file the walk refuses"""
    p, blocks = 0, []
    while p + 18 <= len(raw):
        if raw[p] != 0x1f or raw[p + 1] != 0x8b or raw[p + 2] != 8 or not raw[p + 3] & 4:
            return None
        xlen = raw[p + 10] | raw[p + 11] << 8
        q, bsize = p + 12, None
        while q + 4 <= p + 12 + xlen and q + 4 <= len(raw):
            slen = raw[q + 2] | raw[q + 3] << 8
            if raw[q] == 66 and raw[q + 1] == 67 and slen == 2 and q + 6 <= len(raw):
                bsize = (raw[q + 4] | raw[q + 5] << 8) + 1
            q += 4 + slen
        if bsize is None or p + bsize > len(raw) or bsize < 12 + xlen + 8:
            return None
        crc, isize = struct.unpack("<II", raw[p + bsize - 8:p + bsize])
        if isize > 65536:
            return None
        blocks.append((raw[p + 12 + xlen:p + bsize - 8], crc, isize))
        p += bsize
    return blocks, p


def verdict(raw):
    """zlib's word on a file: None (the frame is refused), or a dict of n_blocks, out_bytes, raw_bytes, good (per block),
    texts (per block; None where refused), bad_block, crc_block"""
    w = walk(raw)
    if w is None:
        return None
    blocks, used = w
    good, texts, bad, crc_bad = [], [], NONE, NONE
    for i, (payload, crc, isize) in enumerate(blocks):
        if isize == 0:
            good.append(True)
            texts.append(b"")
            continue
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(payload, isize + 1)
            ok = d.eof and len(text) == isize
        except zlib.error:
            ok = False
        good.append(ok)
        texts.append(text if ok else None)
        if not ok and bad == NONE:
            bad = i
        if ok and zlib.crc32(text) != crc and crc_bad == NONE:
            crc_bad = i
    return {"n_blocks": len(blocks), "out_bytes": sum(b[2] for b in blocks), "raw_bytes": used, "good": good, "texts": texts,
            "bad_block": bad, "crc_block": crc_bad}


# ---- contents ---------------------------------------------------------------------------------
def bam_records(n=300, seed=5):
    import numpy as np

    from tests import bamgen
    r = np.random.default_rng(seed)
    out = bamgen.header()
    for k in range(n):
        out += bamgen.record(b"read%d_%s" % (k, bamgen.barcode(r, 8)), bamgen.aux_z(b"CR", bamgen.barcode(r, 12)) +
                             bamgen.aux_int(b"NH", 1), pos=100 + k, seq_len=int(r.integers(20, 90)))
    return out


def fibonacci(seed=7):
    r = random.Random(seed)
    a, b, text = 1, 1, bytearray()
    for s in range(22):      # 46 367 bytes: an unlimited Huffman code would be 21 bits deep
        text += bytes([65 + s]) * a
        a, b = b, a + b
    text = list(text)
    r.shuffle(text)
    return bytes(text)


_CONTENTS = {}


def contents():
    if not _CONTENTS:
        from tests.test_pgzip import fastq_text
        r = random.Random(11)
        _CONTENTS.update({
            "empty": b"", "one": b"Q", "fastq": fastq_text(400, 3)[:60000], "bam": bam_records()[:65280], "zeros": bytes(65536),
            "period_32768": r.randbytes(32768) * 2, "period_32769": (r.randbytes(32769) * 2)[:60000],
            "noise": r.randbytes(60000), "fibonacci": fibonacci(), "one_distance": (r.randbytes(100) * 400)[:30011],
        })
    return _CONTENTS


SETTINGS = {
    "l0": dict(level=0), "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9), "fixed": dict(strategy=Z_FIXED),
    "huffman": dict(strategy=Z_HUFFMAN_ONLY), "rle": dict(strategy=Z_RLE), "mem1": dict(mem=1),
}


def with_flushes(data):
    return dict(flushes=((len(data) // 3, zlib.Z_SYNC_FLUSH), (2 * len(data) // 3, zlib.Z_FULL_FLUSH)))


def period_by_hand():
    """the largest distance there is: 32 768 literals, then matches of (258, 32768) - zlib itself stops at 32 506"""
    data = contents()["period_32768"]
    toks = list(data[:32768]) + [(258, 32768)] * 126 + [(130, 32768)] * 2
    return data, fixed_block(toks).bytes()


def one_bit_distance_code():
    """a distance alphabet of ONE code of one bit (incomplete: the shape zlib accepts), all matches at distance 100"""
    data = contents()["one_distance"][:5000]
    lit_lens = [9] * 286
    lit_lens[256] = 1   # end-of-block on one bit, the other 285 symbols share the other half at 9 / 10 bits
    rest = [s for s in range(286) if s != 256]
    for s in rest[:227]:
        lit_lens[s] = 9
    for s in rest[227:]:
        lit_lens[s] = 10     # 227 / 512 + 58 / 1024 = 0.5
    dist_lens = [0] * 13 + [1]   # distance symbol 13: 97 .. 128
    toks = list(data[:100])
    at = 100
    while at < len(data):
        n = min(258, len(data) - at)
        if n < 3:
            toks += list(data[at:at + n])
        else:
            toks.append((n, 100))
        at += n
    return data, dynamic_block(toks, lit_lens, dist_lens).bytes()


def long_codes_by_hand():
    """literal/length codes of every length from 1 to 15 (the slow walk behind the look-up table), no distance codes"""
    lit_lens = [0] * 257
    used = [66 + k for k in range(14)]      # lengths 2 .. 15 for fourteen letters, 15 again for 'A', 1 for end-of-block
    lit_lens[256] = 1
    for k, s in enumerate(used):
        lit_lens[s] = 2 + k
    lit_lens[65] = 15
    r = random.Random(2)
    data = bytes(r.choice(used + [65, 79, 79]) for _ in range(3000))
    return data, dynamic_block(list(data), lit_lens, [0]).bytes()


_FILES = {}


def well_formed():
    """name -> file; every block of every one inflates and has its right CRC"""
    if _FILES:
        return _FILES
    C, F = contents(), _FILES
    for cname, data in C.items():
        for sname, kw in SETTINGS.items():
            if len(deflate(data, **kw)) + 26 <= 65536:
                F["%s-%s" % (cname, sname)] = text_block(data, **kw) + EOF
    for cname in ("fastq", "bam", "zeros"):
        F[cname + "-flushes"] = text_block(C[cname], **with_flushes(C[cname])) + EOF
    F["fastq-mem1-flushes"] = text_block(C["fastq"][:20000], mem=1, **with_flushes(C["fastq"][:20000])) + EOF
    for name, (data, payload) in (("period-by-hand", period_by_hand()), ("one-bit-distance", one_bit_distance_code()),
                                  ("long-codes", long_codes_by_hand())):
        F[name] = text_block(data, payload) + EOF
    F["several-deflate-blocks"] = text_block(b"abcabcabcxyz", _chain()) + EOF
    text = C["fastq"]
    for n in (1, 2, 63, 64, 65):
        piece = max(1, len(text) // 65)
        F["%d-blocks" % n] = b"".join(text_block(text[k * piece:(k + 1) * piece], level=(1, 6, 9)[k % 3]) for k in range(n)) + EOF
    F["subfield-in-front"] = text_block(text[:3000], extra=b"XY" + struct.pack("<H", 0)) + EOF   # XLEN = 10
    F["eof-in-the-middle"] = text_block(text[:700]) + EOF + text_block(text[700:1500]) + EOF
    for stray in (1, 9, 17):
        F["stray-%d" % stray] = text_block(text[:500]) + EOF + bytes([0x1f] * stray)
    F["no-eof-block"] = text_block(text[:500])
    F["nothing"] = b""
    for made in (match_geometry, queue_rounds, sizes, payload_alignment, stored_at_the_window_edge):
        F.update(made())
    return F


def _chain():
    """'abcabcabcxyz' as an empty dynamic block, a fixed block, an empty stored block and a final stored block"""
    b = dynamic_block([], [0] * 256 + [1], [0], False)
    b = fixed_block([97, 98, 99, (6, 3)], False, b)
    b = stored_block(b"", False, b)
    return stored_block(b"xyz", True, b).bytes()


def many_blocks(n):
    """n blocks of about 64 bytes of text each"""
    text = contents()["fastq"]
    return b"".join(text_block(text[(k * 61) % 50000:][:64], level=1 if k & 1 else 6) for k in range(n)) + EOF


# ---- the work around the walk -----------------------------------------------------------------
# What the wavefront does around the one walking lane (staging, the copies of a round's queue, the CRC stripes, the
# flush, the two atomicMin) decides nothing by itself, so a file made by zlib meets its edges only by chance.  These
# files are built to meet them.
def text_of(tokens, text=b""):
    """what tokens (literals and (length, distance) matches) write behind text"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(text):])


GEOMETRY_DISTANCES = list(range(1, 131)) + [191, 192, 193, 255, 256, 257, 258, 259, 511, 512, 513]
GEOMETRY_LENGTHS = [3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258]


def match_geometry():
    """one fixed block per distance d: d + (0 .. 15) literals of noise, then every length around the wavefront's 64 lanes as
    the match (length, d) with a literal of noise behind it.  Noise, so that a byte read too early, too late or from the
    wrong place of the period is another byte."""
    r = random.Random(1)
    blocks = []
    for d in GEOMETRY_DISTANCES:
        toks = list(r.randbytes(d + r.randrange(16)))
        for length in GEOMETRY_LENGTHS:
            toks += [(length, d), r.randrange(256)]
        blocks.append(text_block(text_of(toks), fixed_block(toks).bytes()))
    return {"match-geometry": b"".join(blocks) + EOF}


QUEUE_ENTRIES = (63, 64, 65, 127, 128, 129, 200)


def chained_matches(r, n, text, literal_behind_the_last):
    """n matches, one to three literals of noise between two of them; every match has the length of the one before it as
    its distance, so it reads what that one wrote - the first reads the last bytes of text"""
    toks, d = [], min(len(text), r.randrange(3, 40))
    for k in range(n):
        length = r.choice([3, 4, 17, 63, 64, 65, 128, 258, r.randrange(3, 259), r.randrange(3, 259)])
        toks.append((length, d))
        d = length
        if k + 1 < n or literal_behind_the_last:
            toks += list(r.randbytes(r.randrange(1, 4)))
    return toks


def queue_rounds():
    """blocks of exactly 63 .. 200 queue entries (a match or a non-empty stored run is one, a literal is none; the queue
    holds 64).  In the blocks of 64 and 128 the last entry is the last token and ends at ISIZE.  The last block's entries
    are stored runs - more than the queue holds in a row - and matches that reach back into them."""
    r = random.Random(2)
    blocks = []
    for n in QUEUE_ENTRIES:
        start = r.randbytes(r.randrange(3, 40))
        toks = list(start) + chained_matches(r, n, start, n % 64 != 0)
        assert sum(isinstance(t, tuple) for t in toks) == n and isinstance(toks[-1], tuple) == (n % 64 == 0)
        blocks.append(text_block(text_of(toks), fixed_block(toks).bytes()))
    b, text = Bits(), b""
    for k in range(70):
        run = r.randbytes(r.randrange(1, 40))
        b, text = stored_block(run, False, b), text + run
    for n_stored, n_matches, final in ((0, 30, False), (3, 0, False), (0, 40, True)):
        for k in range(n_stored):
            run = r.randbytes(r.randrange(1, 300))
            b, text = stored_block(run, False, b), text + run
        if n_matches:
            toks = [(r.randrange(3, 259), r.randrange(1, len(text) + 1)), r.randrange(256)] + chained_matches(r, n_matches - 1, text, True)
            b, text = fixed_block(toks, final, b), text + text_of(toks, text)
    blocks.append(text_block(text, b.bytes()))
    return {"queue-rounds": b"".join(blocks) + EOF}


SIZES = list(range(1, 50)) + [254, 255, 256, 257, 509, 510, 511, 4095, 4096, 4097, 65279, 65280, 65281, 65535, 65536]
SIZES_WRONG_CRC = (1, 2, 3, 4, 255, 256, 65280, 65281, 65535, 65536)


@functools.lru_cache(None)
def sizes_blocks():
    """one block per ISIZE of SIZES: the CRC's path for less than four bytes, one stripe and one more, all 256 stripes, a
    head of 1, 255 and 256 bytes in front of them; fastq text and noise in turn under levels 0 to 9, the two largest a
    period of 997 bytes of noise (65 536 bytes of noise are no BGZF block)"""
    r = random.Random(31)
    noise, fastq = r.randbytes(70000), contents()["fastq"]
    period = (r.randbytes(997) * 66)[:65536]
    blocks = []
    for k, n in enumerate(SIZES):
        if n >= 65535:
            data, level = period[65536 - n:], (1, 9)[k & 1]
        elif n >= 65279:
            data, level = noise[k:k + n], (0, 1, 6)[k % 3]
        else:
            data, level = (fastq, noise)[k & 1][5 * k:5 * k + n], (0, 1, 6, 9)[(k // 2) % 4]
        assert len(data) == n
        blocks.append(text_block(data, level=level))
    assert {sum(SIZES[:k]) % 16 for k in range(len(SIZES))} == set(range(16))   # where a block's text starts in the output
    return blocks


def sizes():
    return {"sizes": b"".join(sizes_blocks()) + EOF}


@functools.lru_cache(None)
def sizes_wrong_crc():
    """name -> (file, block): the file above with one bit of one block's stored CRC-32 changed"""
    blocks, out = sizes_blocks(), {}
    for n in SIZES_WRONG_CRC:
        at, bit = SIZES.index(n), (7 * n) % 32
        b = bytearray(blocks[at])
        b[len(b) - 8 + (bit >> 3)] ^= 1 << (bit & 7)
        out["sizes-wrong-crc-%d" % n] = (b"".join(blocks[:at]) + bytes(b) + b"".join(blocks[at + 1:]) + EOF, at)
    return out


def skewed_text(r, n):
    """bytes a Huffman code shortens by a few per cent: Z_HUFFMAN_ONLY makes ONE dynamic block of them, every bit of
    which is read through the staging windows (noise, which zlib stores, would be copied from the file itself)"""
    return bytes(min(255, int(r.expovariate(0.012))) for _ in range(n))


def huffman_payload(data):
    payload = deflate(data, strategy=Z_HUFFMAN_ONLY)
    assert (payload[0] >> 1) & 3 == 2 and len(payload) > 3 * 4096, len(payload)   # dynamic; more than three windows
    return payload


def payload_alignment():
    """16 blocks; block k has a subfield of k bytes in front of BC, and its payload - of a text of 14 000 + k bytes, more
    than three staging windows long - has the length that puts the NEXT payload's start three residues mod 16 further,
    so the starts take all 16 (the file's first byte lies at a multiple of 16 on the device) and the ends eight"""
    r = random.Random(41)
    out, starts, ends = b"", set(), set()
    for k in range(16):
        extra = b"XY" + struct.pack("<H", k) + r.randbytes(k)
        start = len(out) + 12 + len(extra) + 6
        for attempt in range(2000):
            data = skewed_text(r, 14000 + k)
            payload = huffman_payload(data)
            if k == 15 or (len(payload) + 8 + 12 + len(extra) + 1 + 6) % 16 == 3:   # (the next subfield is a byte longer)
                break
        else:
            raise AssertionError("no payload of the length block %d needs" % k)
        starts.add(start % 16)
        ends.add((start + len(payload)) % 16)
        out += text_block(data, payload, extra)
        assert walk(out)[0][k][0] == payload and out[start:start + len(payload)] == payload
    assert starts == set(range(16)) and len(ends) >= 8, (starts, ends)
    return {"payload-alignment": out + EOF}


def stored_at_the_window_edge():
    """for k in -6 .. 6 a payload that starts at a multiple of 16 and whose first stored block ends at byte 4096 + k, the
    end of the first staged window: the header of the fixed block behind it, and that of the stored block behind that
    one, lie on every offset around a window's edge, and twice the walk jumps over bytes that were never staged"""
    r = random.Random(43)
    out = b""
    for k in range(-6, 7):
        extra = b"XY" + struct.pack("<H", -(len(out) + 22) % 16) + bytes(-(len(out) + 22) % 16)
        assert (len(out) + 12 + len(extra) + 6) % 16 == 0
        text = r.randbytes(4096 + k - 5)
        b = stored_block(text, False)
        assert len(b.bytes()) == 4096 + k
        toks = ([r.randrange(256), (40, len(text) - 7), r.randrange(256), (258, 300), (5, 1), (200, len(text) + 40 + 2)] +
                list(r.randbytes((k + 6) % 5)) + [(70, 64), (3, 4096 + k - 9)])
        b, text = fixed_block(toks, False, b), text + text_of(toks, text)
        last = r.randbytes(5000)
        b, text = stored_block(last, True, b), text + last
        out += text_block(text, b.bytes(), extra)
    return {"stored-at-the-window-edge": out + EOF}


def cut_payloads():
    """name -> (whole text, payload): the dynamic block of payload_alignment, and 14 000 bytes of noise, which zlib stores"""
    r = random.Random(47)
    data, noise = skewed_text(r, 14000), r.randbytes(14000)
    stored = deflate(noise, strategy=Z_HUFFMAN_ONLY)
    assert len(stored) == 14005 and stored[0] == 1
    return {"cut-at-the-window-edge": (data, huffman_payload(data)), "cut-stored-at-the-window-edge": (noise, stored)}


@functools.lru_cache(None)
def cut_at_the_window_edge():
    """payloads cut short at their end and around the ends of the staged windows, behind a good block; ISIZE and CRC are
    those of the whole text.  What follows a cut payload is its CRC-32, which is not zero: a walk that read on there
    instead of taking zeros would not stop where zlib does.  zlib refuses every one, or this sweep has lost its purpose."""
    D = {}
    good = text_block(contents()["fastq"][:100])
    for name, (data, payload) in cut_payloads().items():
        n = len(payload)
        cuts = sorted({n - k for k in (1, 2, 3, 4, 5, 8, 9)} | {4096 + k for k in range(-3, 4)} | {8192 + k for k in range(-3, 4)} |
                      {3072 + k for k in (-1, 0, 1)})
        assert len(cuts) == 24 and zlib.crc32(data) & 0xFF and zlib.crc32(data) >> 24
        for c in cuts:
            D["%s-%d" % (name, c)] = good + block(payload[:c], len(data), zlib.crc32(data)) + EOF
            assert verdict(D["%s-%d" % (name, c)])["bad_block"] == 1, (name, c)
    return D


def several_findings():
    """150 small blocks with three refused ones (each for another reason) and three wrong CRCs among them: the first of
    either kind is chosen among candidates that workgroups report in any order.  In the second file the first wrong CRC
    lies behind the first refused block."""
    text = contents()["fastq"]
    r = random.Random(53)
    good, at = [], 0
    for k in range(150):
        n = r.randrange(20, 200)
        good.append(text_block(text[at:at + n], level=(1, 6, 9, 0)[k % 4]))
        at += n
    b = Bits()
    b.put(1, 1)
    b.put(3, 2)
    refused = {"type-3": block(b.bytes() + b"\0\0\0\0", 5, zlib.crc32(b"hello")),
               "distance": block(fixed_block([97, 98, 99, (6, 4)]).bytes(), 9, zlib.crc32(b"abcabcabc")),
               "isize": block(deflate(text[:301]), 300, zlib.crc32(text[:300]))}

    def wrong(raw):
        return raw[:-8] + bytes([raw[-8] ^ 0x10]) + raw[-7:]

    D = {}
    for name, bad, crc in (("several-findings", {5: "type-3", 9: "distance", 40: "isize"}, (3, 7, 60)),
                           ("several-findings-crc-behind", {5: "distance", 9: "isize", 40: "type-3"}, (7, 60))):
        blocks = [refused[bad[k]] if k in bad else wrong(g) if k in crc else g for k, g in enumerate(good)]
        D[name] = b"".join(blocks) + EOF
        v = verdict(D[name])
        assert (v["bad_block"], v["crc_block"]) == (5, crc[0]) and v["good"].count(False) == 3
    return D


def malformed_frames():
    """name -> file the header walk refuses"""
    good = text_block(contents()["fastq"][:800])
    M = {}
    M["magic"] = b"\x1e" + good[1:]
    M["method"] = good[:2] + b"\x07" + good[3:]
    M["no-fextra"] = good[:3] + b"\x00" + good[4:]
    M["no-bc"] = good[:12] + b"BD" + good[14:]
    M["bc-of-length-3"] = good[:14] + struct.pack("<H", 3) + good[16:]
    M["bsize-past-the-file"] = good + good[:-1]
    M["bsize-too-small"] = block(b"", 0, 0, bsize=24) + good          # 25 bytes < 12 + 6 + 8
    M["isize-above-65536"] = block(deflate(b"a"), 65537, zlib.crc32(b"a")) + EOF
    M["second-block-wrong"] = good + b"\x00" * 40
    return M


def damaged():
    """name -> a small file with one damaged payload; what is expected of each is zlib's word (verdict)"""
    text = contents()["fastq"]
    D = {}
    r = random.Random(23)
    for k in range(40):
        data = text[k * 97:][:r.randrange(40, 400)]
        payload = bytearray(deflate(data, level=(1, 6, 9)[k % 3], strategy=(0, 0, Z_FIXED, Z_HUFFMAN_ONLY)[k % 4]))
        bit = r.randrange(len(payload) * 8)
        payload[bit >> 3] ^= 1 << (bit & 7)
        D["flip-%02d" % k] = (text_block(text[:300]) + text_block(text[300:500]) + text_block(data, bytes(payload)) +
                              text_block(text[500:900]) + EOF)
    one = lambda data, payload, isize=None: (text_block(text[:200]) + block(payload, len(data) if isize is None else isize,
                                                                             zlib.crc32(data)) + EOF)
    D["len-nlen"] = one(b"hello", stored_block(b"hello", nlen=0x1234).bytes())
    b = Bits()
    b.put(1, 1)
    b.put(3, 2)
    D["type-3"] = one(b"hello", b.bytes() + b"\0\0\0\0")
    D["hlit-287"] = one(b"a", dynamic_block([97], [8] * 286, [5] * 30, hlit=287).bytes())
    D["hdist-31"] = one(b"a", dynamic_block([97], [8] * 256 + [1], [5] * 30, hdist=31).bytes())
    D["distance-beyond-the-start"] = one(b"abcabcabc", fixed_block([97, 98, 99, (6, 4)]).bytes())
    D["distance-at-the-start"] = one(b"abcabcabc", fixed_block([97, 98, 99, (6, 3)]).bytes())     # accepted
    D["cut-short"] = one(text[:300], deflate(text[:300])[:-1])
    D["isize-plus-one"] = one(text[:300], deflate(text[:301]), 300)
    D["isize-minus-one"] = one(text[:300], deflate(text[:299]), 300)
    D["length-symbol-286"] = one(b"aaaa", fixed_block([97, ("raw", 286, 0, 0, 0, 0, 0)]).bytes())
    D["distance-symbol-30"] = one(b"aaaa", fixed_block([97, ("raw", 257, 0, 0, 30, 0, 0)]).bytes())
    D["no-end-of-block-code"] = one(b"a", dynamic_block([97], [8] * 256 + [0], [5] * 30).bytes())
    D["oversubscribed-literals"] = one(b"a", dynamic_block([], [1, 1, 1] + [0] * 253 + [2], [0]).bytes())
    D["incomplete-literals"] = one(b"a", dynamic_block([], [2] + [0] * 255 + [2], [0]).bytes())
    D["incomplete-distances"] = one(b"a", dynamic_block([], [1] + [0] * 255 + [1], [2, 2]).bytes())
    D["oversubscribed-distances"] = one(b"a", dynamic_block([], [1] + [0] * 255 + [1], [1, 1, 1]).bytes())
    D["code-length-code-incomplete"] = one(b"a", dynamic_block([], [1] + [0] * 255 + [1], [0], cl_lens=[4] * 15 + [0] * 4).bytes())
    D["code-length-code-oversubscribed"] = one(b"a", dynamic_block([], [1] + [0] * 255 + [1], [0], cl_lens=[4] * 16 + [4, 0, 0]).bytes())
    D["repeat-with-nothing-before"] = one(b"a", dynamic_block([], [0] * 257, [0], cl_lens=[2, 2] + [0] * 14 + [2, 2, 0],
                                                                 cl_syms=[(16, 2, 0)]).bytes())
    D["repeat-past-the-end"] = one(b"a", dynamic_block([], [0] * 257, [0], cl_lens=[2, 2] + [0] * 14 + [2, 2, 0],
                                                          cl_syms=[1, (17, 3, 7)] + [1] + [(17, 3, 7)] * 24 + [1, 1, (17, 3, 7)]).bytes())
    D["unused-distance-code"] = one(b"aaaa", dynamic_block([97, 257], [0] * 97 + [1] + [0] * 158 + [2, 2], [0]).bytes() + b"\0\0")
    D["stored-past-the-input"] = one(b"hello", stored_block(b"hello").bytes()[:-2])
    D["stored-past-isize"] = one(b"hello", stored_block(b"hello!").bytes(), 5)
    D["wrong-crc"] = text_block(text[:200]) + block(deflate(text[200:700]), 500, 12345) + text_block(text[700:900]) + EOF  # accepted
    D.update(cut_at_the_window_edge())
    D.update(several_findings())
    D.update({name: raw for name, (raw, _) in sizes_wrong_crc().items()})   # accepted
    return D


def sweeps():
    """the names in damaged() of the two sweeps, which have tests of their own"""
    return sorted(cut_at_the_window_edge()), sorted(sizes_wrong_crc())


# Why the decoder core refuses the first refused block of the hand-made files of damaged() (fqg_inflate_core.h: kInfBad*;
# include/fqg_codes.h: FQG_E_INFLATE_*).  zlib has no such number; these were read off the core once and are kept.
REASONS = {
    "type-3": 32,
    "len-nlen": 33,
    "hlit-287": 34, "hdist-31": 34, "no-end-of-block-code": 34, "oversubscribed-literals": 34, "incomplete-literals": 34,
    "incomplete-distances": 34, "oversubscribed-distances": 34, "code-length-code-incomplete": 34,
    "code-length-code-oversubscribed": 34, "repeat-with-nothing-before": 34, "repeat-past-the-end": 34,
    "length-symbol-286": 35, "distance-symbol-30": 35, "unused-distance-code": 35,
    "distance-beyond-the-start": 36,
    "isize-plus-one": 37, "isize-minus-one": 37, "stored-past-isize": 37,
    "cut-short": 38, "stored-past-the-input": 38,
    "several-findings": 32, "several-findings-crc-behind": 36,
}


def reason(name):
    """the reason a file of damaged() is refused for, or None where this table does not say (the flipped bits)"""
    return 38 if name in cut_at_the_window_edge() else REASONS.get(name)
