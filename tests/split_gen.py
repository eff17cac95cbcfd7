"""Seeded interleaved FASTQ inputs for fastq_split_interleaved: the small ones that tools/gen_golden.py commits under
tests/golden/data (syn_split_*.fastq.gz), and the large ones that the golden generator and the GPU test both make
from the same seed (no GPU, no product code in here)."""
import numpy as np

STYLES = ("casava", "slash", "nosuffix")


def _name(style, i, mate):
    if style == "casava":
        return b"@SPL:7:FC1:%d:%d:%d:%d %d:N:0:ACGTAC" % (1 + i % 8, 1101 + i % 17, 1000 + 13 * i, 2000 + 7 * i, mate)
    if style == "slash":
        return b"@split_read_%d/%d" % (i, mate)
    return b"@split_read_%d" % i


def record(rng, style, i, mate, length):
    seq = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, length, p=[0.247, 0.247, 0.247, 0.247, 0.012])].tobytes()
    qual = (rng.integers(2, 41, length) + 33).astype(np.uint8).tobytes()
    return _name(style, i, mate) + b"\n" + seq + b"\n+\n" + qual + b"\n"


def pairs(seed, n_pairs, style="casava", len1=(30, 151), len2=None):
    """a list of 2 * n_pairs records, mates alternating; lengths drawn from [lo, hi)"""
    rng = np.random.default_rng(seed)
    len2 = len2 or len1
    out = []
    for i in range(n_pairs):
        out.append(record(rng, style, i, 1, int(rng.integers(*len1))))
        out.append(record(rng, style, i, 2, int(rng.integers(*len2))))
    return out


def lines_of(image):
    """the lines of an image with their newlines (a last line may lack one)"""
    parts = image.split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def _lines(rec, k):
    """the first k lines of a record"""
    return b"".join(lines_of(rec)[:k])


def small_files():
    """name -> plain bytes of the committed fixtures"""
    f = {}
    for s, style in enumerate(STYLES):
        f["syn_split_clean_%s" % style] = b"".join(pairs(100 + s, 24, style))
    base = pairs(7, 20)
    other = pairs(8, 20)  # (other coordinates in the names)
    for where, k in (("pair0", 0), ("mid", 11)):
        r = list(base)
        r[2 * k + 1] = other[2 * k + 3]
        f["syn_split_mismatch_%s" % where] = b"".join(r)
    for mate in (1, 2):
        r = list(base)
        k = 2 * 7 + mate - 1
        ln = r[k].split(b"\n")
        ln[1] = ln[1][:5] + b"X" + ln[1][6:]
        r[k] = b"\n".join(ln)
        f["syn_split_invalid_m%d" % mate] = b"".join(r)
        for nl in (1, 2, 3):
            f["syn_split_trunc_m%d_l%d" % (mate, nl)] = b"".join(base[:2 * 9 + mate - 1]) + _lines(base[2 * 9 + mate - 1], nl)
    f["syn_split_odd"] = b"".join(base[:2 * 9 + 1])
    f["syn_split_no_final_newline"] = b"".join(base)[:-1]
    f["syn_split_empty"] = b""
    r = list(base)
    r[8] = r[8].replace(b"N:0:ACG", b"N:0:A\0G", 1)    # behind the blank: the name is whole, the line a shorter C string
    r[13] = r[13].replace(b"\n+\n", b"\n+\0tail\n", 1)
    f["syn_split_nul_in_header"] = b"".join(r)
    r = list(base)
    ln = r[10].split(b"\n")
    ln[1] = ln[1][:9] + b"\0" + ln[1][10:]
    r[10] = b"\n".join(ln)
    f["syn_split_nul_in_sequence"] = b"".join(r)
    f["syn_split_mates_26_150"] = b"".join(pairs(9, 24, "casava", (26, 27), (150, 151)))
    return f


# ---- the large inputs: about 3 MiB, records of uneven size so that pieces of 1 MiB frame odd numbers of records --------
BIG_PAIRS = 6600


def big_clean():
    return pairs(23, BIG_PAIRS, "casava", (60, 151), (20, 151))


def big_files():
    """name -> plain bytes: the clean file, a copy with a mismatching pair and a copy cut short, both in the second MiB"""
    recs = big_clean()
    out = {"big_clean.fastq": b"".join(recs)}
    at, size = None, 0
    for i, r in enumerate(recs):
        size += len(r)
        if size > (3 << 19) and i % 2 == 1:  # 1.5 MiB: inside the second piece of FQGPU_CHUNK_MB=1
            at = i
            break
    other = pairs(22, 4)
    r = list(recs)
    r[at] = other[3]
    out["big_mismatch.fastq"] = b"".join(r)
    out["big_trunc.fastq"] = b"".join(recs[:at]) + _lines(recs[at], 2)
    return out


def deinterleave(image):
    """what fastq_split_interleaved writes for a clean image: (mates 1, mates 2), every line as the C string gzgets leaves
    (it ends at its first NUL byte, and then has no newline)"""
    lines = lines_of(image)
    out = ([], [])
    for k in range(0, len(lines) - len(lines) % 8, 4):
        for ln in lines[k:k + 4]:
            out[(k // 4) % 2].append(ln.split(b"\0")[0] if b"\0" in ln else ln)
    return b"".join(out[0]), b"".join(out[1])
