"""SAM text of fastq_pre_barcodes -> the BAM stream samtools 0.1.19 makes of it, or "refused, line n".

A restatement of what `samtools view -b` does to the text `fastq_pre_barcodes --sam` prints (sh/fastq2bam):
sam_header_read + sam_read1 (bam_import.c:216-467) and bam_header_write + bam_write1 (bam.c), for lines of the one
shape that program prints:

    <number> TAB <flag> TAB * TAB 0 TAB 255 TAB * TAB * TAB 0 TAB <tlen> TAB <SEQ> TAB <QUAL> { TAB xx:Z:<value> }

The branches of sam_read1 such a line can reach:
  * fields end at every isspace() byte except the blank (kseq.h KS_SEP_TAB: 9..13), and a '\\n' or '\\r' ends the
    record: a byte 9..13 inside a string moves every later field.  Refused (stricter than libbam in the one sub-case
    where the pieces happen to be well-formed fields again).
  * name: the field up to its first NUL, with the NUL; flag: strtol; "*" -> tid -1 (no @SQ line: any other name
    leaves with "missing header"); pos, mpos "0" -> atoi - 1 = -1; mapq 255; CIGAR "*": no operations,
    bin = reg2bin(-1, 0) = 4680; isize = atoi(column 9).
  * SEQ: "*" -> l_qseq 0 and a NULL pointer that the QUAL loop then offsets (refused: memory libbam does not own,
    although nothing is written through it when QUAL is "*" too); else l_qseq = strlen and
    bam_nt16_table[(int)char] per base - a char >= 0x80 is a negative index (refused).
  * QUAL: not "*" and strlen != l_qseq -> parse_error "sequence and quality are inconsistent", abort (refused);
    "*" -> 0xff per base, else byte - 33.
  * aux: every further field needs str->l >= 6 and ':' at [2] and [4], else parse_error "missing colon in auxiliary
    data", abort: an EMPTY Z value ("on:Z:") is refused.  Type Z: tag, 'Z', value, NUL.
  * an empty SEQ field gives l_qseq 0; the program prints an empty QUAL with it or a QUAL of another length (the
    lengths come from two lines of the FASTQ record), and an empty QUAL is an empty op:Z: value: refused either way,
    so "an empty SEQ or QUAL field" is refused as a rule of its own.
"""
import struct

# bam_nt16_table, bam_import.c:17-34 (data: the table's 256 values)
NT16 = [15] * 256
for _c, _v in zip("=ACMGRSVTWYHKDBN", range(16)):
    NT16[ord(_c)] = _v
    NT16[ord(_c.lower())] = _v
for _i, _v in enumerate((1, 2, 4, 8)):
    NT16[ord("0") + _i] = _v

CUTS = frozenset((9, 11, 12, 13))  # (10 ends the line before this module sees it)
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


class Refused(Exception):
    def __init__(self, line, why):
        super().__init__("line %d: %s" % (line, why))
        self.line, self.why = line, why


def header(text: bytes) -> bytes:
    """bam_header_write of the header lines, kept verbatim; no reference sequences"""
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)


def header_for_argv(argv0, argv) -> bytes:
    """the header of `argv0 argv...` (the reference leaves the last argument out of the @PG line)"""
    words = [argv0] + list(argv[:-1])
    return header(b"@HD\tVN:1.0 SO:unknown\n@PG\tID:1 PN:fastq_pre_barcodes CL:" + " ".join(words).encode("latin-1") + b"\n")


def record(line: bytes, n: int) -> bytes:
    """one alignment line (without its '\\n') -> block_size + record"""
    f = line.split(b"\t")
    if len(f) < 11:
        raise Refused(n, "fewer than 11 fields")
    for s in f:
        if any(c in CUTS for c in s):
            raise Refused(n, "a byte libbam cuts fields at inside a field")
    name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if (rname, pos, mapq, cigar, rnext, pnext) != (b"*", b"0", b"255", b"*", b"*", b"0"):
        raise Refused(n, "not a line of fastq_pre_barcodes")
    if not seq or not qual:
        raise Refused(n, "empty SEQ or QUAL")
    if seq == b"*":
        raise Refused(n, "SEQ is *")
    if any(c >= 0x80 for c in seq):
        raise Refused(n, "base >= 0x80")
    if qual != b"*" and len(qual) != len(seq):
        raise Refused(n, "sequence and quality are inconsistent")
    l_seq = len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i, c in enumerate(seq):
        packed[i // 2] |= NT16[c] << (4 * (1 - i % 2))
    q = b"\xff" * l_seq if qual == b"*" else bytes((c - 33) & 0xFF for c in qual)
    aux = b""
    for a in f[11:]:
        if len(a) < 6 or a[2:3] != b":" or a[4:5] != b":":
            raise Refused(n, "missing colon in auxiliary data")
        if a[3:4] != b"Z":
            raise Refused(n, "not a line of fastq_pre_barcodes")
        aux += a[:2] + b"Z" + a[5:] + b"\0"
    qname = name + b"\0"
    body = struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | (255 << 8) | len(qname), int(flag) << 16, l_seq, -1, -1,
                       int(tlen) - (1 << 32) if int(tlen) >= 1 << 31 else int(tlen))
    body += qname + bytes(packed) + q + aux
    return struct.pack("<i", len(body)) + body


def sam2bam(sam: bytes):
    """-> dict(header, records: [bytes], refused: None or (line number as libbam counts it, 1 = the first line of the
    text; why)).  records holds what lies in front of a refused line."""
    lines = sam.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    n_head = 0
    while n_head < len(lines) and lines[n_head].startswith(b"@"):
        n_head += 1
    out = {"header": header(b"".join(ln + b"\n" for ln in lines[:n_head])), "records": [], "refused": None}
    for i in range(n_head, len(lines)):
        try:
            out["records"].append(record(lines[i], i + 1))
        except Refused as e:
            out["refused"] = (e.line, e.why)
            break
    return out


def stream(sam: bytes) -> bytes:
    r = sam2bam(sam)
    if r["refused"]:
        raise Refused(*r["refused"])
    return r["header"] + b"".join(r["records"])


def bgzf_inflate(raw: bytes):
    """-> (the inflated stream, [ISIZE of every block])"""
    import zlib
    out, sizes, p = [], [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 12:p + 16] == b"BC\x02\x00", "not a BGZF block at %d" % p
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        assert isize == len(data) and zlib.crc32(data) == crc
        out.append(data)
        sizes.append(isize)
        p += bsize
    return b"".join(out), sizes
