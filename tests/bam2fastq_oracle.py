"""bam2fastq restated in plain Python (reference src/bam2fastq.c, libbam 0.1.19 underneath): the option table, the
alignment loop (:249-355) with its routing, aux-tag lookups, read-name repair and messages, over an INFLATED BAM stream.
Test infrastructure: tests/test_oracle_bam2fastq.py pins it to the reference's recorded runs (tests/golden/bam2fastq.json),
tests/test_gpu_bam2fastq.py compares the GPU bulk call with it.

Two inputs have no defined output in the reference and raise Refused here: a read of 10 000 bases or
more (10 000-byte stack buffers, :242-243), and a record whose aux walk or C strings would leave the record."""
import struct

VERSION = "0.25.3"
USAGE = "\nERROR: Usage: bam2fastq --bam in.bam --out fastq_prefix [--verbose --10x|-X]\n"
NT16 = b"=ACMGRSVTWYHKDBN"
PAIRS = [bytes((NT16[b >> 4], NT16[b & 15])) for b in range(256)]
PLUS33 = bytes((33 + b) & 0xFF for b in range(256))
BUF_SIZE = 10000
R1, R2, CELL, SAMPLE, UMI, SE, I1 = 0, 1, 2, 3, 4, 5, 2
EXT = ["_1", "_2", "_cell", "_sample", "_umi", ""]
EXT_10X = ["_R1", "_R2", "_I1"]
UNUSED = 0xFFFFFFFFFFFFFFFF
# finding codes, include/fqg_codes.h
E_CELL, E_CELL_QUAL, E_UMI, E_UMI_QUAL, E_SAMPLE_QUAL, E_NOT_FASTQ2BAM, E_TOO_LONG, E_AUX = 24, 25, 26, 27, 28, 29, 30, 31
FATAL_TEXT = {E_CELL: "missing cell tag in entry  %d\n", E_CELL_QUAL: "missing cell quality tag in entry  %d\n",
              E_UMI: "missing umi tag in entry  %d\n", E_UMI_QUAL: "missing umi quality tag in entry  %d\n"}
TAGS = (b"on", b"op", b"CR", b"CY", b"RX", b"QX", b"UB", b"UY", b"BC", b"QT")


class Refused(Exception):
    def __init__(self, code, record):
        Exception.__init__(self, "code %d at record %d" % (code, record))
        self.code, self.record = code, record


class Fatal(Exception):
    """a FATAL_ERROR of the loop: finding code, record index, exit status, message"""
    def __init__(self, code, record, status, text):
        Exception.__init__(self, text)
        self.code, self.record, self.status, self.text = code, record, status, text


def header_end(raw):
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    return p


def record_offsets(raw):
    """bam_read1 until it fails: a record that does not end inside the stream ends the loop"""
    p, offs = header_end(raw), []
    while p + 4 <= len(raw):
        block = struct.unpack_from("<i", raw, p)[0]
        if block < 32 or p + 4 + block > len(raw):
            break
        offs.append(p)
        p += 4 + block
    return offs


def _type2size(t):  # bam.h bam_aux_type2size
    return 1 if t in b"CcA" else 2 if t in b"Ss" else 4 if t in b"IifF" else 0


def _walk(rec, s):
    """bam_aux_get's walk over rec[s:], once: {tag: offset of its type byte} for the first field of every name.
    None when the walk reads or steps behind the record."""
    end, found = len(rec), {}
    while s < end:
        if s + 2 > end:
            return None
        found.setdefault(rec[s:s + 2], s + 2)
        s += 2
        if s >= end:
            return None
        t = rec[s:s + 1].upper()  # __skip_tag upper-cases the type ('d' becomes 'D': size 0)
        s += 1
        if t in (b"Z", b"H"):
            z = rec.find(b"\0", s)
            if z < 0:
                return None
            s = z + 1
        elif t == b"B":
            if s + 5 > end:
                return None
            cnt = struct.unpack_from("<i", rec, s + 1)[0]
            if cnt < 0:
                return None
            s += 5 + _type2size(rec[s:s + 1]) * cnt
        else:
            s += _type2size(t)
        if s > end:
            return None
    return found


def _cstr(b):
    z = b.find(b"\0")
    return b if z < 0 else b[:z]


def restore_read_name(s):  # :128-143, on a copy; returns (name, pos)
    s = bytearray(s)
    i, n = 0, len(s)
    at = lambda k: s[k] if k < n else 0
    while i < n:
        if s[i] == 0x40:
            s[i] = 0x20
            if at(i + 1) in (0x31, 0x32) and at(i + 2) == 0x3A:
                i += 1
                break
        i += 1
    if i >= n:
        i = 0
    return s, i


def convert(raw, tenx=False, offsets=None, first_alignment=0, warned=False):
    """The loop over the alignments at `offsets` (default: all).  Returns a dict: n_alignments, streams (six byte
    strings, three used with tenx), first_record[6], warn_record, and `fatal` (a Fatal, or None): everything describes
    the records BEFORE the fatal one.  Raises Refused."""
    offs = record_offsets(raw) if offsets is None else list(offsets)
    out = [bytearray() for _ in range(6)]
    first = [UNUSED] * 6
    res = {"n_alignments": len(offs), "streams": out, "first_record": first, "warn_record": UNUSED, "fatal": None,
           "opens_at_fatal": []}

    def put(stream, k, *parts):
        if first[stream] == UNUSED:
            first[stream] = k
        for p in parts:
            out[stream] += p

    for k, o in enumerate(offs):
        num = first_alignment + k + 1
        block = struct.unpack_from("<i", raw, o)[0]
        rec = raw[o + 4:o + 4 + block]
        x = struct.unpack_from("<8I", rec, 0)
        l_qname, flag, n_cigar, l_qseq = x[2] & 0xFF, x[3] >> 16, x[3] & 0xFFFF, x[4]
        if flag & 0x100:
            continue
        seq_at = 32 + l_qname + 4 * n_cigar
        aux_at = seq_at + (l_qseq + 1) // 2 + l_qseq
        if aux_at > len(rec):
            raise Refused(E_AUX, k)
        tags = _walk(rec, aux_at)
        if tags is None or rec.find(b"\0", 32) < 0:
            raise Refused(E_AUX, k)
        if l_qseq >= BUF_SIZE:
            raise Refused(E_TOO_LONG, k)

        def get_tag(name):  # NULL -> None; present but not Z / H -> the empty string
            s = tags.get(name)
            if s is None:
                return None
            return _cstr(rec[s + 1:]) if rec[s:s + 1] in (b"Z", b"H") else b""

        seq = b"".join(PAIRS[b] for b in rec[seq_at:seq_at + (l_qseq + 1) // 2])[:l_qseq]
        hdr, qual = get_tag(b"on"), get_tag(b"op")
        if hdr is None:
            if not warned and res["warn_record"] == UNUSED:
                res["warn_record"] = k
                if tenx:
                    res["fatal"] = Fatal(E_NOT_FASTQ2BAM, k, 1, "Unable to continue - bam file was not generated by fastq2bam\n")
                    return res
            name = _cstr(rec[32:])
            q = _cstr(rec[seq_at + (l_qseq + 1) // 2:aux_at].translate(PLUS33))
            to = SE if not flag & 1 else R1 if flag & 4 else R2
            suffix = b"" if to == SE else b"/%d" % (to + 1)
            put(to, k, b"@", name, suffix, b"\n", seq, b"\n+\n", q, b"\n")
        elif tenx:
            cell, cell_q = get_tag(b"CR"), get_tag(b"CY")
            umi = get_tag(b"RX")
            umi = get_tag(b"UB") if umi is None else umi
            umi_q = get_tag(b"QX")
            umi_q = get_tag(b"UY") if umi_q is None else umi_q
            for code, v in ((E_CELL, cell), (E_CELL_QUAL, cell_q), (E_UMI, umi), (E_UMI_QUAL, umi_q)):
                if v is None:
                    res["fatal"] = Fatal(code, k, 3, FATAL_TEXT[code] % num)
                    return res
            sample, sample_q = get_tag(b"BC"), get_tag(b"QT")
            if sample is not None and sample_q is None:
                res["fatal"] = Fatal(E_SAMPLE_QUAL, k, 3, "missing sample quality tag in entry  %d for sample %s\n" % (num, sample.decode("latin-1")))
                res["opens_at_fatal"] = [R1] if first[R1] == UNUSED else []
                return res
            name, pos = restore_read_name(hdr)
            suf = (lambda t: b"/%d" % (t + 1)) if pos == 0 else (lambda t: b"")
            if pos:
                name[pos] = 0x31
            put(R1, k, b"@", name, suf(R1), b"\n", cell, umi, b"\n+\n", cell_q, umi_q, b"\n")
            if sample is not None:
                put(I1, k, b"@", name, suf(I1), b"\n", sample, b"\n+\n", sample_q, b"\n")
            if pos:
                name[pos] = 0x32
            put(R2, k, b"@", name, suf(R2), b"\n", seq, b"\n+\n", qual or b"", b"\n")
        elif not flag & 1 or flag & 0x40:
            put(R1 if flag & 1 else SE, k, b"@", hdr, b"\n", seq, b"\n+\n", qual or b"", b"\n")
            for to, a, b in ((CELL, b"CR", b"CY"), (UMI, b"RX", b"QX"), (SAMPLE, b"BC", b"QT")):
                if get_tag(a) is not None:
                    put(to, k, b"@", hdr, b"\n", get_tag(a), b"\n+\n", get_tag(b) or b"", b"\n")
        else:
            put(R2, k, b"@", hdr, b"\n", seq, b"\n+\n", qual or b"", b"\n")
    return res


# ---- the program ------------------------------------------------------------------------------------------------------
LONG = [("verbose", 0, None), ("help", 0, None), ("bam", 1, "b"), ("out", 1, "o"), ("10xV2", 0, None), ("10xV3", 0, None)]
SHORT = {"X": 0, "b": 1, "o": 1, "h": 0}


def parse_args(argv):
    """glibc getopt_long with the table of :180-196 (options may stand anywhere, long names may be abbreviated).
    Returns ({bam, out, help, tenx}, stderr text of getopt itself)."""
    opt = {"bam": None, "out": None, "help": False, "tenx": False}
    err, i = "", 0

    def take(name, val):
        if name in ("b", "bam"):
            opt["bam"] = val
        elif name in ("o", "out"):
            opt["out"] = val
        elif name in ("h", "help"):
            opt["help"] = True
        elif name in ("X", "10xV2", "10xV3"):
            opt["tenx"] = True

    while i < len(argv):
        a = argv[i]
        i += 1
        if a == "--":
            break
        if a.startswith("--"):
            name, eq, val = a[2:].partition("=")
            hits = [l for l in LONG if l[0] == name] or [l for l in LONG if l[0].startswith(name)]
            if not hits:
                err += "bam2fastq: unrecognized option '--%s'\n" % name
            elif len(hits) > 1:
                err += "bam2fastq: option '--%s' is ambiguous; possibilities:%s\n" % (name, "".join(" '--%s'" % h[0] for h in hits))
            elif hits[0][1]:
                if eq:
                    take(hits[0][0], val)
                elif i < len(argv):
                    take(hits[0][0], argv[i])
                    i += 1
                else:
                    err += "bam2fastq: option '--%s' requires an argument\n" % hits[0][0]
            elif eq:
                err += "bam2fastq: option '--%s' doesn't allow an argument\n" % hits[0][0]
            else:
                take(hits[0][0], None)
        elif a.startswith("-") and len(a) > 1:
            j = 1
            while j < len(a):
                c = a[j]
                j += 1
                if c not in SHORT:
                    err += "bam2fastq: invalid option -- '%s'\n" % c
                elif SHORT[c]:
                    if j < len(a):
                        take(c, a[j:])
                    elif i < len(argv):
                        take(c, argv[i])
                        i += 1
                    else:
                        err += "bam2fastq: option requires an argument -- '%s'\n" % c
                    break
                else:
                    take(c, None)
    return opt, err


def run(argv, read_file, stdin=b"", writable=lambda name: True):
    """bam2fastq argv...: (exit status, stderr, {file name: inflated bytes} in the order they were opened).
    read_file(path) -> the INFLATED bytes of a BAM file, or None when it cannot be opened."""
    err = "bam2fastq version %s\n" % VERSION
    opt, e = parse_args(argv)
    err += e
    if opt["help"]:
        return 0, err + USAGE, {}
    if opt["bam"] is None or opt["out"] is None:
        return 1, err + USAGE, {}
    raw = stdin if opt["bam"] == "-" else read_file(opt["bam"])
    if raw is None:
        return 1, err + "open: No such file or directory\n\nERROR: Failed to open BAM file %s\n" % opt["bam"], {}
    err += "Processing %s\n" % opt["bam"]
    tenx = opt["tenx"]
    res = convert(raw, tenx=tenx)
    ext = EXT_10X if tenx else EXT
    order = {R1: 0, R2: 2, I1: 1} if tenx else {R1: 0, SE: 0, R2: 0, CELL: 1, UMI: 2, SAMPLE: 3}
    fatal = res["fatal"]
    n_seen = fatal.record + 1 if fatal else res["n_alignments"]
    events = [(k - 1, -2, "\b" * 15 + "%d" % k, None) for k in range(100000, n_seen + 1, 100000)]
    if res["warn_record"] != UNUSED:
        events.append((res["warn_record"], -1, "Warning: bam file was not generated with fastq2bam.\n", None))
    opened = [(res["first_record"][s], order[s], s) for s in order if res["first_record"][s] != UNUSED]
    if fatal:
        opened += [(fatal.record, order[s], s) for s in res["opens_at_fatal"]]
    for k, rank, s in opened:
        events.append((k, rank, "opening %s%s.fastq.gz\n" % (opt["out"], ext[s]), s))
    files = {}
    for k, rank, text, s in sorted(events, key=lambda e: e[:2]):
        if s is not None:
            name = "%s%s.fastq.gz" % (opt["out"], ext[s])
            if not writable(name):  # fastq_open, src/fastq.c:631-660
                return 1, err + "\nERROR: Unable to open %s\n" % name, files
            files[name] = bytes(res["streams"][s])
        err += text
    if fatal:
        return fatal.status, err + "\nERROR: " + fatal.text + "\n", files
    return 0, err + "\b" * 15 + "\n" + "Alignments processed: %d\n" % res["n_alignments"], files
