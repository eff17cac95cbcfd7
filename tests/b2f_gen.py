"""Seeded alignment records for the bam2fastq tests (test infrastructure, host side only): records as sh/fastq2bam
writes them (the read's original name and quality in `on` / `op`, barcodes in CR/CY, RX/QX or UB/UY, BC/QT) and records
of any other BAM, with every field bam2fastq looks at under the caller's control.  tools/gen_golden.py writes the
committed fixtures tests/golden/data_b2f/syn_*.bam with it; tests/test_gpu_bam2fastq.py builds its streams with it."""
import struct

import numpy as np

from tests import bamgen

PAIRED, UNMAP, READ1, READ2, SECONDARY = 0x1, 0x4, 0x40, 0x80, 0x100


def record(name, seq_codes=b"", qual=None, aux=b"", flag=0, l_qname=None, n_cigar=1, l_qseq=None):
    """seq_codes: one 4-bit code per base; qual: one byte per base (default 30)"""
    n = len(seq_codes)
    qn = name + b"\0"
    packed = bytearray((n + 1) // 2)
    for i, c in enumerate(seq_codes):
        packed[i >> 1] |= (c & 15) << (0 if i & 1 else 4)
    qual = bytes([30]) * n if qual is None else qual
    core = struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | (255 << 8) | (len(qn) if l_qname is None else l_qname),
                       (flag << 16) | n_cigar, n if l_qseq is None else l_qseq, -1, -1, 0)
    body = core + qn + struct.pack("<I", n << 4) * n_cigar + bytes(packed) + qual + aux
    return struct.pack("<i", len(body)) + body


def every_type():
    """one field of every aux type (A c C s S i I f d Z H B): `d` is walked the way libbam 0.1.19 walks it"""
    return (b"XAAq" + bamgen.aux_int(b"Xc", -3, b"c") + bamgen.aux_int(b"XC", 200, b"C") + bamgen.aux_int(b"Xs", -300, b"s") +
            bamgen.aux_int(b"XS", 60000, b"S") + bamgen.aux_int(b"Xi", -70000, b"i") + bamgen.aux_int(b"XI", 4000000000, b"I") +
            b"Xff" + struct.pack("<f", 1.5) + bamgen.aux_z(b"XZ", b"text") + b"XHH1AE3\0" +
            b"XBBs" + struct.pack("<i3h", 3, 1, 2, 3) + b"XbBC" + struct.pack("<i", 0))


def fastq2bam_record(rng, i, paired=False, cell=True, umi="RX", sample=False, long_read=0, name=None, extra=b""):
    """one record of a fastq2bam BAM: `on`/`op` + the barcode tags asked for"""
    n = long_read or int(rng.integers(0, 60))
    codes = bytes(rng.integers(0, 16, n, dtype=np.uint8))
    q = bytes((rng.integers(33, 74, n)).astype(np.uint8))
    on = name if name is not None else b"M%d:%d@%d:N:0:ACGT" % (i, int(rng.integers(0, 10 ** 6)), 1 + (i & 1))
    aux = extra + bamgen.aux_z(b"on", on) + bamgen.aux_z(b"op", q)
    if cell:
        c = bamgen.barcode(rng, 16)
        aux += bamgen.aux_z(b"CR", c) + bamgen.aux_z(b"CY", b"F" * 16)
    if umi:
        u = bamgen.barcode(rng, 10)
        aux += bamgen.aux_z(umi.encode(), u) + bamgen.aux_z({"RX": b"QX", "UB": b"UY"}[umi], b"E" * 10)
    if sample:
        aux += bamgen.aux_z(b"BC", bamgen.barcode(rng, 8)) + bamgen.aux_z(b"QT", b"D" * 8)
    flag = UNMAP | ((PAIRED | (READ1 if i % 2 == 0 else READ2)) if paired else 0)
    return record(b"r%d" % i, codes, None, aux, flag=flag)


def plain_record(rng, i, long_read=0):
    """a record of a BAM that fastq2bam did not write: no `on`; every routing of :284-293"""
    n = long_read or int(rng.integers(0, 60))
    codes = bytes(rng.integers(0, 16, n, dtype=np.uint8))
    q = bytes(rng.integers(0, 42, n).astype(np.uint8))
    flag = int(rng.choice([0, UNMAP, PAIRED | READ1, PAIRED | UNMAP | READ1, PAIRED | READ2 | UNMAP, PAIRED | READ2, SECONDARY, 16]))
    aux = bamgen.aux_int(b"NH", 1) if rng.random() < 0.5 else b""
    return record(b"plain%d:%d" % (i, int(rng.integers(0, 10 ** 6))), codes, q, aux, flag=flag)


def stream(recs):
    return bamgen.header(((b"chr1", 1000000),)) + b"".join(recs)


def golden_bams():
    """{file name: inflated stream} of the committed synthetic fixtures (each BAM under 100 KB)"""
    rng = np.random.default_rng(20260)
    out = {}
    f2b = lambda i, **kw: fastq2bam_record(rng, i, **kw)
    # fastq2bam records, unpaired and paired, with and without CR / RX / BC; a secondary one now and then
    recs = []
    for i in range(400):
        r = f2b(i, paired=i >= 200, cell=rng.random() < 0.7, umi="RX" if rng.random() < 0.7 else "", sample=rng.random() < 0.4)
        recs.append(r)
        if i % 37 == 5:
            recs.append(record(b"sec%d" % i, b"\1\2\4\10", None, bamgen.aux_z(b"on", b"never written"), flag=SECONDARY))
    out["syn_f2b.bam"] = stream(recs)
    # everything --10xV2 needs, every read name shape of restore_read_name, UB/UY instead of RX/QX, BC with QT
    names = [b"plain_name", b"at_last@", b"r@3:N:0@2:N:0:AC", b"a@b@c@1:N:0:TTGA", b"@1:x", b"@2:", b"x@1", b"x@12:", b"",
             b"two@2:N:0:A@1:N:0:C"]
    recs = [f2b(i, umi="UB" if i % 3 == 0 else "RX", sample=i % 4 == 1, name=names[i % len(names)] if i % 2 else None)
            for i in range(300)]
    out["syn_10x.bam"] = stream(recs)
    # a 10x file whose first fatal record is not the first record: UMI quality missing in record 57, sample quality in 40
    recs = [f2b(i) for i in range(80)]
    recs[57] = record(b"r57", b"\1\2", None, bamgen.aux_z(b"on", b"r57@1:N") + bamgen.aux_z(b"op", b"II") + bamgen.aux_z(b"CR", b"AC") +
                      bamgen.aux_z(b"CY", b"FF") + bamgen.aux_z(b"UB", b"GG"))
    out["syn_10x_fatal_umi_qual.bam"] = stream(recs)
    recs = [f2b(i) for i in range(80)]
    recs[0] = record(b"sec", b"", None, b"", flag=SECONDARY)   # (so that record 40 is the first one that opens anything but R1/R2)
    recs[40] = f2b(40, sample=True)
    recs[40] = recs[40][:recs[40].rindex(b"QTZ")]
    recs[40] = struct.pack("<i", len(recs[40]) - 4) + recs[40][4:]
    out["syn_10x_fatal_sample_qual.bam"] = stream(recs)
    # aux fields: `on` as a non-Z type, duplicate tags, every aux type in front of the wanted tags, CR as an integer
    recs = [record(b"q0", b"\1\2\4", None, bamgen.aux_int(b"on", 7, b"i") + bamgen.aux_z(b"op", b"III")),
            record(b"q1", b"\1\2\4", None, bamgen.aux_z(b"on", b"first") + bamgen.aux_z(b"on", b"second") + bamgen.aux_z(b"op", b"ABC") +
                   bamgen.aux_z(b"op", b"DEF") + bamgen.aux_z(b"CR", b"AAAA") + bamgen.aux_z(b"CR", b"CCCC")),
            record(b"q2", b"\1\2\4", None, every_type() + bamgen.aux_z(b"on", b"behind@2:all") + bamgen.aux_z(b"op", b"JJJ") +
                   bamgen.aux_z(b"CR", b"ACGT") + bamgen.aux_z(b"CY", b"FFFF") + bamgen.aux_z(b"RX", b"GG") + bamgen.aux_z(b"QX", b"EE")),
            record(b"q3", b"\1\2\4", None, bamgen.aux_z(b"on", b"q3@1:N") + bamgen.aux_int(b"op", 3) + bamgen.aux_int(b"CR", 9) +
                   bamgen.aux_int(b"CY", 9) + bamgen.aux_int(b"RX", 1, b"s") + b"QXH00FF\0" + b"BCzlower\0"),
            record(b"q4", b"\1\2\4", None, bamgen.aux_z(b"on", b"q4") + bamgen.aux_z(b"op", b"III") + b"XddCRZAAAA\0" + bamgen.aux_z(b"CR", b"TT")),
            record(b"q5", b"\1\2\4", None, bamgen.aux_z(b"on", b"") + bamgen.aux_z(b"CR", b"") + bamgen.aux_z(b"CY", b"") +
                   bamgen.aux_z(b"RX", b"") + bamgen.aux_z(b"QX", b""))]
    out["syn_aux.bam"] = stream(recs * 3)
    # read lengths around the byte and 16-byte edges and the longest the reference can hold; quality bytes that wrap
    recs = []
    for k, n in enumerate((0, 1, 2, 15, 16, 17, 9999, 31, 33)):
        codes = bytes(rng.integers(0, 16, n, dtype=np.uint8))
        q = bytearray(rng.integers(0, 94, n).astype(np.uint8))
        recs.append(record(b"len%d" % n, codes, bytes(q), b"", flag=[0, PAIRED | UNMAP, PAIRED][k % 3]))
        recs.append(fastq2bam_record(rng, 1000 + k, long_read=n) if n else f2b(1000 + k, name=b"empty read"))
    recs.append(record(b"q255", b"\1" * 6, bytes([0xFF, 10, 0xFF, 11, 0xFF, 12])))
    recs.append(record(b"q223", b"\2" * 6, bytes([40, 41, 223, 42, 43, 44])))       # 223 + 33 wraps to NUL: the line ends there
    recs.append(record(b"q223first", b"\4" * 3, bytes([223, 41, 42])))
    recs.append(record(b"name\0hidden", b"\10" * 2, bytes([1, 2])))                  # the name is a C string
    out["syn_lengths.bam"] = stream(recs)
    # records with and without `on` in one file
    recs = [f2b(i, sample=i % 5 == 0) if rng.random() < 0.5 else plain_record(rng, i) for i in range(500)]
    out["syn_mixed.bam"] = stream(recs)
    out["syn_plain.bam"] = stream([plain_record(rng, i) for i in range(600)])
    # a stream that ends inside a record: bam_read1 fails, the loop ends without a word
    whole = stream([f2b(i) for i in range(20)])
    out["syn_truncated.bam"] = whole[:-25]
    return out
