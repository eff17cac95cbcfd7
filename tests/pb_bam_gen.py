"""Made-up inputs for fastq_pre_barcodes --bam: tiny FASTQ files whose SAM lines reach the corners of libbam's
sam_read1 (tests/sam2bam_oracle.py).  tools/gen_golden.py runs the reference's fastq_pre_barcodes --sam on them and
the vendored libbam on its text (tests/golden/pre_barcodes_bam.json); the tests run ours.

cases() -> {name: (files {name: bytes}, argv with --sam, comment)}; the file names are relative to the run's directory.
"""


def fq(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


def _pairs(n, seq_len=lambda i: 20 + i, name=lambda i: b"r%d" % i):
    """READ1, READ2 and an index file (8 cell + 6 UMI bases) with the same names"""
    alphabet = b"ACGTNacgtnRYKMSWBDHV=.XUu0123"
    r1, r2, ix = [], [], []
    for i in range(n):
        L = seq_len(i)
        s1 = bytes(alphabet[(7 * i + 3 * j) % len(alphabet)] for j in range(L))
        s2 = bytes(alphabet[(5 * i + 11 * j + 1) % len(alphabet)] for j in range(L + 1))
        q1 = bytes(33 + (i * 13 + j * 7) % 94 for j in range(L))
        q2 = bytes(33 + (i * 5 + j * 3) % 94 for j in range(L + 1))
        r1.append((name(i) + b" 1:N:0", s1, q1))
        r2.append((name(i) + b" 2:N:0", s2, q2))
        ix.append((name(i) + b" 1:N:0", bytes(b"ACGT"[(i + j) % 4] for j in range(14)), bytes(40 + (i + j) % 50 for j in range(14))))
    return fq(r1), fq(r2), fq(ix)


UMI = ["--umi_read", "index1", "--umi_offset", "8", "--umi_size", "6"]
CELL = ["--cell_read", "index1", "--cell_offset", "0", "--cell_size", "8"]
SAMPLE = ["--sample_read", "index1", "--sample_offset", "2", "--sample_size", "4"]


def cases():
    out = {}
    r1, r2, ix = _pairs(12)
    pe = {"r1.fastq": r1, "r2.fastq": r2, "ix.fastq": ix}
    base = ["--read1", "r1.fastq", "--read2", "r2.fastq", "--index1", "ix.fastq", "--phred_encoding", "33"]
    tail = ["--outfile1", "-", "--sam"]
    out["pairs_umi_cell_sample"] = (pe, base + UMI + CELL + SAMPLE + tail, "the blank-glued CR on the second mate, behind QX")
    out["pairs_cell_only"] = (pe, base + CELL + tail, "the blank-glued CR behind op")
    out["pairs_umi_only_10x"] = (pe, base + UMI + ["--10x"] + tail, "UB / UY")
    out["pairs_no_tags"] = (pe, base + tail, "on and op alone")
    out["pairs_sliced"] = (pe, base + UMI + CELL + ["--read1_offset", "3", "--read1_size", "9", "--read2_offset", "0", "--read2_size", "4"] + tail,
                           "slices of both mates")
    # single end: lengths 1, 2, odd, even; QUAL "*"; every quality byte; IUPAC, lower case, '=', '.', control bytes
    se = fq([(b"one", b"A", b"I"), (b"two", b"ac", b"!~"), (b"star1", b"G", b"*"), (b"star5", b"ACGTN", b"*"),
             (b"iupac with blanks 1", b"=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn.0123", bytes(range(33, 33 + 36))),
             (b"quals", b"ACGT" * 24, bytes(range(33, 127)) + b"!!"), (b"ctl", b"A\x01C\x7fG\x1fT", b"IIIIIII")])
    out["single_shapes"] = ({"r1.fastq": se}, ["--read1", "r1.fastq", "--phred_encoding", "33"] + tail, "lengths, QUAL *, the base table")
    # what libbam does not survive
    bad = {
        "refused_qual_shorter": fq([(b"a", b"ACGT", b"IIII"), (b"b", b"ACGT", b"II"), (b"c", b"AC", b"II")]),
        "refused_empty_seq": fq([(b"a", b"ACGT", b"IIII"), (b"b", b"", b""), (b"c", b"AC", b"II")]),
        "refused_empty_name": fq([(b"a", b"ACGT", b"IIII"), (b"", b"ACGT", b"IIII")]),
        "refused_tab_in_name": fq([(b"a", b"ACGT", b"IIII"), (b"b\tXY:Z:1", b"ACGT", b"IIII"), (b"c", b"AC", b"II")]),
        "refused_tab_in_seq": fq([(b"a", b"AC\tGT", b"IIIII"), (b"c", b"AC", b"II")]),
        "refused_cr_in_qual": fq([(b"a", b"ACGT", b"IIII"), (b"b", b"ACGT", b"II\rI")]),
        "refused_high_base": fq([(b"a", b"ACGT", b"IIII"), (b"b", b"AC\xe9T", b"IIII")]),
    }
    for name, img in bad.items():
        out[name] = ({"r1.fastq": img}, ["--read1", "r1.fastq", "--phred_encoding", "33"] + tail, "a line libbam aborts on, or worse")
    return out
