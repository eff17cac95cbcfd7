"""fqg_barcodes_transform with out_sam = FQG_OUT_BAM against sam2bam(pre_barcodes_oracle(...)): the seeded cases and the
check, shared by tests/test_gpu_pre_barcodes_bam.py (in its own process, at the default tile size) and by the runs it
starts as `python -m tests.pb_bam_cases` under another FQGPU_BC_LDS (the library reads that variable once).

No reference binary, no golden file: the expectation is made of the two Python oracles, both checked against recorded
runs of the reference and of libbam by the CPU tests.
"""
import json
import os
import sys

import numpy as np

from oracle import pre_barcodes_oracle as pbo
from tests import sam2bam_oracle as s2b

READ1, READ2, INDEX1, INDEX2, INDEX3 = 1, 2, 3, 4, 5
REF_NAME = {READ1: "read1", READ2: "read2", INDEX1: "index1", INDEX2: "index2", INDEX3: "index3"}
ALPHABET = np.frombuffer(b"ACGTNACGTNACGTNacgtnRYKMSWBDHVrykmswbdhv=.XUu0123\x01\x1f\x7f-", dtype=np.uint8)


def records(rng, n, length, tag=b"", qual_lo=33, qual_hi=127, star_every=0, alphabet=ALPHABET, name=None):
    """n FASTQ records with the names every file of a case shares; length(i) -> bases of record i"""
    out = []
    for i in range(n):
        L = int(length(i))
        s = alphabet[rng.integers(0, len(alphabet), L)].tobytes()
        q = rng.integers(qual_lo, qual_hi, L).astype(np.uint8).tobytes()
        if star_every and i % star_every == star_every - 1:
            q = b"*"   # (with L != 1 the record's SEQ and QUAL differ in length: libbam takes "*" all the same)
        nm = name(i) if name else b"M:%d:%d" % (i % 7, i)
        out.append([b"@" + nm + b" " + tag, s, b"+", q])
    return out


def image(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def case(name, recs_by_ref, umi=None, cell=None, sample=None, min_qual=0, tenx=False, slices=None, first=0, n=None):
    return {"name": name, "images": {x: image(r) for x, r in recs_by_ref.items()}, "umi": umi, "cell": cell, "sample": sample,
            "min_qual": min_qual, "tenx": tenx, "slices": slices or {}, "first": first,
            "n": n if n is not None else min(len(r) for r in recs_by_ref.values())}


def argv_of(c):
    a = []
    for x in sorted(c["images"]):
        a += ["--" + REF_NAME[x], REF_NAME[x] + ".fastq"]
    for tag in ("umi", "cell", "sample"):
        if c[tag]:
            a += ["--%s_read" % tag, REF_NAME[c[tag][0]], "--%s_offset" % tag, str(c[tag][1]), "--%s_size" % tag, str(c[tag][2])]
    for x, (off, size) in sorted(c["slices"].items()):
        a += ["--read%d_offset" % x, str(off), "--read%d_size" % x, str(size)]
    a += ["--phred_encoding", "33", "--min_qual", str(c["min_qual"])]
    if c["tenx"]:
        a += ["--10x"]
    return a + ["--outfile1", "-", "--sam"]


def barcode_lengths(i):   # an index read of 26 bases, now and then too short for its barcodes
    return 26 if i % 11 != 5 else 9


def cases():
    out = []
    rng = np.random.default_rng(20261019)
    # READ1 alone: lengths 1, 2, odd, even; the read numbers cross 9 -> 10, 99 -> 100 and 999 -> 1000 inside tiles;
    # every base class and every quality byte; QUAL "*" on reads of one base and of many
    out.append(case("se_plain", {READ1: records(rng, 1100, lambda i: 1 + i % 37, star_every=13)}))
    out.append(case("se_umi_from_the_read", {READ1: records(rng, 300, lambda i: 1 + (i * 7) % 50, qual_lo=33, qual_hi=60)},
                    umi=(READ1, 2, 5), min_qual=3, slices={READ1: (6, 100)}))
    out.append(case("se_read_numbers_beyond_32_bits", {READ1: records(rng, 40, lambda i: 30 + i)}, first=9_999_999_980,
                    umi=(READ1, 0, 4)))
    # pairs: a UMI only, a cell only (the second mate's CR glued to op), all three, none, --10x
    def pair(n, l1=lambda i: 20 + i % 31, l2=lambda i: 1 + i % 40, **kw):
        return {READ1: records(rng, n, l1, b"1:N:0", **kw), READ2: records(rng, n, l2, b"2:N:0", **kw)}
    out.append(case("pe_umi_only", pair(150), umi=(READ1, 3, 6)))
    out.append(case("pe_cell_only", pair(150), cell=(READ1, 0, 8)))
    out.append(case("pe_all_three_10x", pair(150, qual_lo=40, qual_hi=75), umi=(READ1, 8, 6), cell=(READ1, 0, 8), sample=(READ2, 0, 1),
                    tenx=True, min_qual=10))
    out.append(case("pe_none_sliced", pair(150), slices={READ1: (3, 11), READ2: (0, 200)}))
    # fitting and non-fitting tiles alternate: reads of 4 - 9 kb among short ones (k_bc_emit_direct)
    long_len = lambda i: int(4000 + (i * 977) % 5000) if i % 19 == 7 else 20 + i % 60
    out.append(case("pe_long_reads_mixed", pair(120, l1=long_len, l2=lambda i: long_len(i + 3)), umi=(READ1, 0, 8), cell=(READ2, 1, 9)))
    # READ1 + INDEX1, the 10x layout: discards (short index reads, low qualities) between kept reads, a slice of the read
    out.append(case("r1_i1_10x_layout", {READ1: records(rng, 400, lambda i: 40 + i % 90, b"2:N:0"),
                                         INDEX1: records(rng, 400, barcode_lengths, b"1:N:0", qual_lo=42, qual_hi=75,
                                                         alphabet=ALPHABET[:5])},
                    umi=(INDEX1, 16, 10), cell=(INDEX1, 0, 16), min_qual=10, slices={READ1: (5, 30)}))
    out.append(case("r1_r2_i1", {READ1: records(rng, 200, lambda i: 25 + i % 17, b"1:N:0"), READ2: records(rng, 200, lambda i: 2 + i % 29, b"2:N:0"),
                                 INDEX1: records(rng, 200, barcode_lengths, b"1:N:0", alphabet=ALPHABET[:5])},
                    umi=(INDEX1, 8, 6), cell=(INDEX1, 0, 8), sample=(INDEX1, 14, 4)))
    five = {x: records(rng, 200, (lambda i: 30 + i % 23) if x <= READ2 else barcode_lengths, b"2:N:0" if x == READ2 else b"1:N:0", alphabet=ALPHABET if x <= READ2 else ALPHABET[:5])
            for x in (READ1, READ2, INDEX1, INDEX2, INDEX3)}
    out.append(case("five_files", five, umi=(INDEX2, 0, 10), cell=(INDEX3, 4, 12), sample=(INDEX1, 1, 7), tenx=True))
    # a NUL byte inside lines: they are C strings - the sequence and the quality end at theirs, the name too
    nul = records(rng, 90, lambda i: 30 + i % 9, alphabet=ALPHABET[:5])
    nul[20][1] = nul[20][1][:11] + b"\0" + nul[20][1][12:]
    nul[20][3] = nul[20][3][:11] + b"\0" + nul[20][3][12:]
    nul[21][0] = nul[21][0][:4] + b"\0" + nul[21][0][5:]
    out.append(case("se_nul_bytes", {READ1: nul}, umi=(READ1, 0, 4)))

    # ---- refused: the first such record ends the batch ----
    def refused(name, mutate, paired=False, at=57, n=100, **kw):
        r = {READ1: records(rng, n, lambda i: 20 + i % 30, b"1:N:0", alphabet=ALPHABET[:5])}
        if paired:
            r[READ2] = records(rng, n, lambda i: 10 + i % 30, b"2:N:0", alphabet=ALPHABET[:5])
        mutate(r, at)
        c = case(name, r, **kw)
        c["refused_at"] = at
        return c

    def set_line(x, line, f):
        def m(r, at):
            r[x][at][line] = f(r[x][at][line])
        return m
    out.append(refused("refused_qual_shorter", set_line(READ1, 3, lambda q: q[:-3])))
    out.append(refused("refused_qual_one_char_not_star", set_line(READ1, 3, lambda q: b"I")))
    out.append(refused("refused_empty_seq_and_qual", lambda r, at: r[READ1][at].__setitem__(slice(1, 4), [b"", b"+", b""])))
    out.append(refused("refused_seq_star", lambda r, at: r[READ1][at].__setitem__(slice(1, 4), [b"*", b"+", b"*"])))
    out.append(refused("refused_tab_in_header", set_line(READ1, 0, lambda h: h[:3] + b"\t" + h[3:])))
    out.append(refused("refused_vt_in_seq", set_line(READ1, 1, lambda s: s[:5] + b"\x0b" + s[6:])))
    out.append(refused("refused_cr_in_qual", set_line(READ1, 3, lambda q: q[:2] + b"\r" + q[3:])))
    out.append(refused("refused_ff_in_umi", set_line(READ1, 1, lambda s: s[:1] + b"\x0c" + s[2:]), umi=(READ1, 0, 4), at=3))
    out.append(refused("refused_high_base", set_line(READ1, 1, lambda s: s[:-1] + b"\xe9")))
    out.append(refused("refused_in_the_second_mate", set_line(READ2, 3, lambda q: q + b"II"), paired=True, cell=(READ1, 0, 4)))
    out.append(refused("refused_tab_in_second_mate_at_0", set_line(READ2, 3, lambda q: q[:2] + b"\t" + q[3:]), paired=True, at=0))
    out.append(refused("refused_nul_cuts_the_quality", set_line(READ1, 3, lambda q: q[:9] + b"\0" + q[10:]), at=50))

    # a quality line of the barcode file that ends in front of the barcode's range: an empty QX value; one that ends
    # inside it: the line's '\n' is part of the value (the SAM text breaks there; the batch ends in front of that read)
    def index_quality(cut):
        def m(r, at):
            r[INDEX1] = records(rng, len(r[READ1]), lambda i: 26, b"1:N:0", alphabet=ALPHABET[:5])
            r[INDEX1][at][3] = r[INDEX1][at][3][:cut]
        return m
    out.append(refused("refused_empty_umi_quality", index_quality(10), umi=(INDEX1, 16, 10), at=64))
    out.append(refused("refused_newline_in_umi_quality", index_quality(20), umi=(INDEX1, 16, 10), at=33))
    out.append(refused("refused_in_a_long_read", lambda r, at: (r[READ1][at].__setitem__(1, b"ACGT" * 1500 + b"\tA"),
                                                                  r[READ1][at].__setitem__(3, b"I" * 6002)), at=40))
    # ... and a read that is discarded is no line at all: nothing is refused
    c = refused("discarded_not_refused", set_line(READ1, 0, lambda h: h[:3] + b"\t" + h[3:]), umi=(READ1, 100, 4))
    del c["refused_at"]
    out.append(c)
    return out


def expected(c):
    """-> (record bytes, finding or None): finding = (iteration, mate)"""
    files = {REF_NAME[x] + ".fastq": img for x, img in c["images"].items()}
    want = pbo.run_pre_barcodes(argv_of(c), lambda n: files[n])
    assert want["exit"] == 0, want["stderr"]
    lines = want["stdout"].encode("latin-1").split(b"\n")[2:]
    if c["first"]:   # the oracle counts from 1: the batch's reads are numbered from first + 1
        lines = [(b"%d" % (int(ln.split(b"\t", 1)[0]) + c["first"])) + b"\t" + ln.split(b"\t", 1)[1] if ln else ln for ln in lines]
    r = s2b.sam2bam(b"\n".join(lines))
    if r["refused"] is None:
        return b"".join(r["records"]), None
    at = r["refused"][0] - 1
    while not lines[at].split(b"\t")[0].isdigit():   # (a line break inside a value: the piece belongs to the line in front)
        at -= 1
    bad = lines[at].split(b"\t")
    number, mate = int(bad[0]), 2 if bad[1] == b"141" else 1
    # (the batch ends in front of the ITERATION: a first mate's record in front of a refused second mate is not kept)
    front = [rec for rec, ln in zip(r["records"], lines) if int(ln.split(b"\t", 1)[0]) < number]
    return b"".join(front), (number - 1 - c["first"], mate)


def run_case(ctx, A, c):
    """-> (record bytes, finding or None, result dict) from the library"""
    frames, states = {}, {}
    try:
        for x, img in c["images"].items():
            st = A.probe_first_record(img, True)
            r = ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)
            assert r["code"] == 0, (c["name"], x, r)
            frames[x], states[x] = ctx.retain_frame(), st
        r = ctx.barcodes_transform(frames, states, c["n"], umi=c["umi"], cell=c["cell"], sample=c["sample"], phred=33,
                                   min_qual=c["min_qual"], sam=A.OUT_BAM, tenx=c["tenx"], first_read_number=c["first"], slices=c["slices"])
        data = ctx.barcodes_output(0, r["out_bytes"][0])
        return data, ((r["iteration"], r["file"]) if r["code"] else None), r
    finally:
        for f in frames.values():
            f.release()


def check_case(ctx, A, c):
    """'' or what is wrong"""
    want, want_finding = expected(c)
    got, finding, r = run_case(ctx, A, c)
    if "refused_at" in c and (want_finding is None or want_finding[0] != c["refused_at"]):
        return "%s: the oracles do not refuse record %d: %r" % (c["name"], c["refused_at"], want_finding)
    if (finding is None) != (want_finding is None) or (finding and (r["code"] != A.E_BAM_RECORD or finding != want_finding)):
        return "%s: finding %r (code %d), expected %r" % (c["name"], finding, r["code"], want_finding)
    if finding and r["n_done"] != want_finding[0]:
        return "%s: n_done %d" % (c["name"], r["n_done"])
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        return "%s: %d bytes against %d expected, first difference at byte %d" % (c["name"], len(got), len(want), at)
    again, _, _ = run_case(ctx, A, c)
    if again != got:
        return "%s: the same transform twice gave other bytes" % c["name"]
    return ""


def main():
    import fastq_utils_amd as fq
    from fastq_utils_amd import abi as A
    bad = []
    with fq.Context(0) as ctx:
        for c in cases():
            msg = check_case(ctx, A, c)
            if msg:
                bad.append(msg)
    print(json.dumps({"lds": os.environ.get("FQGPU_BC_LDS"), "cases": len(cases()), "failed": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
