"""The census with a whitelist attached (fqg_census_set_whitelist): what it keeps must be what a plain census keeps,
filtered and rewritten afterwards by tests/whitelist_rescue_oracle.py - exact (bam_umi_count --known_cells: valid_barcode,
src/bam_umi_count.c:523-535), then with the one-mismatch rescue.  The inputs are those of tests/test_gpu_census.py: the
barcode_test* files with the names the reference binary wrote, and synthetic 10x-v2 pairs under min_qual, so that the
census's own skip rules (reads the transform dropped, reads without a UMI) run in front of the look-up."""
import gzip
import os
from collections import defaultdict

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import bam_tags_oracle as bto
from oracle import pre_barcodes_oracle as pbo
from oracle import umi_oracle as uo
from tests import whitelist_rescue_oracle as wro
from tests.test_gpu_census import CASES, GOLDEN, parse
from tests.test_gpu_pre_barcodes import make_10x
from tests.util import GOLD

pytestmark = pytest.mark.gpu
A = fq.abi


def string_pairs(fastq_text: bytes):
    """names of the reads fastq_pre_barcodes kept -> (cell value, packed UMI) of the reads bam_umi_count would count"""
    pairs = []
    for line in fastq_text.split(b"\n"):
        if not line.startswith(b"@STAGS_"):
            continue
        qname = line[1:].split(b" ")[0].split(b"\t")[0] + b"\0"
        ok, cell, umi, _sample = bto.get_barcodes(qname, 0, len(qname))
        if not ok or not umi:
            continue
        pairs.append((bytes(cell), uo.char2uint_64(umi)))
    return pairs


def lines_of(pairs):
    per_cell = defaultdict(lambda: [0, set()])
    for c, u in pairs:
        per_cell[c][0] += 1
        per_cell[c][1].add(u)
    return sorted((c, v[0], len(v[1])) for c, v in per_cell.items())


def run(ctx, images, specs, opt, attach=None):
    """transform + census.  attach: called with the fresh census before the first batch.
    -> n_added, sorted pairs, per-cell lines, whitelist_info, the arrays as the device holds them, the transform's result"""
    frames, states = {}, {}
    for x, img in images.items():
        st = A.probe_first_record(img, True)
        r = ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)
        assert r["code"] == 0
        frames[x], states[x] = ctx.retain_frame(), st
    n = min(f.n_records for f in frames.values())
    z = ctx.census()
    try:
        if attach:
            attach(z)
        kw = dict(umi=specs["umi"], cell=specs["cell"], sample=specs["sample"], phred=opt["phred"], min_qual=opt["min_qual"], sam=False)
        r = ctx.barcodes_transform(frames, states, n, **kw)
        assert r["code"] == 0
        added = ctx.barcodes_census(z, frames, states, r["n_done"], **kw)
        info = z.whitelist_info()
        n_pairs, n_cells = z.finish()
        assert n_pairs == added
        ce, um = z.pairs(n_pairs)
        cells = z.cells(n_cells)
        return added, list(zip(ce.tolist(), um.tolist())), [tuple(int(v) for v in row) for row in cells], info, r
    finally:
        z.close()
        for f in frames.values():
            f.release()


def compare(ctx, images, specs, opt, pairs, lines, want_rescued=False):
    """pairs: string_pairs of what the reference keeps; lines: the whitelist file's lines"""
    W = wro.members(lines)
    plain = run(ctx, images, specs, opt)
    assert plain[1] == sorted((wro.pack(c), u) for c, u in pairs)   # the census under test sees what the oracle sees
    assert plain[3] == {"exact": 0, "rescued": 0, "ambiguous": 0, "dropped": 0}
    w = A.Whitelist.from_lines(ctx, b"".join(ln + b"\n" for ln in lines))
    try:
        for mm in (0, 1):
            kept, info = wro.census_filter(pairs, W, mm)
            added, got_pairs, got_lines, got_info, _ = run(ctx, images, specs, opt, attach=lambda z: z.set_whitelist(w, mm))
            assert got_pairs == sorted(kept), mm
            assert got_lines == lines_of(kept), mm
            assert added == len(kept) and got_info == info, (mm, got_info, info)
            if mm == 0:
                assert info["rescued"] == info["ambiguous"] == 0
            elif want_rescued:
                assert info["rescued"] > 0 and info["ambiguous"] > 0 and info["dropped"] > info["ambiguous"] and info["exact"] > 0
        # attached and detached again: the census that never saw a whitelist, bit for bit
        def on_off(z):
            z.set_whitelist(w, 1)
            z.set_whitelist(None)
        again = run(ctx, images, specs, opt, attach=on_off)
        assert again[:4] == plain[:4]
    finally:
        w.close()


# umi only (every cell is 0), a cell of 8 from the same file under min_qual 10 and 1, cell and sample from other files
GOLDEN_CASES = [i for i in CASES if i in (2, 3, 4, 5)]


@pytest.mark.parametrize("i", GOLDEN_CASES)
def test_reference_output_names_under_a_whitelist(i):
    case = GOLDEN[i]
    files, specs, opt = parse(case["args"])
    images = {x: gzip.decompress(open(os.path.join(GOLD, name), "rb").read()) for x, name in files.items()}
    pairs = string_pairs(case["files"]["OUT1"].encode("latin-1"))
    cells = sorted({c for c, _ in pairs})
    # every other cell of the file is known, the others lie one substitution beside a known one (rescued to a cell the
    # file does not hold); without a cell barcode every read is cell 0, kept iff 0 is in W
    beside = [(b"C" if c[:1] in b"Aa" else b"A") + c[1:] for c in cells[1::2] if c]
    lines = cells[::2] + beside if specs["cell"] else [b"ACGT", b""]
    with fq.Context(0) as ctx:
        compare(ctx, images, specs, opt, pairs, lines)
        if not specs["cell"]:   # ... and dropped when it is not: nothing is one substitution away from no barcode
            w0 = A.Whitelist.from_lines(ctx, b"ACGT\n")
            added, got_pairs, _, info, _ = run(ctx, images, specs, opt, attach=lambda z: z.set_whitelist(w0, 1))
            assert added == 0 and got_pairs == [] and info == {"exact": 0, "rescued": 0, "ambiguous": 0, "dropped": len(pairs)}
            w0.close()


def test_golden_cases_cover_the_layouts():
    assert len(GOLDEN_CASES) == 4


_SYN = {}


def synthetic():
    """10x-v2 pairs whose cells are members of a pool, members with one substitution (some of them between two members),
    members in lower case, and noise; the names fastq_pre_barcodes gives the reads it keeps under min_qual 10"""
    if _SYN:
        return _SYN
    rng = np.random.default_rng(23)
    n = 12000
    r1, r2 = make_10x(rng, n)
    bases = list(b"ACGT")
    pool = [bytes(rng.choice(bases, 16).astype(np.uint8)) for _ in range(60)]
    for k in range(0, 20, 2):   # pairs of members two substitutions apart: the reads between them are ambiguous
        b = bytearray(pool[k])
        b[3], b[9] = (b"ACGT"[(b"ACGT".index(b[3]) + 1) % 4], b"ACGT"[(b"ACGT".index(b[9]) + 1) % 4])
        pool[k + 1] = bytes(b)
    upool = [bytes(rng.choice(list(b"ACGTN"), 10).astype(np.uint8)) for _ in range(300)]
    lines = r1.split(b"\n")
    for k in range(n):
        s = lines[4 * k + 1]
        if len(s) != 26:
            continue
        kind = int(rng.integers(0, 10))
        j = int(rng.integers(0, 60))
        cell = bytearray(pool[j])
        if kind == 5:                       # one substitution anywhere
            p = int(rng.integers(0, 16))
            cell[p] = int(rng.choice([c for c in b"ACGTN" if c != cell[p]]))
        elif kind == 6 and j < 20:          # between the two members of a pair
            cell[3] = (pool[j ^ 1])[3]
        elif kind == 7:
            cell = bytearray(bytes(cell).lower())
        elif kind == 8:
            cell = bytearray(s[:16])        # noise
        elif kind == 9:
            cell[int(rng.integers(0, 16))] = ord("N")
        lines[4 * k + 1] = bytes(cell) + (upool[int(rng.integers(0, 300))] if k % 3 else s[16:])
    r1 = b"\n".join(lines)
    specs = {"umi": (A.INDEX1, 16, 10), "cell": (A.INDEX1, 0, 16), "sample": None}
    args = ["--read1", "r2.fastq", "--index1", "r1.fastq", "--phred_encoding", "33", "--min_qual", "10", "--outfile1", "o.fastq.gz",
            "--umi_read", "index1", "--umi_offset", "16", "--umi_size", "10", "--cell_read", "index1", "--cell_offset", "0", "--cell_size", "16"]
    files = {"r1.fastq": r1, "r2.fastq": r2}
    want = pbo.run_pre_barcodes(args, lambda name: files[name])
    assert want["exit"] == 0
    _SYN.update(r1=r1, r2=r2, specs=specs, pool=pool, pairs=string_pairs(want["files"][1]), n=n)
    return _SYN


def test_10x_synthetic_exact_then_rescue():
    s = synthetic()
    with fq.Context(0) as ctx:
        images = {A.READ1: s["r2"], A.INDEX1: s["r1"]}
        opt = {"phred": 33, "min_qual": 10}
        # the transform keeps fewer reads than it saw: the census's own rules run in front of the look-up
        assert len(s["pairs"]) < s["n"]
        compare(ctx, images, s["specs"], opt, s["pairs"], s["pool"][:50] + [s["pool"][0], b""], want_rescued=True)
        r = run(ctx, images, s["specs"], opt)[4]
        assert r["n_discarded"] > 0


@pytest.mark.parametrize("n", [1, 64, 65])
def test_a_cell_value_in_the_last_bytes_of_the_image(n):
    """One file, the UMI its first base and the cell its second.  The last record is `@r\\nCA\\n+\\nII\\n`: 7 bytes lie
    between its cell value and the image's end, so census_fetch leaves it to the byte-wise packer - plain, under a
    whitelist that holds it, and under one that holds its neighbour `C` only (rescued)."""
    rng = np.random.default_rng(n)
    recs = []
    for i in range(n - 1):
        s = bytes(rng.choice(list(b"ACGTNacgt"), int(rng.integers(1, 9))).astype(np.uint8))   # (one base: too short, discarded)
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    img = b"".join(recs) + b"@r\nCA\n+\nII\n"
    specs = {"umi": (A.READ1, 0, 1), "cell": (A.READ1, 1, 1), "sample": None}
    args = ["--read1", "r.fastq", "--phred_encoding", "33", "--min_qual", "10", "--outfile1", "o.fastq.gz", "--umi_read", "read1",
            "--umi_offset", "0", "--umi_size", "1", "--cell_read", "read1", "--cell_offset", "1", "--cell_size", "1"]
    want = pbo.run_pre_barcodes(args, lambda name: img)
    assert want["exit"] == 0
    pairs = string_pairs(want["files"][1])
    assert pairs[-1] == (b"A", wro.pack(b"C"))
    with fq.Context(0) as ctx:
        for lines in ([b"A"], [b"C"]):
            compare(ctx, {A.READ1: img}, specs, {"phred": 33, "min_qual": 10}, pairs, lines)
            kept, info = wro.census_filter(pairs[-1:], wro.members(lines), 1)
            assert kept == [(wro.pack(lines[0]), wro.pack(b"C"))] and info["rescued"] == (lines == [b"C"])


def frames_of(ctx, s):
    frames, states = {}, {}
    for x, img in ((A.READ1, s["r2"]), (A.INDEX1, s["r1"])):
        st = A.probe_first_record(img, True)
        ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)
        frames[x], states[x] = ctx.retain_frame(), st
    return frames, states


KW_10X = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), min_qual=10, sam=False)


def test_a_whitelist_call_without_its_bytes_leaves_the_census_its_status_bytes():
    s = synthetic()
    with fq.Context(0) as ctx:
        frames, states = frames_of(ctx, s)
        w = A.Whitelist.from_lines(ctx, b"\n".join(s["pool"]) + b"\n")
        z = ctx.census()
        r = ctx.barcodes_transform(frames, states, s["n"], **KW_10X)
        assert ctx.barcodes_whitelist(frames[A.INDEX1], w, 0, 16)["n_valid"] > 0
        assert ctx.barcodes_whitelist_correct(frames[A.INDEX1], w, 0, 16, 1, want_cells=True)["n_rescued"] > 0
        added = ctx.barcodes_census(z, frames, states, r["n_done"], **KW_10X)
        n_pairs, _ = z.finish()
        ce, um = z.pairs(n_pairs)
        assert added == n_pairs and list(zip(ce.tolist(), um.tolist())) == sorted((wro.pack(c), u) for c, u in s["pairs"])
        z.close()
        w.close()
        for f in frames.values():
            f.release()


@pytest.mark.parametrize("call", ["whitelist", "whitelist_correct"])
def test_a_whitelist_call_that_writes_its_bytes_ends_the_transform_for_the_census(call):
    """Both calls write their per-record bytes where the transform wrote its status bytes: a census behind them would
    read 0 / 1 validity as keep / discard.  It is refused instead (FQG_ERR_STATE) until the next transform."""
    s = synthetic()
    with fq.Context(0) as ctx:
        frames, states = frames_of(ctx, s)
        w = A.Whitelist.from_lines(ctx, b"\n".join(s["pool"]) + b"\n")
        z = ctx.census()
        r = ctx.barcodes_transform(frames, states, s["n"], **KW_10X)
        if call == "whitelist":
            ctx.barcodes_whitelist(frames[A.INDEX1], w, 0, 16, want_flags=True)
        else:
            ctx.barcodes_whitelist_correct(frames[A.INDEX1], w, 0, 16, 1, want_status=True)
        with pytest.raises(A.FqgError):
            ctx.barcodes_census(z, frames, states, r["n_done"], **KW_10X)
        r = ctx.barcodes_transform(frames, states, s["n"], **KW_10X)
        assert ctx.barcodes_census(z, frames, states, r["n_done"], **KW_10X) == len(s["pairs"])
        z.close()
        w.close()
        for f in frames.values():
            f.release()


def test_set_whitelist_is_refused_where_it_cannot_hold():
    s = synthetic()
    with fq.Context(0) as ctx:
        frames, states = {}, {}
        for x, img in ((A.READ1, s["r2"]), (A.INDEX1, s["r1"])):
            st = A.probe_first_record(img, True)
            ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)
            frames[x], states[x] = ctx.retain_frame(), st
        w = A.Whitelist.from_lines(ctx, b"\n".join(s["pool"]) + b"\n")
        z = ctx.census()
        kw = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), min_qual=10, sam=False)
        with pytest.raises(A.FqgError):
            z.set_whitelist(w, 2)                      # 0 or 1
        # a cell of 20 characters: fine for the exact look-up, refused with max_mismatch 1 by the next census call
        long_cell = dict(kw, cell=(A.READ1, 0, 20))
        r = ctx.barcodes_transform(frames, states, 2000, **long_cell)
        z.set_whitelist(w, 1)
        with pytest.raises(A.FqgError):
            ctx.barcodes_census(z, frames, states, r["n_done"], **long_cell)
        z.set_whitelist(w, 0)
        assert ctx.barcodes_census(z, frames, states, r["n_done"], **long_cell) == 0   # (20 bases of cDNA: no member)
        z.set_whitelist(w, 1)                          # still empty: allowed
        r = ctx.barcodes_transform(frames, states, 2000, **kw)
        assert ctx.barcodes_census(z, frames, states, r["n_done"], **kw) > 0
        with pytest.raises(A.FqgError):
            z.set_whitelist(None)                      # the census holds pairs
        with pytest.raises(A.FqgError):
            z.set_whitelist(w, 0)
        info = z.whitelist_info()
        assert info["exact"] > 0 and info["dropped"] >= info["ambiguous"]
        z.close()
        w.close()
        for f in frames.values():
            f.release()
