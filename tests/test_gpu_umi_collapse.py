"""The census with UMI collapse (fqg_census_collapse_umis) against tests/umi_collapse_oracle.py: the whole table, the
per-cell counts and the result struct, on pairs given through Census.append so that the finish and collapse kernels run
at their own edges (a wavefront, a workgroup of 256, a scan span of 2048, a run of 64 rows), then behind real batches."""
import gzip
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from oracle import pre_barcodes_oracle as pbo
from tests import umi_collapse_oracle as uco
from tests import whitelist_rescue_oracle as wro
from tests.test_gpu_census import CASES, GOLDEN, parse
from tests.test_gpu_census_whitelist import string_pairs
from tests.test_gpu_pre_barcodes import make_10x
from tests.util import GOLD

pytestmark = pytest.mark.gpu
A = fq.abi
STATE, ARG = "libfqgpu error -5", "libfqgpu error -3"


def split(pairs):
    a = np.array(pairs, dtype=np.uint64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def collapsed(z, mm):
    """collapse_umis + both accessors on a finished census; pairs() and cells() are the bytes they were"""
    n_pairs, n_cells = z.finish()
    before = [x.tobytes() for x in z.pairs(n_pairs)] + [z.cells(n_cells).tobytes()]
    res = z.collapse_umis(mm)
    table = z.umis(res["n_umis"])
    per_cell = z.cells_collapsed(n_cells)
    assert [x.tobytes() for x in z.pairs(n_pairs)] + [z.cells(n_cells).tobytes()] == before
    lines = z.cells(n_cells)
    # per cell: as many rows as the line has distinct UMIs, and their reads are the line's reads
    if n_cells:
        starts = np.flatnonzero(np.r_[True, table["cell"][1:] != table["cell"][:-1]])
        assert (table["cell"][starts] == lines[:, 0]).all()
        assert (np.diff(np.r_[starts, len(table)]).astype(np.uint64) == lines[:, 2]).all()
        assert (np.add.reduceat(table["reads"], starts) == lines[:, 1]).all()
    return table.tolist(), per_cell.tolist(), res


def check(ctx, pairs, cell_size, umi_size, mm=1, pieces=1):
    """pairs -> append (in `pieces` calls) -> finish -> collapse; everything against the oracle.  -> the oracle's results"""
    want = uco.collapse(pairs, mm)
    z = ctx.census()
    try:
        ce, um = split(pairs)
        for k in range(pieces):
            z.append(ce[k::pieces], um[k::pieces], cell_size, umi_size)
        table, per_cell, res = collapsed(z, mm)
    finally:
        z.close()
    assert res == want[2]
    assert per_cell == want[1]
    assert table == want[0]
    return want


def test_an_empty_census():
    with fq.Context(0) as ctx:
        z = ctx.census()
        assert z.finish() == (0, 0)
        for mm in (1, 0):
            assert z.collapse_umis(mm) == {"n_umis": 0, "n_absorbed": 0, "n_roots": 0, "longest_chain": 0}
            assert len(z.umis(0)) == 0 and len(z.cells_collapsed(0)) == 0
        z.close()


def test_the_smallest_cases():
    with fq.Context(0) as ctx:
        assert check(ctx, [(7, 123)], 3, 3)[0] == [(7, 123, 1, 123)]
        assert check(ctx, [(7, 123)] * 5, 3, 3)[0] == [(7, 123, 5, 123)]
        # a chain 1 < 2 < 3 reads whose ends are two digits apart: the weakest value's root is the far end
        t, c, r = check(ctx, [(7, 111)] + [(7, 112)] * 2 + [(7, 122)] * 3, 3, 3)
        assert t[0] == (7, 111, 1, 122) and t[1] == (7, 112, 2, 122) and c == [1] and r["longest_chain"] == 2
        # two equally strong parents: the smaller value wins - found by pass A (112 < 121), by pass B (115 < 154)
        assert check(ctx, [(7, 111)] + [(7, 112)] * 2 + [(7, 121)] * 2, 3, 3)[0][0] == (7, 111, 1, 112)
        assert check(ctx, [(7, 155)] + [(7, 154)] * 2 + [(7, 115)] * 2, 3, 3)[0][2] == (7, 155, 1, 115)
        # ... and the stronger one wins over the smaller one, from either pass
        assert check(ctx, [(7, 111)] + [(7, 112)] * 2 + [(7, 121)] * 3, 3, 3)[0][0] == (7, 111, 1, 121)
        assert check(ctx, [(7, 155)] + [(7, 154)] * 3 + [(7, 115)] * 2, 3, 3)[0][2] == (7, 155, 1, 154)
        # equal reads: nobody is absorbed
        assert check(ctx, [(7, 111), (7, 112), (7, 121)] * 2, 3, 3)[2]["n_absorbed"] == 0
        # 5 and 6 digits in one cell are never neighbours; the value 0 and a value with a digit 0 are left alone
        assert check(ctx, [(7, 11111)] + [(7, 111111)] * 2 + [(7, 211111)] * 2 + [(7, 55555)] * 3, 6, 6)[2]["n_absorbed"] == 0
        t = check(ctx, [(7, 0)] + [(7, 1)] * 2 + [(7, 2)] * 3 + [(7, 101)] + [(7, 111)] * 2, 3, 3)[0]
        assert t == [(7, 0, 1, 0), (7, 1, 2, 2), (7, 2, 3, 2), (7, 101, 1, 101), (7, 111, 2, 111)]


@pytest.mark.parametrize("d", [1, 2, 3, 9, 10, 11, 19])
def test_the_differing_digit_at_every_position(d):
    """one cell per position (odd and even splits, either side of the half boundary): the weaker value is absorbed, in
    either direction of the difference, and a value two digits away is not"""
    base = int("3" * d)
    pairs = []
    for p in range(d):
        pairs += [(2 * p + 1, base)] * 2 + [(2 * p + 1, base + 10 ** p)]           # 4 at position p, one read
        pairs += [(2 * p + 2, base)] + [(2 * p + 2, base - 2 * 10 ** p)] * 2       # 1 at position p, two reads
        if d > 1:
            pairs += [(2 * p + 2, base - 2 * 10 ** p + 10 ** ((p + 1) % d))]       # two digits from base, one from the other
    with fq.Context(0) as ctx:
        want = check(ctx, pairs, 4, d)
    assert want[2]["n_absorbed"] == (3 * d if d > 1 else 2 * d)


@pytest.mark.parametrize("at", [30, 64, 256, 2047, 2048])
@pytest.mark.parametrize("weak_first", [False, True])
def test_no_absorption_across_a_cell_boundary(at, weak_first):
    """the same two neighbouring UMIs in two cells adjacent in sort order, the second cell's row at index `at` of the
    table (inside a wavefront, at its edge, at a workgroup's edge, at a scan span's edge - as a row and, one earlier, as
    a pair); in one cell the weaker one is absorbed - the control"""
    u1 = 3333333333
    n_fill = at - 1
    fill = [(c + 1, u1) for c in range(n_fill)]
    a, b = n_fill + 1, n_fill + 2
    with fq.Context(0) as ctx:
        for u2 in (3333343333, 3333433333):   # the digit in the low half (pass A), in the high half (pass B)
            two = [(a, u2), (b, u1), (b, u1)] if weak_first else [(a, u1), (a, u1), (b, u2)]
            want = check(ctx, fill + two, 5, 10)
            assert want[2]["n_absorbed"] == 0 and want[2]["n_umis"] == at + 1
            assert check(ctx, fill + [(a, u) for _, u in two], 5, 10)[2]["n_absorbed"] == 1


@pytest.mark.parametrize("rows", [63, 64, 65, 3125])
def test_runs_on_both_sides_of_the_walk_limit(rows):
    """`rows` low-half variants of one 10-digit high half (a run of pass A) and, in another cell, as many high-half
    variants of one low half (pass B); a third cell holds both, crossed"""
    rng = np.random.default_rng(rows)
    half = sorted(int("".join(s)) for s in np.array(np.meshgrid(*[list("12345")] * 5)).T.reshape(-1, 5))
    assert len(set(half)) == 3125
    pairs = []
    for k in range(rows):   # (the smallest ones: they differ in few digits, so the run is full of neighbours)
        pairs += [(1, 12345 * 10 ** 5 + half[k])] * int(rng.integers(1, 5))
        pairs += [(2, half[k] * 10 ** 5 + 54321)] * int(rng.integers(1, 5))
        pairs += [(3, 12345 * 10 ** 5 + half[k])] * int(rng.integers(1, 5)) + [(3, half[k] * 10 ** 5 + 12345)] * int(rng.integers(1, 5))
    with fq.Context(0) as ctx:
        want = check(ctx, pairs, 1, 10)
    assert want[2]["n_absorbed"] > rows // 2


def test_one_large_cell_beside_many_small_ones():
    rng = np.random.default_rng(5)
    u = np.unique((rng.integers(1, 6, (130000, 8)) * 10 ** np.arange(8)).sum(axis=1))[:100000]
    assert len(u) == 100000
    big = np.repeat(u, rng.integers(1, 4, len(u)))
    cells = np.r_[np.full(len(big), 10000), np.arange(1, 20001) + (np.arange(20000) >= 9999)]   # 10 000 cells on either side
    umis = np.r_[big, (rng.integers(1, 6, (20000, 8)) * 10 ** np.arange(8)).sum(axis=1)]
    order = rng.permutation(len(cells))
    with fq.Context(0) as ctx:
        want = check(ctx, list(zip(cells[order].tolist(), umis[order].tolist())), 5, 8, pieces=3)
    assert want[2]["n_umis"] == 120000 and want[2]["n_absorbed"] > 10000


@pytest.mark.parametrize("alphabet,d,n_cells,n_pairs", [(2, 6, 50, 20000), (3, 5, 300, 200000)])
def test_random_dense_cells(alphabet, d, n_cells, n_pairs):
    rng = np.random.default_rng(1)
    cells = rng.integers(1, n_cells + 1, n_pairs)
    umis = (rng.integers(1, alphabet + 1, (n_pairs, d)) * 10 ** np.arange(d)).sum(axis=1)
    with fq.Context(0) as ctx:
        want = check(ctx, list(zip(cells.tolist(), umis.tolist())), 3, d)
    # the rule is exercised, not idle
    assert 2 * want[2]["n_absorbed"] > want[2]["n_umis"] and want[2]["longest_chain"] >= 3


def dense_pairs():
    rng = np.random.default_rng(3)
    return list(zip(rng.integers(1, 40, 5000).tolist(), (rng.integers(1, 4, (5000, 4)) * 10 ** np.arange(4)).sum(axis=1).tolist()))


def test_max_mismatch_0_is_numpys_unique():
    pairs = dense_pairs()
    with fq.Context(0) as ctx:
        table = check(ctx, pairs, 2, 4, mm=0)[0]
    uniq, counts = np.unique(np.array(pairs, dtype=np.uint64), axis=0, return_counts=True)
    assert [(c, u, r) for c, u, r, _ in table] == [(int(c), int(u), int(r)) for (c, u), r in zip(uniq, counts)]
    assert all(u == root for _, u, _, root in table)


def test_collapse_called_again():
    pairs = dense_pairs()
    with fq.Context(0) as ctx:
        z = ctx.census()
        z.append(*split(pairs), 2, 4)
        got = [collapsed(z, mm) for mm in (1, 0, 1)]
        z.close()
    assert got[0] == got[2] == uco.collapse(pairs, 1) and got[1] == uco.collapse(pairs, 0)
    assert got[0][2]["n_absorbed"] > 0


def test_refusals():
    with fq.Context(0) as ctx:
        z = ctx.census()
        z.append(*split([(1, 11), (1, 12), (1, 12)]), 2, 2)
        with pytest.raises(A.FqgError, match=STATE):
            z.collapse_umis(1)                                   # before finish
        with pytest.raises(A.FqgError, match=ARG):
            z.append(*split([(1, 13), (1, 100)]), 2, 2)          # a value >= 10^umi_size: nothing is appended
        with pytest.raises(A.FqgError, match=ARG):
            z.append(*split([(100, 13)]), 2, 2)
        assert z.finish() == (3, 1)
        ce, um = z.pairs(3)
        assert (ce.tolist(), um.tolist()) == ([1, 1, 1], [11, 12, 12])
        for call in (lambda: z.umis(1), lambda: z.cells_collapsed(1)):
            with pytest.raises(A.FqgError, match=STATE):
                call()                                           # the accessors before a collapse
        with pytest.raises(A.FqgError, match=ARG):
            z.collapse_umis(2)
        with pytest.raises(A.FqgError, match=STATE):
            z.append(*split([(1, 13)]), 2, 2)                    # after finish
        assert z.collapse_umis(1) == {"n_umis": 2, "n_absorbed": 1, "n_roots": 1, "longest_chain": 1}
        assert z.whitelist_info() == {"exact": 0, "rescued": 0, "ambiguous": 0, "dropped": 0}
        z.close()
        # a umi_size of 20: the table, not the rule
        z = ctx.census()
        z.append(*split([(1, 11), (1, 12), (1, 12)]), 2, 20)
        z.finish()
        with pytest.raises(A.FqgError, match=ARG):
            z.collapse_umis(1)
        assert z.collapse_umis(0)["n_umis"] == 2
        z.close()


def frames_of(ctx, images):
    frames, states = {}, {}
    for x, img in images.items():
        st = A.probe_first_record(img, True)
        assert ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)["code"] == 0
        frames[x], states[x] = ctx.retain_frame(), st
    return frames, states


def test_append_behind_real_batches():
    """a barcode_test* case through transform + census, then the same pairs once more through append: every line's
    reads double, its distinct UMIs stay"""
    def fits(specs):
        return bool(specs["cell"] and specs["umi"] and 1 <= specs["umi"][2] <= 19)
    i = next(i for i in CASES if fits(parse(GOLDEN[i]["args"])[1]))
    files, specs, opt = parse(GOLDEN[i]["args"])
    images = {x: gzip.decompress(open(os.path.join(GOLD, name), "rb").read()) for x, name in files.items()}
    kw = dict(umi=specs["umi"], cell=specs["cell"], sample=specs["sample"], phred=opt["phred"], min_qual=opt["min_qual"], sam=False)
    with fq.Context(0) as ctx:
        frames, states = frames_of(ctx, images)
        n = min(f.n_records for f in frames.values())
        lines = []
        for twice in (False, True):
            z = ctx.census()
            r = ctx.barcodes_transform(frames, states, n, **kw)
            added = ctx.barcodes_census(z, frames, states, r["n_done"], **kw)
            assert added > 0
            if twice:
                ce, um = z.pairs(added)
                z.append(ce, um, specs["cell"][2], specs["umi"][2])
            n_pairs, n_cells = z.finish()
            assert n_pairs == (2 * added if twice else added)
            lines.append(z.cells(n_cells))
            pairs = list(zip(*(x.tolist() for x in z.pairs(n_pairs))))
            want = uco.collapse(pairs, 1)
            res = z.collapse_umis(1)
            assert (z.umis(res["n_umis"]).tolist(), z.cells_collapsed(n_cells).tolist(), res) == want
            z.close()
        for f in frames.values():
            f.release()
    assert (lines[1][:, 0] == lines[0][:, 0]).all() and (lines[1][:, 1] == 2 * lines[0][:, 1]).all()
    assert (lines[1][:, 2] == lines[0][:, 2]).all()


_SYN = {}


def synthetic():
    """10x-v2 pairs: 20 cells (some with one substitution: the whitelist's work) of 40 UMIs each, one substitution in
    the UMI of every tenth read or so; the names fastq_pre_barcodes gives the reads it keeps under min_qual 10"""
    if _SYN:
        return _SYN
    rng = np.random.default_rng(29)
    n = 12000
    r1, r2 = make_10x(rng, n)
    pool = [bytes(rng.choice(list(b"ACGT"), 16).astype(np.uint8)) for _ in range(20)]
    upool = [bytes(rng.choice(list(b"ACGT"), 10).astype(np.uint8)) for _ in range(40)]
    lines = r1.split(b"\n")
    planted = 0
    for k in range(n):
        if len(lines[4 * k + 1]) != 26:
            continue
        cell, umi = bytearray(pool[int(rng.integers(0, 20))]), bytearray(upool[int(rng.integers(0, 40))])
        if rng.random() < 0.05:
            p = int(rng.integers(0, 16))
            cell[p] = int(rng.choice([c for c in b"ACGT" if c != cell[p]]))
        if rng.random() < 0.10:
            p = int(rng.integers(0, 10))
            umi[p] = int(rng.choice([c for c in b"ACGTN" if c != umi[p]]))
            planted += 1
        lines[4 * k + 1] = bytes(cell) + bytes(umi)
    r1 = b"\n".join(lines)
    args = ["--read1", "r2.fastq", "--index1", "r1.fastq", "--phred_encoding", "33", "--min_qual", "10", "--outfile1", "o.fastq.gz",
            "--umi_read", "index1", "--umi_offset", "16", "--umi_size", "10", "--cell_read", "index1", "--cell_offset", "0", "--cell_size", "16"]
    files = {"r1.fastq": r1, "r2.fastq": r2}
    want = pbo.run_pre_barcodes(args, lambda name: files[name])
    assert want["exit"] == 0
    _SYN.update(r1=r1, r2=r2, pool=pool, pairs=string_pairs(want["files"][1]), n=n, planted=planted)
    return _SYN


@pytest.mark.parametrize("whitelist", [False, True])
def test_10x_synthetic_end_to_end(whitelist):
    """transform + census (+ whitelist rescue) + collapse against the oracle on the composition of the pinned oracles"""
    s = synthetic()
    kw = dict(umi=(A.INDEX1, 16, 10), cell=(A.INDEX1, 0, 16), phred=33, min_qual=10, sam=False)
    if whitelist:
        kept, info = wro.census_filter(s["pairs"], wro.members(s["pool"]), 1)
        assert info["rescued"] > 0
    else:
        kept = [(wro.pack(c), u) for c, u in s["pairs"]]
    want = uco.collapse(kept, 1)
    assert want[2]["n_absorbed"] > s["planted"] // 2 and want[2]["n_roots"] >= 20 * 40
    with fq.Context(0) as ctx:
        frames, states = frames_of(ctx, {A.READ1: s["r2"], A.INDEX1: s["r1"]})
        w = A.Whitelist.from_lines(ctx, b"".join(ln + b"\n" for ln in s["pool"])) if whitelist else None
        z = ctx.census()
        if w:
            z.set_whitelist(w, 1)
        r = ctx.barcodes_transform(frames, states, s["n"], **kw)
        assert ctx.barcodes_census(z, frames, states, r["n_done"], **kw) == len(kept)
        assert collapsed(z, 1) == want
        z.close()
        if w:
            w.close()
        for f in frames.values():
            f.release()
