"""The walk of k_bc_emit_tile (its own loop: the order of tile_walk, fastq_utils_amd/csrc/fqg_fastq_tile.h, written out in
fqg_barcode_kernels.hip, and without spans in flight for any set of files) over more tiles than wavefronts:
fqg_barcodes_transform as FASTQ text and as SAM lines against oracle/pre_barcodes_oracle.py, run as
`python -m tests.pb_walk_cases` by tests/test_gpu_pre_barcodes_walk.py with FQGPU_BC_LDS=4096 (small tiles),
FQGPU_TILE_WAVES=1, 2 or 3 (the grid) and FQGPU_BC_DEBUG=1 - the library reads the first two once, and the line it then
prints per transform says what was walked: T, the emit kernel's grid, the tiles that took the record-by-record kernel.

Per kind and set of files one frame of R records; the cases differ in the number of iterations, in where they start
and in where READ1's long record (6000 bases: more than the whole LDS budget) lies.  A long record changes places with
another record's sequence and quality lines, so every arrangement is a frame of the same bytes and the same T.
"""
import json
import os
import sys
import tempfile

import numpy as np

from oracle import pre_barcodes_oracle as pbo
from tests.pb_bam_cases import ALPHABET, INDEX1, INDEX2, READ1, READ2, REF_NAME, image

R = 460          # records of every frame: seven tiles of 64 and the start of the case that does not begin at record 0
LONG = 6000      # bases of a long record
FILE_SETS = {
    "r1": dict(files=(READ1,), umi=(READ1, 0, 6)),
    "r1_r2": dict(files=(READ1, READ2), cell=(READ1, 0, 8)),                          # a SAM lane pair shares a tile
    "r1_i1": dict(files=(READ1, INDEX1), umi=(INDEX1, 16, 10), cell=(INDEX1, 0, 16)),
    "r1_i2": dict(files=(READ1, INDEX2), umi=(INDEX2, 0, 10)),                        # no kernel of its own: MASK 0
}


def base_records(rng, x, n_long):
    """the records of file x; READ1's first n_long records are the long ones"""
    out = []
    for i in range(R):
        if x in (INDEX1, INDEX2):
            L = 26 if i % 11 != 5 else 9   # now and then too short for its barcodes: a discarded iteration
        else:
            L = 30 + (i * 7) % 31          # 30..60, and every run of a few records close to the mean
        if x == READ1 and i < n_long:
            L = LONG
        s = ALPHABET[:5][rng.integers(0, 5, L)].tobytes()
        q = rng.integers(40, 75, L).astype(np.uint8).tobytes()
        out.append([b"@W:%d:%d " % (i % 7, i) + (b"2:N:0" if x == READ2 else b"1:N:0"), s, b"+", q])
    return out


def arranged(recs, long_at):
    """READ1's long records (at 0, 1, ..) change sequence and quality lines with the records at long_at"""
    r1 = [list(r) for r in recs[READ1]]
    for j, p in enumerate(long_at):
        r1[j][1], r1[p][1] = r1[p][1], r1[j][1]
        r1[j][3], r1[p][3] = r1[p][3], r1[j][3]
    out = dict(recs)
    out[READ1] = r1
    return out


def expected(kind, fs, recs, first, n):
    files = {REF_NAME[x] + ".fastq": image(recs[x][first:first + n]) for x in fs["files"]}
    argv = []
    for x in fs["files"]:
        argv += ["--" + REF_NAME[x], REF_NAME[x] + ".fastq"]
    for tag in ("umi", "cell"):
        if fs.get(tag):
            argv += ["--%s_read" % tag, REF_NAME[fs[tag][0]], "--%s_offset" % tag, str(fs[tag][1]), "--%s_size" % tag, str(fs[tag][2])]
    argv += ["--phred_encoding", "33"]
    if kind == "sam":
        want = pbo.run_pre_barcodes(argv + ["--outfile1", "-", "--sam"], lambda name: files[name])
        assert want["exit"] == 0, want["stderr"]
        return {0: want["stdout"].encode("latin-1").split(b"\n", 2)[2]}
    want = pbo.run_pre_barcodes(argv + ["--outfile1", "o1"] + (["--outfile2", "o2"] if READ2 in fs["files"] else []), lambda name: files[name])
    assert want["exit"] == 0, want["stderr"]
    return dict(want["files"])


def with_debug_line(fn):
    """fn() with the library's stderr in a file -> (fn(), the fields of the line bc_emit printed)"""
    import re
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as t:
        os.dup2(t.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        t.seek(0)
        text = t.read().decode("latin-1")
    m = re.findall(r"fqgpu barcodes: T=(\d+) in_cap=\d+ out_cap=\d+ emit grid=(\d+) \(\d+/CU\) big tiles=(\d+)", text)
    assert len(m) == 1, text
    return r, dict(zip(("T", "grid", "big"), map(int, m[0])))


class Frames:
    """the retained frames of one arrangement"""

    def __init__(self, ctx, A, fs, recs):
        self.ctx, self.A, self.fs, self.frames, self.states = ctx, A, fs, {}, {}
        for x in fs["files"]:
            img = image(recs[x])
            st = A.probe_first_record(img, True)
            r = ctx.validate(img, None, st, final=True, flags=A.VALIDATE_FRAME_ONLY)
            assert r["code"] == 0, (x, r)
            self.frames[x], self.states[x] = ctx.retain_frame(), st

    def transform(self, kind, first, n):
        """-> ({output: bytes}, the debug line)"""
        import ctypes as C
        ctx, A, fs = self.ctx, self.A, self.fs
        p, fr, stt, first_rec = ctx._barcode_args(self.frames, self.states, fs.get("umi"), fs.get("cell"), None, 33, 0,
                                                  A.OUT_SAM if kind == "sam" else False, False)
        for x in fs["files"]:
            first_rec[x] = first
        r = A.BarcodeResult()
        _, dbg = with_debug_line(lambda: ctx._check(A.load().fqg_barcodes_transform(ctx.h, fr, stt, first_rec, C.byref(p), n, 0, C.byref(r))))
        assert r.code == 0 and r.n_done == n, (r.code, r.n_done)
        return {i: ctx.barcodes_output(i, r.out_bytes[i]) for i in range(3) if r.out_bytes[i]}, dbg

    def release(self):
        for f in self.frames.values():
            f.release()


def run_group(ctx, A, kind, name, waves, bad):
    """every case of one kind and set of files; what is wrong goes to `bad`"""
    fs = FILE_SETS[name]
    rng = np.random.default_rng(sum(name.encode()) * 2 + (kind == "sam"))
    n_cases = 0

    def check(label, F, recs, first, n, T, want_big):
        nonlocal n_cases
        n_cases += 1
        got, dbg = F.transform(kind, first, n)
        tiles = (n + T - 1) // T
        where = "%s %s %s (first %d, %d iterations, %d tiles): " % (kind, name, label, first, n, tiles)
        if dbg["T"] != T or dbg["grid"] != min(waves, tiles):
            bad.append(where + "the walk was %r" % dbg)
        if not want_big(dbg["big"], tiles):
            bad.append(where + "big tiles %d" % dbg["big"])
        want = {k: v for k, v in expected(kind, fs, recs, first, n).items() if v}
        if got != want:
            bad.append(where + "outputs %r of %r bytes against %r expected" % (sorted(got), [len(v) for v in got.values()], [len(v) for v in want.values()]))

    none_big = lambda big, tiles: big == 0
    some_big = lambda big, tiles: 0 < big < tiles
    # ---- no long record: 1, 2, 3, 4 and 7 tiles, the last one holding one iteration and holding T ----
    recs = {x: base_records(rng, x, 0) for x in fs["files"]}
    F = Frames(ctx, A, fs, recs)
    try:
        _, dbg = F.transform(kind, 0, R)
        T = dbg["T"]
        assert 1 <= T and 7 * T <= R - 5, dbg
        counts = [T * (m - 1) + 1 for m in (1, 2, 3, 4, 7)] + [T * m for m in (1, 2, 3, 4, 7)]
        for n in sorted(set(counts)):
            check("plain", F, recs, 0, n, T, none_big)           # record 0 in lane 0
        check("not from record 0", F, recs, 5, 3 * T + 1, T, none_big)   # no lane holds record 0
    finally:
        F.release()
    # ---- one long record in the first, a middle and the last tile ----
    recs = {x: base_records(rng, x, 1) for x in fs["files"]}
    F = Frames(ctx, A, fs, recs)
    try:
        _, dbg = F.transform(kind, 0, R)
        T = dbg["T"]
        assert 1 <= T and 7 * T <= R - 5 and dbg["big"] >= 1, dbg
    finally:
        F.release()
    for n in sorted(set(c for c in [T * (m - 1) + 1 for m in (2, 3, 4, 7)] + [T * m for m in (2, 3, 4, 7)] if c > T)):
        tiles = (n + T - 1) // T
        for tile in sorted({0, tiles // 2, tiles - 1}):
            at = min(tile * T + T // 2, n - 1)
            arr = arranged(recs, [at])
            F = Frames(ctx, A, fs, arr)
            try:
                check("long record in tile %d" % tile, F, arr, 0, n, T, some_big)
                if n == 3 * T + 1 and tile == tiles // 2:
                    check("long record, not from record 0", F, arr, 1, n - 1, T, some_big)
            finally:
                F.release()
    # ---- two long records in two tiles that one wavefront walks one after the other ----
    recs = {x: base_records(rng, x, 2) for x in fs["files"]}
    F = Frames(ctx, A, fs, recs)
    try:
        _, dbg = F.transform(kind, 0, R)
        T = dbg["T"]
        assert 1 <= T and 7 * T <= R - 5 and dbg["big"] >= 1, dbg
    finally:
        F.release()
    arr = arranged(recs, [2 + T, 2 + T + min(waves, 7) * T])   # tile 1 and the tile a stride behind it
    F = Frames(ctx, A, fs, arr)
    try:
        check("two long records a stride apart", F, arr, 0, 7 * T, T, lambda big, tiles: big == 2)
    finally:
        F.release()
    return n_cases


def main():
    import fastq_utils_amd as fq
    from fastq_utils_amd import abi as A
    waves = int(os.environ["FQGPU_TILE_WAVES"])
    assert os.environ.get("FQGPU_BC_LDS") == "4096" and os.environ.get("FQGPU_BC_DEBUG")
    bad, n_cases = [], 0
    with fq.Context(0) as ctx:
        for kind in ("fastq", "sam"):
            for name in FILE_SETS:
                n_cases += run_group(ctx, A, kind, name, waves, bad)
    print(json.dumps({"waves": waves, "cases": n_cases, "failed": bad}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
