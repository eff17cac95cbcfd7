"""fqg_records_split (the de-interleave behind fastq_split_interleaved) against a plain Python de-interleave of the
image's records and against fqg_records_gather with the even and the odd list.  FQGPU_SPLIT_T, FQGPU_BC_LDS and
FQGPU_TILE_WAVES are read once per process: every environment runs its cases in ONE child process (this file as a
program), which prints a line per case and leaves with status 0 when all of them held."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


# ---- the child's side ----------------------------------------------------------------------------------------------
def make_image(rng, n_records, lengths, header=b"@r%d x"):
    import numpy as np
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n_records):
        L = lengths(i)
        seq = bases[rng.integers(0, 4, L)].tobytes()
        qual = (rng.integers(2, 41, L) + 33).astype(np.uint8).tobytes()
        out.append(header % (i // 2) + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return out


class Split:
    def __init__(self):
        import fastq_utils_amd as fq
        self.fq = fq
        self.ctx = fq.Context(0)
        self.failed = []

    def frame_of(self, image):
        fq = self.fq
        st = fq.abi.probe_first_record(image[:4096], True) if image else fq.abi.FileState()
        self.ctx.validate(image, None, st, final=True,
                          flags=fq.abi.VALIDATE_FRAME_ONLY | fq.abi.VALIDATE_NO_STATS | fq.abi.VALIDATE_INDEX)
        return self.ctx.retain_frame()

    def check(self, label, image, first=0, n=None, frame=None):
        """streams 0 / 1 of records [first, first + n) == the Python de-interleave == records_gather(even / odd list)"""
        import numpy as np
        from tests import split_gen
        fr = frame or self.frame_of(image)
        total = fr.n_records
        n = total - first if n is None else n
        lines = split_gen.lines_of(image)
        assert len(lines) >= 4 * total
        want = split_gen.deinterleave(b"".join(lines[4 * first:4 * (first + n)]))
        sizes, got = self.ctx.records_split(fr, first, n, want_output=True)
        info = self.ctx.records_split_info()
        ok = sizes == (len(want[0]), len(want[1])) and got == want
        for s in (0, 1):
            lst = np.arange(first + s, first + n, 2, dtype=np.uint64)
            nb, text = self.ctx.records_gather(fr, lst, want_output=True)
            ok = ok and nb == len(want[s]) and (text or b"") == want[s]
        if frame is None:
            fr.release()
        print("%s %s: records %d..+%d bytes %s %s" % ("ok  " if ok else "FAIL", label, first, n, sizes, info), flush=True)
        if not ok:
            self.failed.append(label)
        return info, want


def child(group):
    import numpy as np
    from tests import split_gen
    S = Split()
    rng = np.random.default_rng(5)
    uniform = lambda L: (lambda i: L)
    if group == "default":
        for pairs in (0, 1, 31, 32, 33):  # (0 pairs: of a frame that holds records - a context keeps no empty frame)
            S.check("pairs_%d" % pairs, b"".join(make_image(rng, max(2 * pairs, 2), uniform(50))), 0, 2 * pairs)
        S.check("uniform_150", b"".join(make_image(rng, 2000, uniform(150))))
        recs = make_image(rng, 2000, lambda i: int(rng.integers(1, 601)))
        _, want = S.check("random_1_600", b"".join(recs))
        # every output offset mod 16 is reached in both streams (the tile images start at any skew)
        for s in (0, 1):
            seen, at = set(), 0
            for r in recs[s::2]:
                seen.add(at % 16)
                at += len(r)
            assert seen == set(range(16)), (s, sorted(seen))
        S.check("mates_26_150", b"".join(make_image(rng, 2000, lambda i: 26 if i % 2 == 0 else 150)))
        img = b"".join(make_image(rng, 200, lambda i: int(rng.integers(20, 120))))
        S.check("no_final_newline", img[:-1])
        # NUL bytes inside header, sequence and quality lines: a line ends at its first NUL
        recs = make_image(rng, 120, lambda i: int(rng.integers(30, 90)))
        for k, line in ((3, 0), (10, 1), (11, 3), (40, 0), (77, 1), (118, 3), (119, 0)):
            ln = recs[k].split(b"\n")
            ln[line] = ln[line][:7] + b"\0" + ln[line][8:]
            recs[k] = b"\n".join(ln)
        info, want = S.check("nul_bytes", b"".join(recs))
        assert info["big_tiles"] == info["tiles"] and sum(map(len, want)) < sum(map(len, recs))
        # an even first record behind the start, a range short of the end; then a smaller call on the same context
        recs = make_image(rng, 600, lambda i: int(rng.integers(10, 300)))
        img = b"".join(recs)
        fr = S.frame_of(img)
        S.check("first_246_n_300", img, 246, 300, frame=fr)
        S.check("whole_then", img, 0, 600, frame=fr)
        S.check("smaller_second_call", img, 2, 8, frame=fr)
        S.check("odd_first_record", img, 1, 598, frame=fr)
        for first, n in ((0, 3), (0, 601), (0, 602), (598, 4), (601, 0), (10, 2 ** 63)):
            try:
                S.ctx.records_split(fr, first, n)
                S.failed.append("no FQG_ERR_ARG for %d, %d" % (first, n))
            except S.fq.abi.FqgError as e:
                assert "libfqgpu error -3:" in str(e), str(e)  # FQG_ERR_ARG
        assert S.ctx.records_split(fr, 600, 0)[0] == (0, 0) and S.ctx.records_split(fr, 4, 0)[0] == (0, 0)
        fr.release()
    elif group.startswith("T"):
        T = int(group[1:])
        for pairs in (T // 2 - 1, T // 2, T // 2 + 1):
            info, _ = S.check("T%d_pairs_%d" % (T, pairs), b"".join(make_image(rng, max(2 * pairs, 2), lambda i: int(rng.integers(20, 60)))),
                              0, 2 * pairs)
            assert pairs == 0 or (info["T"] == T and info["big_tiles"] == 0), info  # (the tile kernel, not the direct path)
        if T == 2:
            # enough tiles that one wavefront walks at least four: the grid is min(tiles, resident wavefronts)
            info, _ = S.check("grid_probe", b"".join(make_image(rng, 64, uniform(30))))
            n = 4 * 2 * 256 * 32 + 2 * 1001  # four rounds of the largest grid a device of 256 CUs x 32 wavefronts gives
            info, _ = S.check("many_tiles", b"".join(make_image(rng, n, lambda i: 20 + i % 23)))
            assert info["T"] == 2 and info["tiles"] >= 4 * info["grid"] > 0 and info["big_tiles"] == 0, info
    elif group == "lds4096":
        recs = make_image(rng, 2000, lambda i: int(rng.integers(40, 100)))
        recs[777:778] = make_image(rng, 1, uniform(20000))
        info, _ = S.check("one_20kb_record", b"".join(recs))
        assert 0 < info["big_tiles"] < info["tiles"], info  # both paths ran
        recs = make_image(rng, 400, lambda i: 20000 if i % 50 == 7 else 60)
        info, _ = S.check("alternating_fit", b"".join(recs))
        assert 0 < info["big_tiles"] < info["tiles"], info
    S.ctx.close()
    print("failed:", S.failed, flush=True)
    sys.exit(1 if S.failed else 0)


# ---- the tests ---------------------------------------------------------------------------------------------------------
GROUPS = {"default": {}, "T2": {"FQGPU_SPLIT_T": "2"}, "T8": {"FQGPU_SPLIT_T": "8"}, "T64": {"FQGPU_SPLIT_T": "64"},
          "lds4096": {"FQGPU_BC_LDS": "4096"},
          # the cases of "default" with two wavefronts in k_split_emit_tile's grid: each walks many tiles (tile after next,
          # the prefetch for it, a direct tile in between)
          "default@waves2": {"FQGPU_TILE_WAVES": "2"}}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_records_split(group):
    env = {k: v for k, v in os.environ.items() if k not in ("FQGPU_SPLIT_T", "FQGPU_BC_LDS", "FQGPU_TILE_WAVES")}
    env.update(GROUPS[group])
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), group.split("@")[0]], cwd=REPO, env=env, capture_output=True, timeout=300)
    out = p.stdout.decode("latin-1") + p.stderr.decode("latin-1")[-3000:]
    print(out)
    assert p.returncode == 0, out
    assert "FAIL" not in p.stdout.decode("latin-1")


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    child(sys.argv[1])
