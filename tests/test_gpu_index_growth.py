"""A name index that grows while it holds earlier frames (index_grow, fqg_index_abi.inc): three images of 3000 records
with 9000 distinct names go one after another into an index made for 1024 names.  The table goes 2048 -> 8192 -> 16384 ->
32768 slots; the second insert re-inserts one retained segment through k_index_insert(regrow), the third two.  Directly on
the ABI, with FQGPU_STREAM_MIN=256 so that the images reach the streaming pass, over the three name sources: the line
index, the capture records (FQG_VALIDATE_NAMES) and the digests (FQG_VALIDATE_NAME_DIGESTS, an index that keeps no
names).  Every expectation is made in Python: the counts, who answers whom, the duplicate's record."""
import os

import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import fuzz

pytestmark = pytest.mark.gpu
N = 3000
E_DUP_NAME = 3  # FQG_E_DUP_NAME
# (name, validate flags, the index will be asked)
SOURCES = [("lines", 0, True), ("records", fq.abi.VALIDATE_NAMES, True), ("digests", fq.abi.VALIDATE_NAME_DIGESTS, False)]


def records(img):
    lines = img.split(b"\n")
    return [b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range((len(lines) - 1) // 4)]


@pytest.fixture(scope="module")
def images():
    """three images of N records, 3 N distinct names; a fourth with all of them in a seeded order and, per asker, the
    insertion-order record of its name; a third image with record 1234 of the first again at position 2000"""
    imgs = [fuzz.make_fastq(np.random.default_rng(70 + k), N, 50, 150, "casava", first_index=k * N) for k in range(3)]
    recs = [r for img in imgs for r in records(img)]
    assert len(recs) == 3 * N
    where = {r.split(b"\n", 1)[0].split(b" ")[0]: i for i, r in enumerate(recs)}
    assert len(where) == 3 * N
    perm = np.random.default_rng(7).permutation(3 * N)
    askers = b"".join(recs[i] for i in perm)
    want = np.array([where[recs[i].split(b"\n", 1)[0].split(b" ")[0]] for i in perm], dtype=np.uint64)
    third = records(imgs[2])
    dup = b"".join(third[:2000] + [recs[1234]] + third[2000:])
    return {"imgs": imgs, "askers": askers, "want": want, "dup": dup}


@pytest.fixture()
def streamed():
    old = {k: os.environ.get(k) for k in ("FQGPU_STREAM_MIN", "FQGPU_NAMES_BUILD")}
    os.environ["FQGPU_STREAM_MIN"] = "256"
    os.environ.pop("FQGPU_NAMES_BUILD", None)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def insert_all(ctx, idx, st, imgs, flags):
    out = []
    for img in imgs:
        r = ctx.validate(img, None, st, flags=fq.abi.VALIDATE_NO_STATS | flags)
        assert r["code"] == 0, r
        out.append(idx.insert_unique(st))
    return out


def load_frames(idx):
    return int(fq.abi.load().fqg_index_n_frames(idx.h))


def new_index(ctx, lookups):
    idx = ctx.name_index(1024)
    if not lookups:
        idx.expect_lookups(False)
    return idx


@pytest.mark.parametrize("build", [None, "1"], ids=["by_size", "build"])
def test_three_inserts_grow_the_table(images, streamed, build):
    """n_entries 3000, 6000, 9000 with no finding, index_mem the same whichever way the names came; build: the second and
    third insert merge into a table that is not empty (FQGPU_NAMES_BUILD=1)"""
    if build:
        os.environ["FQGPU_NAMES_BUILD"] = build
    mem = {}
    with fq.Context(0) as ctx:
        st = fq.abi.probe_first_record(images["imgs"][0], False)
        for name, flags, lookups in SOURCES:
            idx = new_index(ctx, lookups)
            got = insert_all(ctx, idx, st, images["imgs"], flags)
            print(name, got)
            assert [(g["code"], g["n_entries"]) for g in got] == [(0, N), (0, 2 * N), (0, 3 * N)], (name, got)
            assert load_frames(idx) == 3
            mem[name] = [g["index_mem"] for g in got]
            idx.close()
    assert mem["lines"] == mem["records"] == mem["digests"], mem


@pytest.mark.parametrize("name,flags,lookups", SOURCES[:2], ids=[s[0] for s in SOURCES[:2]])
def test_every_name_answers_after_growth(images, streamed, name, flags, lookups):
    """all 9000 names asked in a seeded order: each asker gets the insertion-order record of its name, nothing is left"""
    with fq.Context(0) as ctx:
        st = fq.abi.probe_first_record(images["imgs"][0], False)
        idx = new_index(ctx, lookups)
        got = insert_all(ctx, idx, st, images["imgs"], flags)
        assert [(g["code"], g["n_entries"]) for g in got] == [(0, N), (0, 2 * N), (0, 3 * N)], got
        r = ctx.validate(images["askers"], None, st, flags=fq.abi.VALIDATE_NO_STATS | flags)
        assert r["code"] == 0, r
        mr, match = idx.probe_delete_np(st, 3 * N)
        print(name, mr, int((match != images["want"]).sum()))
        assert mr["code"] == 0, mr
        assert np.array_equal(match, images["want"])
        assert mr["n_entries"] == 0, mr
        assert not idx.alive_np(3 * N).any()
        idx.close()


@pytest.mark.parametrize("name,flags,lookups", SOURCES, ids=[s[0] for s in SOURCES])
def test_a_name_of_the_first_frame_again_in_the_third(images, streamed, name, flags, lookups):
    """the finding is the third frame's, at the record's place in that frame"""
    with fq.Context(0) as ctx:
        st = fq.abi.probe_first_record(images["imgs"][0], False)
        idx = new_index(ctx, lookups)
        got = insert_all(ctx, idx, st, images["imgs"][:2] + [images["dup"]], flags)
        print(name, got)
        assert [(g["code"], g["n_entries"]) for g in got[:2]] == [(0, N), (0, 2 * N)], got
        assert (got[2]["code"], got[2]["record"]) == (E_DUP_NAME, 2000), got[2]
        idx.close()
