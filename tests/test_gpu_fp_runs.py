"""The owner side of the read-name exchange on arrays: k_fp_runs and k_fp_pair_runs (fqg_index_kernels.hip) classify
runs of equal fingerprints in the sorted order.  Whole-file pairing runs reach them only with the runs real names make;
here the (fingerprint, index) pairs are made in numpy - every shape of run, a run across the border of two workgroups,
a run as the last elements, equal fingerprints under different check bits, a `cap` smaller than the output - and
FingerprintSet.candidates() / pair_runs() are held against the model of the comment above k_fp_pair_runs
(tests/name_model.py: candidates_model, pair_runs_model).

Not here: the clamp of a fingerprint at kSlotEmpty - 1 (k_names_fingerprint).  It needs a name whose hash is one of the
two largest 64-bit values - a preimage of name_fin - and cannot be reached from a name anybody can write down; feeding
the set such a value by hand would test the set, which does not clamp."""
import ctypes as C

import numpy as np
import pytest

import fastq_utils_amd as fq
from tests import name_model as nm

pytestmark = pytest.mark.gpu
F2 = nm.FP_FILE2
# (holders, askers, the two carry different check bits)
SHAPES = [(1, 1, False), (1, 1, True), (2, 0, False), (0, 2, False), (2, 1, False), (1, 2, False), (3, 3, False),
          (1, 0, False), (0, 1, False)]


def build(n, seed, at_border=False):
    """n entries in a shuffled arrival order: runs of every shape; at_border: entries 255..257 of the sorted order are
    one run (two holders and an asker), the last six another (3, 3)"""
    rng = np.random.default_rng(seed)
    shapes = []
    if at_border:
        shapes = [(1, 0, False)] * 255 + [(2, 1, False)]
    tail = [(3, 3, False)] if n >= 300 else []
    room = n - sum(h + a for h, a, _ in shapes + tail)
    k = 0
    while room > 0:
        h, a, d = SHAPES[(k * 5 + int(rng.integers(0, 3))) % len(SHAPES)]
        k += 1
        if h + a > room:
            h, a, d = (1, 0, False) if k % 2 else (0, 1, False)
        shapes.append((h, a, d))
        room -= h + a
    shapes += tail
    keys = rng.integers(1, 1 << 61, len(shapes) * 2, dtype=np.uint64) * np.uint64(4) + np.uint64(1)
    keys = np.unique(keys)[:len(shapes)]
    assert len(keys) == len(shapes)
    fps, idx, g = [], [], 0
    slots = list(rng.permutation(n + 50))       # record indices, in no order: first_unpaired is a true minimum
    for f, (h, a, differ) in zip(keys.tolist(), shapes):
        chk = int(rng.integers(0, 1 << 23))
        for j in range(h + a):
            c = chk if not (differ and j) else chk ^ (1 + int(rng.integers(0, 1 << 22)))
            fps.append(f)
            idx.append(int(slots[g]) | (c << 40) | (F2 if j >= h else 0))
            g += 1
    assert g == n
    order = rng.permutation(n)
    return [fps[i] for i in order], [idx[i] for i in order]


def on_device(fps, idx):
    import torch
    pairs = np.empty((len(fps), 2), dtype=np.uint64)
    pairs[:, 0], pairs[:, 1] = fps, idx
    t = torch.from_numpy(pairs.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def records_on_device(recs):
    import torch
    t = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("n,at_border", [(1, False), (2, False), (256, False), (257, False), (258, True), (3001, True), (3000, False)])
def test_runs_against_the_model(n, at_border):
    fps, idx = build(n, 100 + n, at_border)
    want, want_ent = nm.pair_runs_model(fps, idx)
    want_cand = nm.candidates_model(fps, idx)
    if at_border:
        order, runs = nm.runs_of(fps)
        assert (255, 258) in runs and (n < 300 or runs[-1] == (n - 6, n))
    if n >= 3000:
        assert all(want.values()) and want["n_complex"] > 100   # every kind of run is there
    with fq.Context(0) as ctx:
        buf = on_device(fps, idx)
        s = ctx.fingerprint_set(16)                # (smaller than the input: the set grows)
        half = n // 2
        s.insert(buf.data_ptr(), half)
        s.insert(buf.data_ptr() + 16 * half, n - half)
        got, ent = s.pair_runs()
        assert got == want, (got, want)
        assert sorted(ent) == want_ent
        cand, found = s.candidates()
        assert found == len(want_cand) and sorted(cand) == want_cand
        s.close()


def test_equal_fingerprints_with_other_check_bits_are_no_pair_but_are_candidates():
    fps = [1000, 1000, 2000, 2000]
    idx = [7 | (5 << 40), F2 | 9 | (5 << 40), 3 | (5 << 40), F2 | 4 | (6 << 40)]
    with fq.Context(0) as ctx:
        buf = on_device(fps, idx)
        s = ctx.fingerprint_set(16)
        s.insert(buf.data_ptr(), 4)
        got, ent = s.pair_runs()
        assert got == {"matched": 1, "leftover": 0, "unpaired": 0, "first_unpaired": None, "n_complex": 2}
        assert sorted(ent) == [(2, 3), (2, F2 | 4)]
        cand, found = s.candidates()           # k_fp_runs: the check bits are not part of the index
        assert found == 2 and sorted(cand) == [(3, F2 | 4), (7, F2 | 9)]
        s.close()


def test_a_cap_smaller_than_the_output():
    """n_found / n_complex are the true counts, what is handed out is part of the true output, and the words behind
    `cap` entries of the caller's buffer stay as they were"""
    n = 3001
    fps, idx = build(n, 7, True)
    want, want_ent = nm.pair_runs_model(fps, idx)
    want_cand = nm.candidates_model(fps, idx)
    L = fq.abi.load()
    with fq.Context(0) as ctx:
        buf = on_device(fps, idx)
        s = ctx.fingerprint_set(n)
        s.insert(buf.data_ptr(), n)
        for cap in (0, 1, 5, 64):
            guard = 0xA5A5A5A5A5A5A5A5
            out = (C.c_uint64 * (2 * cap + 8))(*([guard] * (2 * cap + 8)))
            r = fq.abi.PairSummary()
            ctx._check(L.fqg_fpset_pair_runs(ctx.h, s.h, C.byref(r), out, cap))
            assert r.n_complex == want["n_complex"] > 64 and (r.matched, r.leftover, r.unpaired) == (want["matched"], want["leftover"], want["unpaired"])
            got = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(cap)]
            assert len(set(got)) == cap and set(got) <= set(want_ent)
            assert all(int(out[i]) == guard for i in range(2 * cap, 2 * cap + 8))
            out = (C.c_uint64 * (2 * cap + 8))(*([guard] * (2 * cap + 8)))
            found = C.c_uint64()
            ctx._check(L.fqg_fpset_candidates(ctx.h, s.h, out, cap, C.byref(found)))
            assert found.value == len(want_cand) > 64
            got = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(cap)]
            assert len(set(got)) == cap and set(got) <= set(want_cand)
            assert all(int(out[i]) == guard for i in range(2 * cap, 2 * cap + 8))
        s.close()


def test_with_names_the_bytes_decide():
    """fqg_fpset_insert_named: a holder and its asker with equal fingerprints AND check bits pair only when their name
    records are the same bytes of a name that fits a record; every other (1, 1) run goes to the resolution by index"""
    tw = nm.twins(2, length=48, word=5, high=True)
    long_one = b"L" * 57
    rows = [  # (fingerprint, index word, name)
        (500, 1 | (9 << 40), b"same"), (500, F2 | 11 | (9 << 40), b"same"),                      # a pair
        (600, 2 | (9 << 40), tw[0]), (600, F2 | 12 | (9 << 40), tw[1]),                          # 87 equal bits, other bytes
        (700, 3 | (9 << 40), long_one), (700, F2 | 13 | (9 << 40), long_one),                    # beyond what a record holds
        (800, 4 | (9 << 40), b"x" * 56), (800, F2 | 14 | (9 << 40), b"x" * 56),                  # exactly what it holds: a pair
        (900, 5 | (9 << 40), b"ab"), (900, F2 | 15 | (9 << 40), b"ab\0"),                        # equal bytes, other length
        (950, 6 | (9 << 40), b"same"), (950, F2 | 16 | (8 << 40), b"same"),                      # other check bits: complex
        (990, 7, b"alone"), (995, F2 | 17, b"asks"),
    ]
    rng = np.random.default_rng(2)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    fps, idx, recs = [r[0] for r in rows], [r[1] for r in rows], [nm.travel_record(r[2]) for r in rows]
    want, want_ent = nm.pair_runs_model(fps, idx, recs)
    assert want == {"matched": 2, "leftover": 1, "unpaired": 1, "first_unpaired": 17, "n_complex": 8}
    with fq.Context(0) as ctx:
        buf, names = on_device(fps, idx), records_on_device(recs)
        s = ctx.fingerprint_set(16)
        s.insert(buf.data_ptr(), 6, names.data_ptr())
        s.insert(buf.data_ptr() + 16 * 6, len(rows) - 6, names.data_ptr() + 64 * 6)
        got, ent = s.pair_runs()
        assert got == want, (got, want)
        assert sorted(ent) == want_ent
        s.close()
        # the same pairs without their names: the fingerprints and check bits are all there is
        s = ctx.fingerprint_set(16)
        s.insert(buf.data_ptr(), len(rows))
        got, ent = s.pair_runs()
        assert got == nm.pair_runs_model(fps, idx)[0] and got["matched"] == 5
        s.close()
