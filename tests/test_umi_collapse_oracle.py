"""tests/umi_collapse_oracle.py against a brute-force restatement of the same rule on the UMIs as strings: unpacked
with the pinned uint_642char, neighbours by Hamming distance over the characters, the parent by an explicit sort.
The strings are packed with the pinned char2uint_64, which fixes what a "digit" is: A C G T N = 1..5, the first base
the least significant digit.  Needs no GPU."""
from collections import Counter, defaultdict

import numpy as np
import pytest

from oracle import umi_oracle as uo
from tests import umi_collapse_oracle as uco


def brute(string_pairs):
    """string_pairs: (cell, UMI bytes).  The rule on the strings -> table rows (cell, umi, reads, root) as strings, per-cell
    own-root counts, result."""
    reads = defaultdict(Counter)
    for c, s in string_pairs:
        reads[c][s] += 1
    table, per_cell = [], []
    absorbed = longest = 0
    for c in sorted(reads):
        r = reads[c]
        parent = {}
        for s in r:
            if not s:
                continue   # (packs to 0: no neighbours)
            cands = [t for t in r if len(t) == len(s) and sum(a != b for a, b in zip(s, t)) == 1 and r[t] > r[s]]
            cands.sort(key=lambda t: (-r[t], uo.char2uint_64(t)))
            if cands:
                parent[s] = cands[0]
        own = 0
        for s in sorted(r, key=uo.char2uint_64):
            root, steps = s, 0
            while root in parent:
                root, steps = parent[root], steps + 1
            table.append((c, s, r[s], root))
            own += steps == 0
            absorbed += steps > 0
            longest = max(longest, steps)
        per_cell.append(own)
    return table, per_cell, {"n_umis": len(table), "n_absorbed": absorbed, "n_roots": len(table) - absorbed, "longest_chain": longest}


def random_cells(seed, alphabet, n_cells):
    """small cells over the first `alphabet` bases, lengths 1..6 mixed inside a cell, reads skewed so that parents exist"""
    rng = np.random.default_rng(seed)
    bases = b"ACGTN"[:alphabet]
    pairs = []
    for c in range(n_cells):
        for _ in range(int(rng.integers(1, 40))):
            s = bytes(bases[int(x)] for x in rng.integers(0, alphabet, int(rng.integers(1, 7))))
            pairs += [(c, s)] * int(rng.integers(1, 5))
    return pairs


@pytest.mark.parametrize("alphabet", [2, 3, 5])
def test_oracle_against_the_rule_on_strings(alphabet):
    pairs = random_cells(alphabet, alphabet, 150)
    want_table, want_cells, want = brute(pairs)
    table, cells, got = uco.collapse([(c, uo.char2uint_64(s)) for c, s in pairs], 1)
    assert [(c, uo.uint_642char(u), r, uo.uint_642char(root)) for c, u, r, root in table] == want_table
    assert cells == want_cells and got == want
    if alphabet < 5:
        assert got["n_absorbed"] > 0 and got["longest_chain"] >= 2   # the rule ran


def test_digits_are_bases_first_base_least_significant():
    assert uo.char2uint_64(b"ACGTN") == 54321 and uco.digits(54321) == [1, 2, 3, 4, 5]
    assert uo.uint_642char(54321) == b"ACGTN"
    # one substitution in the string is one digit of the packed value, at the position of the base
    s = b"GATTACA"
    for p in range(len(s)):
        for b in b"ACGTN":
            t = s[:p] + bytes([b]) + s[p + 1:]
            if t != s:
                assert uo.char2uint_64(t) in uco.neighbours(uo.char2uint_64(s))
                assert uo.char2uint_64(t) - uo.char2uint_64(s) == (uo.BASE2INT[b] - uo.BASE2INT[s[p]]) * 10 ** p
    assert len(set(uco.neighbours(uo.char2uint_64(s)))) == 4 * len(s)


def test_values_without_neighbours():
    assert uco.neighbours(0) == [] and uco.neighbours(107) == [] and uco.neighbours(96) == []
    table, cells, res = uco.collapse([(1, 0), (1, 1), (1, 1), (1, 2), (1, 107), (1, 117), (1, 117)], 1)
    assert table == [(1, 0, 1, 0), (1, 1, 2, 1), (1, 2, 1, 1), (1, 107, 1, 107), (1, 117, 2, 117)]
    assert cells == [4] and res == {"n_umis": 5, "n_absorbed": 1, "n_roots": 4, "longest_chain": 1}


def test_the_difference_test_of_the_kernel_is_the_rule():
    """|a - b| = k * 10^p with 1 <= k <= 4 and a's digit p moved by k inside 1..5 <=> one digit differs (digits 1..5),
    exhaustively up to 3 digits (155 values: a fraction of a second)"""
    vals = [v for v in range(1, 556) if uco.digits(v)]
    for a in vals:
        da = uco.digits(a)
        nb = set(uco.neighbours(a))
        for b in vals:
            diff = abs(a - b)
            hit = False
            for p in range(len(da)):
                for k in range(1, 5):
                    if diff == k * 10 ** p and 1 <= da[p] + (k if b > a else -k) <= 5:
                        hit = True
            assert hit == (b in nb), (a, b)


def test_max_mismatch_0_is_the_table_alone():
    pairs = [(c, uo.char2uint_64(s)) for c, s in random_cells(9, 2, 30)]
    table, cells, res = uco.collapse(pairs, 0)
    assert all(u == root for _, u, _, root in table) and res["n_absorbed"] == 0 and res["longest_chain"] == 0
    assert sum(cells) == len(table) == len(set(pairs))
