"""The census with UMI collapse (fqg_census_collapse_umis, include/fqg.h) restated in plain Python over a list of
(cell, UMI) pairs of packed values.  Not a reference result - the reference counts every distinct UMI - so the
definition is the contract, and this is the definition:

  neighbours  two values of the same digit count that differ in exactly one decimal digit; 0, and a value with a digit
              that is not 1..5 (no UMI packs to one), have none
  parent      the neighbour of the same cell with strictly more reads that has the most reads; the smallest value among
              equally strong ones
  root        follow parent until there is none

collapse(pairs, max_mismatch) -> (table, per_cell, result): the table rows (cell, umi, reads, root) sorted by
(cell, umi); per cell, in ascending order, the number of values that are their own root; the result struct as a dict."""
from collections import Counter, defaultdict


def digits(v: int):
    """the decimal digits of a packed value, least significant (the first base) first; None: a value without neighbours"""
    if v <= 0:
        return None
    out = []
    while v:
        out.append(v % 10)
        v //= 10
    return out if all(1 <= x <= 5 for x in out) else None


def neighbours(v: int):
    """every value that differs from v in exactly one digit, over the digits 1..5"""
    ds = digits(v)
    if ds is None:
        return []
    return [v + (x - d) * 10 ** p for p, d in enumerate(ds) for x in range(1, 6) if x != d]


def collapse(pairs, max_mismatch=1):
    assert max_mismatch in (0, 1)
    reads = defaultdict(Counter)
    for c, u in pairs:
        reads[c][u] += 1
    table, per_cell = [], []
    n_absorbed = longest = 0
    for c in sorted(reads):
        r = reads[c]
        parent = {}
        if max_mismatch:
            for u in r:
                stronger = [(-r[v], v) for v in neighbours(u) if v in r and r[v] > r[u]]
                if stronger:
                    parent[u] = min(stronger)[1]
        own = 0
        for u in sorted(r):
            root, steps = u, 0
            while root in parent:
                root, steps = parent[root], steps + 1
            table.append((c, u, r[u], root))
            own += steps == 0
            n_absorbed += steps > 0
            longest = max(longest, steps)
        per_cell.append(own)
    result = {"n_umis": len(table), "n_absorbed": n_absorbed, "n_roots": len(table) - n_absorbed, "longest_chain": longest}
    return table, per_cell, result
