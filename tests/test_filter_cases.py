"""tests/filter_cases.py without a GPU: the generators show the properties they claim (their own assertions run when a
family is made), the pinned counts of the exhaustive poly-A/T image, and every expectation of a filter family is what
oracle/filter_oracle.py gives for the whole image (the programs' restatement: argument parsing, gzgets, the counters)."""
import pytest

from oracle import filter_oracle as fo
from tests import filter_cases as fc

BUDGETS = {"default": {}, "lds4096": {"FQGPU_BC_LDS": "4096"}, "lds65536": {"FQGPU_BC_LDS": "65536"}}
FILTER_FAMILIES = [f for f in fc.FAMILIES if f not in ("span", "pieces", "nul", "tile_walk")]


@pytest.mark.parametrize("family", [f for f in fc.FAMILIES if f != "tile_walk"])
def test_a_family_is_made_and_holds_its_properties(family):
    cases = fc.cases_of(family, {})
    assert cases and len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        assert b"~" not in c["image"]
        assert max(len(r[0]) for r in fc.records_of(c["image"])) < 1000  # (a longer header is cut by the reference's gzgets)


@pytest.mark.parametrize("budget", ["lds4096", "lds65536"])
@pytest.mark.parametrize("family", ["tile_edge", "tile_mix"])
def test_the_tile_families_at_the_other_budgets(family, budget):
    cases = fc.cases_of(family, BUDGETS[budget])
    assert {c["tile"] for c in cases if family == "tile_edge"} in (set(), {fc.tile_for(150, 1, int(BUDGETS[budget]["FQGPU_BC_LDS"]))[:2]})
    assert len(cases) == (48 if family == "tile_edge" else len(fc.TILE_MIX) + 1)


def test_tile_for_restates_the_library():
    # (worked by hand from bc_tile_for: records of 150 bytes at the three budgets)
    assert fc.tile_for(150, 1, 24576) == (57, 9168, 15408)
    assert fc.tile_for(150, 1, 4096) == (9, 1536, 2560)
    assert fc.tile_for(150, 1, 65536) == (64, 10272, 55264)
    assert fc.tile_for(40000, 1, 4096) == (1, 2048, 2048)  # (in_cap + 1024 > budget: half of it)


def test_tile_edge_crosses_the_edge_once():
    for env in BUDGETS.values():
        cases = fc.cases_of("tile_edge", env)
        T, in_cap = cases[0]["tile"]
        sweep = [sum(fc.direct_tiles(fc.records_of(c["image"]), 0, 6 * T, T, in_cap)) for c in cases]
        assert len(cases) == 48 and set(sweep) == {0, 1}
        assert len({len(c["image"]) for c in cases}) == 1


@pytest.mark.parametrize("waves", [1, 2, 3])
def test_tile_walk_has_a_wavefront_walk_one_to_five_tiles(waves):
    cases = fc.tile_walk(fc.DEFAULT_BUDGET, waves)
    assert [c["tiles"] for c in cases] == [waves, waves + 1, 2 * waves, 2 * waves + 1, 3 * waves + 1, 5 * waves]
    assert all(c["grid"] == min(waves, c["tiles"]) for c in cases) and cases[-1]["tiles"] >= 4 * cases[-1]["grid"]
    for c in cases:
        recs = fc.records_of(c["image"])
        flags = fc.direct_tiles(recs, 0, len(recs), *c["tile"])
        assert len(flags) == c["tiles"] and (c["tiles"] < 3 or 0 < sum(flags) < len(flags))


def test_the_exhaustive_image_gives_the_pinned_counts():
    first, second = fc.cases_of("poly_exhaustive", {})
    assert len(fc.records_of(first["image"])) == 9331 and len(first["image"]) == 154897
    assert len(fc.records_of(second["image"])) == 781
    assert [(c["min_poly"], c["min_len"]) for c in first["calls"]] == list(fc.POLY_SETTINGS)
    want = [fc.want_of(first, c) for c in first["calls"]]
    for k, pinned in fc.POLY_PINNED.items():
        assert tuple(w[k] for w in want[:5]) == pinned
    assert want[5]["n_trimmed"] == 0 and want[5]["n_discarded"] == 0  # min_poly -1: nothing is trimmed
    assert want[6]["n_discarded"] == 9331 and want[6]["out_bytes"] == 0  # min_len -1 is 2^64 - 1


def test_the_n_families_reach_both_sides_of_their_edges():
    a, b = fc.cases_of("n_alignment", {})
    ra, rb = fc.records_of(a["image"]), fc.records_of(b["image"])
    at, starts = 0, set()
    for r in ra:
        starts.add(((at + len(r[0])) % 16, len(r[1]) - 1))
        assert r[0].endswith(b"NnNnNnNnNnNnNnNn\n") and r[2] == b"+\n" and set(r[3][:-1]) <= set(b"Nn") and not set(r[1]) & set(b"Nn")
        at += sum(map(len, r))
    assert {(p, L) for p in range(16) for L in fc.N_LENGTHS} <= starts
    assert all((x - p) in {L for q, L in starts if q == p} for p in range(16) for x in (16, 32, 256) if x - p > 0)
    at, seen = 0, set()
    for r in rb:
        pre, seq = (at + len(r[0])) % 16, r[1][:-1]
        hits = [i for i, ch in enumerate(seq) if ch in b"Nn"]
        assert len(hits) == 1 and not set(r[0] + r[2] + r[3]) & set(b"Nn")
        seen.add((pre, len(seq), hits[0]))
        at += sum(map(len, r))
    for pre in range(16):
        for L in fc.N_LENGTHS:
            assert {(pre, L, p) for p in fc.n_positions(pre, L)} <= seen
    assert (3, 513, 0) in seen and (3, 513, 512) in seen and (3, 513, 252) in seen and (3, 513, 253) in seen  # 3 + 253 = 256
    for c in fc.cases_of("n_threshold", {}):
        w = fc.want_of(c, c["calls"][0])
        assert 0 < w["n_kept"] and (c["calls"][0]["max_n"] >= 100 or 0 < w["n_discarded"])


def whole_image(case, c):
    recs = fc.records_of(case["image"])
    n = len(recs) - c["first"] if c["n"] is None else c["n"]
    return b"".join(b"".join(r) for r in recs[c["first"]:c["first"] + n])


@pytest.mark.parametrize("family", FILTER_FAMILIES)
def test_expectations_are_the_oracles_for_the_whole_image(family):
    for case in fc.cases_of(family, {}):
        for c in case["calls"]:
            image = whole_image(case, c)
            if not image:
                continue
            want = fc.want_of(case, c)
            if c["mode"] == fc.FILTER_N:
                r = fo.filter_n(["-n", str(c["max_n"]), "in.fastq"], lambda p: image)
                assert r["exit"] == 0 and r["stdout"] == want["text"], (case["name"], c)
            else:
                r = fo.trim_poly_at(["--file", "in.fastq", "--outfile", "o", "--min_poly_at_len", str(c["min_poly"]), "--min_len",
                                     str(c["min_len"])], lambda p: image)
                assert r["exit"] == 0 and r["out"] == want["text"], (case["name"], c)
                assert r["stderr"].endswith(b"INFO:Reads processed: %d\nINFO:Reads trimmed: %d\nINFO:Reads discarded: %d\n" % (
                    want["n_records"], want["n_trimmed"], want["n_discarded"]))


def test_gather_families_cover_their_paths():
    s = fc.cases_of("span", {})[0]
    recs = fc.records_of(s["image"])
    assert not s["image"].endswith(b"\n") and any(order[-1] == len(recs) - 1 for _, order in s["lists"])
    sizes = [sum(map(len, r)) for r in recs]
    totals = {(len(order) - 64, sum(sizes[k] for k in order[64:])) for name, order in s["lists"] if name.startswith("run_")}
    assert {(m, B) for m in fc.SPAN_M for B in fc.SPAN_BYTES if B >= fc.SMALLEST * m} <= totals
    for name, order in s["lists"]:
        if name.startswith("run_"):
            assert all(b == a + 1 for a, b in zip(order[64:], order[65:])) and all(b != a + 1 for a, b in zip(order[:64], order[1:64]))
    p = fc.cases_of("pieces", {})[0]
    sizes = [sum(map(len, r)) for r in fc.records_of(p["image"])]
    assert set(fc.PIECE_SIZES) <= set(sizes) and sizes[-1] == 16
    over = {name: sum(1 for k in order if sizes[k] > 1024) for name, order in p["lists"]}
    assert all(v == 0 for k, v in over.items() if k.startswith("small_")) and all(v == 1 for k, v in over.items() if k.startswith("one_large_"))
    assert {len(order) for name, order in p["lists"] if name.startswith("small_")} == set(range(1, 10)) | {63, 64, 65, 2051}
