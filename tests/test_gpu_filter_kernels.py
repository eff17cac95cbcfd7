"""fqg_records_filter and fqg_records_gather through the C ABI on the families of tests/filter_cases.py: every family
in this process at the default tile size, the tile families again under FQGPU_BC_LDS = 4096 and 65536, and the tile
walk under FQGPU_TILE_WAVES = 1, 2, 3 - one child process per environment (the library reads both variables once),
one child at a time.  The expectations are the Python oracle's; nothing here needs oracle/_ref."""
import json
import os
import subprocess
import sys

import pytest

from tests import filter_cases as fc
from tests.util import REPO

pytestmark = pytest.mark.gpu
KNOBS = ("FQGPU_BC_LDS", "FQGPU_TILE_WAVES")
CHILDREN = {"tiles_lds4096": ("tiles", {"FQGPU_BC_LDS": "4096"}), "tiles_lds65536": ("tiles", {"FQGPU_BC_LDS": "65536"}),
            "walk_waves1": ("walk", {"FQGPU_TILE_WAVES": "1"}), "walk_waves2": ("walk", {"FQGPU_TILE_WAVES": "2"}),
            "walk_waves3": ("walk", {"FQGPU_TILE_WAVES": "3"})}


@pytest.fixture(scope="module")
def runner():
    r = fc.Runner()
    yield r
    r.close()


@pytest.mark.parametrize("family", [f for f in fc.FAMILIES if f != "tile_walk"])
def test_family(runner, family):
    n, bad = fc.run_families([family], runner)
    assert n > 0 and bad == []


@pytest.mark.parametrize("name", sorted(CHILDREN))
def test_families_in_another_environment(name):
    group, knobs = CHILDREN[name]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    p = subprocess.run([sys.executable, "-m", "tests.filter_cases", group], cwd=REPO, env=env, capture_output=True, timeout=300)
    out, err = p.stdout.decode("latin-1"), p.stderr.decode("latin-1")
    assert out.strip(), err[-3000:]
    res = json.loads(out.strip().split("\n")[-1])
    assert res["group"] == group and res["env"] == {k: knobs.get(k) for k in KNOBS}
    assert res["cases"] == sum(len(fc.cases_of(f, env)) for f in fc.GROUPS[group])
    assert res["failed"] == [] and p.returncode == 0, err[-3000:]
