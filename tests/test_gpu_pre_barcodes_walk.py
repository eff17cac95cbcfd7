"""k_bc_emit_tile walking more tiles than it has wavefronts, as FASTQ text and as SAM lines, for READ1 alone, READ1 +
READ2, READ1 + INDEX1 and READ1 + INDEX2 (the kernel for any set of files, which keeps no spans in flight): the cases of
tests/pb_walk_cases.py against oracle/pre_barcodes_oracle.py, in a process of their own per grid - the library reads
FQGPU_BC_LDS and FQGPU_TILE_WAVES once.  A case whose debug line (FQGPU_BC_DEBUG) does not show the walk it was built for -
T, grid = min(wavefronts, tiles), the big tiles - fails there."""
import json
import os
import subprocess
import sys

import pytest

from tests.util import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("waves", ["1", "2", "3"])
def test_transform_with_few_wavefronts_in_the_grid(waves):
    env = dict(os.environ, FQGPU_BC_LDS="4096", FQGPU_TILE_WAVES=waves, FQGPU_BC_DEBUG="1")
    p = subprocess.run([sys.executable, "-m", "tests.pb_walk_cases"], cwd=REPO, env=env, capture_output=True, timeout=300)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert out.strip(), err[-2000:]
    res = json.loads(out.strip().split("\n")[-1])
    assert res["waves"] == int(waves) and res["cases"] > 200
    assert res["failed"] == [] and p.returncode == 0
