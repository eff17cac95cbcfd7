"""Worker of tests/test_gpu_umi.py: fqg_umi_count's table path on input that would take the per-cell path.
FQGPU_UMI_HASH_PATH is read once per process, so the test starts this one with it set.
argv: <npz with the streams> <out json>.  Every stream runs twice on ONE context: the first call of the context
takes every buffer from hipMalloc, the ones behind it from the arena the first one sized."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastq_utils_amd as fq  # noqa: E402


def main():
    assert os.environ.get("FQGPU_UMI_HASH_PATH")
    data = np.load(sys.argv[1])
    runs = []
    with fq.Context(0) as ctx:
        for name in sorted(data.files):
            stream = data[name].tobytes()
            for _ in range(2):
                got = ctx.umi_count(stream)
                runs.append({"input": name, "code": got["code"], "rl_unresolved": got["rl_unresolved"],
                             "entries": got.get("entries"), "total": got.get("total")})
    with open(sys.argv[2], "w") as f:
        json.dump(runs, f)


if __name__ == "__main__":
    main()
