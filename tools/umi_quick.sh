#!/bin/bash
# quick look at the bam_umi_count kernels on configs[3]: tests + the bench extra alone (output under $OUT_DIR/umi_quick, default out/umi_quick)
O=${OUT_DIR:-out}/umi_quick
mkdir -p $O
if [ "${1:-}" != "notest" ]; then
python -m pytest tests/test_gpu_umi.py -x -q > $O/pytest.txt 2>&1
grep -n "passed\|failed\|rror" $O/pytest.txt | head -5
fi
FQGPU_RL_DEBUG=1 python bench.py --full --reads 4000000 --steps 2 --no-cpu-baseline --no-e2e --no-index-extra --no-dedup-extra --no-barcodes-extra --no-filters-extra --no-shapes-extra --no-filterpair-extra --extras-out $O/bench.json > $O/bench.out 2> $O/bench.err
grep "^\[rl\]" $O/bench.err | tail -2
python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
u = d["umi_count_extra"]
print(u["kernels_ms"], json.dumps(u["kernels_ms_breakdown"]))
print(u["matrix_identical_to_reference_program"], u["rl_tree_replay"])
PY
