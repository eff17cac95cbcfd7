#!/bin/bash
# quick look at fastq_pre_barcodes on the GPU: tests + the bench extra alone (output under $OUT_DIR/bc_quick, default out/bc_quick)
O=${OUT_DIR:-out}/bc_quick
mkdir -p $O
if [ "${1:-}" != "notest" ]; then
python -m pytest tests/test_gpu_pre_barcodes.py tests/test_gpu_filters.py -x -q > $O/pytest.txt 2>&1
grep -n "passed\|failed\|rror" $O/pytest.txt | head -5
fi
python bench.py --full --reads 4000000 --steps 2 --no-cpu-baseline --no-e2e --no-index-extra --no-dedup-extra --no-umi-extra --no-filters-extra --no-shapes-extra --no-filterpair-extra --extras-out $O/bench.json > $O/bench.out 2> $O/bench.err
python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.items():
    if "barcode" in k:
        print(k, json.dumps({a: b for a, b in v.items() if a != "cpu_baseline"})[:1800])
PY
