#!/bin/bash
# quick look at the tile kernels on the GPU (fastq_pre_barcodes + the record filters): the two bench extras alone
O=${OUT_DIR:-out}/bc_quick
mkdir -p $O
python bench.py --full --reads ${1:-100000000} --steps 2 --no-cpu-baseline --no-e2e --no-index-extra --no-dedup-extra --no-umi-extra --no-shapes-extra --no-filterpair-extra --no-tags-extra --extras-out $O/bench.json > $O/bench.out 2> $O/bench.err
python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.items():
    if "barcode" in k or "filter" in k:
        v = {a: b for a, b in v.items() if a not in ("cpu_baseline", "whitelist_stage", "what")}
        print(k, json.dumps(v)[:1500])
PY
