#!/bin/bash
# quick look at bam_add_tags on the GPU: tests + the bench extra alone (output under $OUT_DIR/bt_quick, default out/bt_quick)
O=${OUT_DIR:-out}/bt_quick
mkdir -p $O
if [ "${1:-}" != "notest" ]; then
python -m pytest tests/test_gpu_bam_tags.py -x -q > $O/pytest.txt 2>&1
grep -n "passed\|failed\|rror" $O/pytest.txt | head -5
fi
python bench.py --full --reads 4000000 --steps 2 --no-cpu-baseline --no-e2e --no-index-extra --no-dedup-extra --no-umi-extra --no-barcodes-extra --no-filters-extra --no-shapes-extra --no-filterpair-extra --extras-out $O/bench.json > $O/bench.out 2> $O/bench.err
python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(json.dumps(d.get("bam_add_tags_extra"), indent=0)[:2500])
PY
