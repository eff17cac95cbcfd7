#!/bin/bash
# quick look at the fastq_filterpair bench extra (output under $OUT_DIR/fp_quick, default out/fp_quick)
O=${OUT_DIR:-out}/fp_quick
mkdir -p $O
python bench.py --full --reads 4000000 --steps 2 --no-cpu-baseline --no-e2e --no-index-extra --no-dedup-extra --no-umi-extra --no-barcodes-extra --no-filters-extra --no-shapes-extra --no-tags-extra ${FP_ARGS:-} --extras-out $O/bench.json > $O/bench.out 2> $O/bench.err
python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(json.dumps(d.get("filterpair_extra"), indent=0)[:2500])
PY
tail -3 $O/bench.err
