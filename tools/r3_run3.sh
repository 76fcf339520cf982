#!/bin/bash
set -o pipefail
OUT=${OUT:-build/r3}; export OUT
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests/test_gpu_ops.py -x -q -k "winograd or split" > $OUT/r3_x1.log 2>&1 \
 && timeout -k 10 900 python -m pytest tests/test_gpu_wacnn.py -x -q > $OUT/r3_x2.log 2>&1 \
 && timeout -k 10 900 python -m pytest tests/test_gpu_b16.py -x -q -k "eval or trainer" > $OUT/r3_x3.log 2>&1 \
 && for v in 0 1.0e8 2.0e8 4.0e8 1.0e9; do ICM_WINO_MIN_WORK=$v timeout -k 10 300 python bench.py --no-cpu-baseline --no-extras --no-shape-table --steps 20 > $OUT/r3_b_mw_$v.json 2> $OUT/r3_b_mw_$v.err || exit 1; done \
 && ICM_SHAPE_TABLE=$OUT/r3_shapes_wino2.jsonl timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras --steps 10 > $OUT/r3_b_wino2.json 2> $OUT/r3_b_wino2.err \
 && ICM_SLICE_SPLIT=0 timeout -k 10 300 python bench.py --no-cpu-baseline --no-extras --no-shape-table --steps 20 > $OUT/r3_b_wino2_split0.json 2> $OUT/r3_b_wino2_split0.err
rc=$?
echo "chain rc=$rc"
tail -5 $OUT/r3_x1.log; tail -5 $OUT/r3_x2.log 2>/dev/null; tail -5 $OUT/r3_x3.log 2>/dev/null
python - <<PY
import json,glob
for f in sorted(glob.glob("$OUT/r3_b_mw_*.json"))+["$OUT/r3_b_wino2.json","$OUT/r3_b_wino2_split0.json"]:
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f,round(d["value"],1),"img/s",round(d["ms_per_step"],2),"ms")
    except Exception as e:
        print(f,"failed",e)
PY
exit $rc
