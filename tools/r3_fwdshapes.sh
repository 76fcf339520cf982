#!/bin/bash
set -o pipefail
OUT=${OUT:-build/r3}; export OUT
mkdir -p "$OUT"
ICM_SHAPE_TABLE=$OUT/r3_shapes_fwd2.jsonl timeout -k 10 300 python bench.py --full --no-cpu-baseline --fwd-only --steps 20 > $OUT/r3_b_fwd2.json 2> $OUT/r3_b_fwd2.err \
 && ICM_SHAPE_TABLE=$OUT/r3_shapes_train2.jsonl timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras --steps 10 > $OUT/r3_b_train2.json 2> $OUT/r3_b_train2.err
echo rc=$?
