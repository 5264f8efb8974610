#!/bin/bash
: "${OUT:?set OUT to the directory for the logs}"
mkdir -p "$OUT"
run() {
  tag=$1; shift
  env "$@" timeout -k 10 200 python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-cross-check --check-reads 200 > "$OUT/mx_$tag.json" 2> "$OUT/mx_$tag.err"
  python - <<PY
import json
try:
    d=json.load(open("$OUT/mx_$tag.json"))
    print("$tag", round(d["ms_per_step"],2),"ms", d["config"]["check"], {s:round(x["ms"],2) for s,x in d["roofline"]["stages"].items()})
except Exception as e: print("$tag ERR", e)
PY
}
run la1 TSX_HIP_BUILD_LOOKAHEAD=1
run la2 TSX_HIP_BUILD_LOOKAHEAD=2
run la3 TSX_HIP_BUILD_LOOKAHEAD=3
run la1b TSX_HIP_BUILD_LOOKAHEAD=1
