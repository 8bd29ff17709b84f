#!/bin/bash
LOG=$(mktemp) || exit 1
export LOG
for r in 1 2; do
  for L in ab/base/libcv.so ab/cur/libcv.so; do
    CV_LIB_PATH=$L timeout -k 10 300 python bench.py --full --no-cpu --no-sub --no-keyed --steps 3 > "$LOG" 2>&1 || exit 1
    python - "$L" <<'PY'
import json,os,sys
d=json.loads([l for l in open(os.environ["LOG"]) if l.startswith("{")][-1])
n=d["notary"]; sw={s["batch"]:(round(s["p50_ms"],4), round(s["breakdown_p50_ms"]["transfers_and_host"],4)) for s in d["notary_sweep"]}
print(sys.argv[1], "4096", round(n["p50_ms"],4), round(n["breakdown_p50_ms"]["transfers_and_host"],4), sw)
PY
  done
done
rm -f "$LOG"
