#!/bin/bash
# Round-end validation on the GPU box (repo root): smoke, the WHOLE GPU test suite, full bench line.  Stops at the
# first failure and exits non-zero; records the identity of the tree it ran on (tools/tree_sha.py --verify checks, in
# the build container, that nothing has changed since; it reads the record of the output folder the GPU runs bring back).
# usage: tools/final_check.sh <output dir>   (logs, final_check.json and the full bench line go there)
set -eo pipefail
OUT=${1:?usage: tools/final_check.sh <output dir>}
mkdir -p "$OUT"
SHA=$(python tools/tree_sha.py)
echo "{\"tree_sha\": \"$SHA\", \"gpu_tests_ok\": false, \"stage\": \"started\"}" > $OUT/final_check.json
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/final_smoke.log 2>&1 || { tail -5 $OUT/final_smoke.log; echo "SMOKE FAILED"; exit 1; }
tail -2 $OUT/final_smoke.log
if ! timeout -k 10 900 python -m pytest tests -x -q -m gpu -p no:cacheprovider > $OUT/t_all.log 2>&1; then
  grep -E "^(FAILED|ERROR)|Fatal Python error|Aborted" $OUT/t_all.log | head -5 || true
  tail -5 $OUT/t_all.log | cut -c1-300
  echo "GPU SUITE FAILED"
  exit 1
fi
tail -2 $OUT/t_all.log | cut -c1-200
SUMMARY=$(tail -1 $OUT/t_all.log | tr -d '"')
echo "{\"tree_sha\": \"$SHA\", \"gpu_tests_ok\": true, \"summary\": \"$SUMMARY\"}" > $OUT/final_check.json
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
OUT="$OUT" python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "bench_default.json")))
print(d["config"]["workload"])
print("value", d["value"], "frac", d["roofline"]["frac"], "c2 frac", d.get("workload_c2", {}).get("roofline", {}).get("frac"))
t = d.get("tbptt", {})
print("tbptt N256", t.get("value"), "eager fused", t.get("eager_fused", {}).get("value"), "n64", t.get("n64", {}).get("value"))
PY
