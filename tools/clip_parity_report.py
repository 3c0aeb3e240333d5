#!/usr/bin/env python3
"""``clip_parity_report.py LOG [NAME]``: folds clip_parity_observed.jsonl (appended by tests/test_surrogate_clip_gpu.py, next
to the log of tests/conftest.py::check_grads) into profiles/clip_parity_observed.json: per case what the test observed --
the ulps of the sums of squares, the norms and coefficients of the clipped launches, the captured step's distances d0 / d1
to the eager closure with their bound and the norms it saw, the phase's two tiers.  Every record carries the SHA-256 stamp
of the library it was observed on; the log is append-only across runs, so only the records of its LATEST build (the stamp of
its last line) are kept, the last one per case, and the rest are counted as dropped."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1]
out = os.path.join(ROOT, "profiles", sys.argv[2] if len(sys.argv) > 2 else "clip_parity_observed.json")
records = [json.loads(line) for line in open(src)]
build = records[-1].get("lib")
cases = {}
for r in records:
    if r.get("lib") == build:
        cases[r["case"]] = {k: v for k, v in r.items() if k not in ("case", "lib")}
sums = {k: v for k, v in cases.items() if k.startswith("sumsq-")}
res = {"library_sha256_16": build, "records_of_other_builds_dropped": sum(r.get("lib") != build for r in records),
       "metric": {"sumsq": "|fsum(sumsq) - fsum(g^2)| in fp64 ulps, asserted <= 4; each block's entry, asserted <= 3",
                  "captured-step": "max |parameter difference| after K = 4 steps between fused_step and the eager fused closure, "
                                   "without (d0) and with (d1) the clip; asserted d1 <= 2 d0 + K lr 1e-5"},
       "sumsq_worst": {"total_ulps": max((v["total_ulps"] for v in sums.values()), default=None),
                       "worst_block_ulps": max((v["worst_block_ulps"] for v in sums.values()), default=None), "cases": len(sums)},
       **{k: v for k, v in cases.items() if k not in sums}}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1), "->", out)
