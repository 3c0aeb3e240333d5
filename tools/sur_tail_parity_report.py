#!/usr/bin/env python3
"""``sur_tail_parity_report.py LOG [NAME]``: folds sur_tail_parity_observed.jsonl (appended by
tests/test_surrogate_tail_host.py and tests/test_surrogate_tail_gpu.py, next to the log of tests/conftest.py::check_grads)
into profiles/sur_tail_parity_observed.json: the worst error over its bound of the gradient reduction and the row fold, the
worst units of m', v' and p' per Adam spelling and step count, the two plain-fp32 spellings of the Adam expression per step
count, whether sur_adam_apply and the flush spelling agreed bit for bit, and the delta loss's worst errors in fp32
roundings per shape.  Every record carries the SHA-256 stamp of the library it was observed on; the log is append-only across
runs, so only the records of its LATEST build (the stamp of its last line) are folded and the rest are counted as dropped."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1]
out = os.path.join(ROOT, "profiles", sys.argv[2] if len(sys.argv) > 2 else "sur_tail_parity_observed.json")
sums, adam, loss, other = {}, {}, {}, {}
records = [json.loads(line) for line in open(src)]
build = records[-1].get("lib")
dropped = sum(r.get("lib") != build for r in records)
for r in records:
    if r.get("lib") != build:
        continue
    r.pop("lib", None)
    case = r["case"]
    kind = case.split("-")[0]
    if kind in ("reduction", "fold"):
        s = sums.setdefault(kind, {"launches": 0, "worst_err_over_bound": 0.0})
        s["launches"] += 1
        s["worst_err_over_bound"] = max(s["worst_err_over_bound"], r["worst_err_over_bound"])
    elif kind == "adam" and "t" in r:
        u = adam.setdefault(case[len("adam-"):], {}).setdefault(str(r["t"]), {"m": 0.0, "v": 0.0, "p": 0.0})
        for k in u:
            u[k] = max(u[k], r[k])
    elif kind == "delta":
        shape = "-".join(case.split("-")[2:5])
        u = loss.setdefault(shape, {"loss": 0.0, "hsteploss": 0.0, "means": 0.0, "stds": 0.0})
        for k in u:
            u[k] = max(u[k], r[k])
    else:
        other[case] = {k: v for k, v in r.items() if k != "case"}
res = {"library_sha256_16": build, "records_of_other_builds_dropped": dropped,
       "metric": {"reduction, fold": "max over elements of |g - fp64 sum| / ((ceil(rows / 32) + 32) u sum |partial|), asserted <= 1",
                  "adam": "tests/_sac_models.adam_units against adam_replay(fp32_hyper=True), worst element per step count; "
                          "asserted <= UNIT_BOUND = 4 (p': <= 2)",
                  "delta_loss": "relative error against the fp64 oracle in units of 2^-24, worst over storage and scaling; "
                                "asserted <= 1 (deltas, dd_all and the three call forms: bit-equal)"},
       "reduction_and_fold": sums, "adam": adam, "delta_loss": loss, **other}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps({"library": build, "dropped": dropped, "reduction_and_fold": sums, "adam_worst_p": {k: max(u["p"] for u in v.values()) for k, v in adam.items()},
                  "delta_loss_worst": {k: max(max(u[k] for u in loss.values()), 0.0) for k in ("loss", "hsteploss", "means", "stds")}
                  if loss else {}}, indent=1), "->", out)
