#!/usr/bin/env python3
"""``fno_kernel_parity_report.py LOG [NAME]``: folds fno_kernel_parity_observed.jsonl (appended by
tests/test_fno_kernels_gpu.py during `pytest -m gpu`, next to the log of tests/conftest.py::check_grads) into
profiles/fno_kernel_parity_observed.json: per case and tensor the largest e_ref (the fp32 yardstick against the fp64 oracle)
and e_hip (the kernel against the oracle), both max |diff| / max |ref|, and the maxima per weight set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1]
out = os.path.join(ROOT, "profiles", sys.argv[2] if len(sys.argv) > 2 else "fno_kernel_parity_observed.json")
cases, sets = {}, {}
for line in open(src):
    r = json.loads(line)
    t = cases.setdefault(r["case"], {}).setdefault(r["tensor"], {"e_ref": 0.0, "e_hip": 0.0})
    t["e_ref"], t["e_hip"] = max(t["e_ref"], r["e_ref"]), max(t["e_hip"], r["e_hip"])
for case, tensors in cases.items():
    weights = "stress" if "stress" in case else "default"
    for name, t in tensors.items():
        kind = "backward" if case.startswith("backward") or name.startswith("backward") else "forward"
        kind += " stage-local" if "local" in name else ""
        s = sets.setdefault(weights, {}).setdefault(kind, {"e_ref": 0.0, "e_hip": 0.0, "max_e_hip_over_bound": 0.0})
        s["e_ref"], s["e_hip"] = max(s["e_ref"], t["e_ref"]), max(s["e_hip"], t["e_hip"])
        s["max_e_hip_over_bound"] = max(s["max_e_hip_over_bound"], t["e_hip"] / max(4.0 * t["e_ref"], 2.0 ** -22))
json.dump({"metric": "max |x - x_ref| / max |x_ref| per tensor; e_ref: fp32_as_walk (tests/_fno_oracle.py) against the fp64 "
                     "oracle, e_hip: the HIP kernel against the oracle; asserted: e_hip <= max(4 e_ref, 2^-22)",
           "maxima": sets, "cases": cases}, open(out, "w"), indent=1)
print(json.dumps(sets, indent=1), "->", out)
