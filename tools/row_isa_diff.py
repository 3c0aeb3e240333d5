#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of one source file of the row kernels (csrc/rollout.hip, sur_windows.hip,
replay.hip, collect.hip; hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -S --cuda-device-only): the check of
a change that must leave the generated code alone.  A generic sibling of tools/ks_isa_diff.py: kernels are paired by
demangled name, RENAMED maps a baseline kernel that has gone to the candidate kernel that does its work now.

For each pair: VGPRs, SGPRs, scratch bytes, spills and issued instructions not above the baseline's, and the histogram of
the opcodes that start with v_, global_, flat_, buffer_ or ds_ equal.  Scalar instructions and the order of the
instructions are not compared: a refactor moves a few scalar compares and branches.

usage: tools/row_isa_diff.py BASELINE.s CANDIDATE.s >> profiles/NAME.txt   (exit status 1 if a check fails)"""
import collections
import re
import subprocess
import sys

RENAMED = {"ro_settle_kernel": "ro_settle_kernel<SettleKernelArgs>",
           "ro_settle_dissipation_kernel": "ro_settle_kernel<DissKernelArgs>",
           "co_act_kernel": "co_act_span_kernel", "co_extrema_kernel": "co_span_extrema_kernel"}
PREFIXES = ("v_", "global_", "flat_", "buffer_", "ds_")


def parse(path):
    """{demangled kernel name: (resources, instructions)}"""
    text = open(path).read()
    lines = text.splitlines()
    syms = re.findall(r"\.amdhsa_kernel (\S+)", text)
    names = subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, names):
        name = re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", name))
        name = re.sub(r"\(.*$", "", name)                  # drop the argument list
        blk = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), text, re.S).group(1)
        get = lambda key: int(re.search(r"%s (\d+)" % re.escape(key), blk).group(1))
        j = next(j for j, l in enumerate(lines) if l.split() == [".name:", sym])
        meta = dict(l.split() for l in lines[j:j + 12] if len(l.split()) == 2)
        res = {"vgpr": get(".amdhsa_next_free_vgpr"), "sgpr": get(".amdhsa_next_free_sgpr"),
               "scratch": get(".amdhsa_private_segment_fixed_size"),
               "spill": int(meta[".vgpr_spill_count:"]) + int(meta[".sgpr_spill_count:"])}
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].split()[:1] == [".section"])    # the kernel's code ends
        ins = [t for t in (l.split(";")[0].strip() for l in lines[start + 1:end])
               if t and not t.startswith(".") and not t.endswith(":")]
        out[name] = (res, ins)
    return out


def main():
    base, cand = parse(sys.argv[1]), parse(sys.argv[2])
    ok = True
    print(f"{sys.argv[1]} -> {sys.argv[2]}: {len(base)} baseline kernels, {len(cand)} candidate kernels; columns: VGPR SGPR "
          "scratch spills | issued instructions | instructions in the restricted histogram (%s*)" % "*, ".join(PREFIXES))
    for name in sorted(base):
        to = name if name in cand else RENAMED.get(name)
        if to not in cand:
            print(f"{name}\n    no candidate kernel  FAIL")
            ok = False
            continue
        (rb, ib), (rc, ic) = base[name], cand[to]
        if to != name and to in base:                      # the kernel is gone: the survivor against its own baseline
            print(f"{name}: gone, its entry launches {to}, which is compared with itself below")
            continue
        hist = lambda ins: collections.Counter(i.split()[0] for i in ins if i.startswith(PREFIXES))
        hb, hc = hist(ib), hist(ic)
        good = all(rc[k] <= rb[k] for k in rb) and len(ic) <= len(ib) and hb == hc
        ok &= good
        print(f"{name}" + (f" -> {to}" if to != name else "") +
              f"\n    {rb['vgpr']}->{rc['vgpr']} {rb['sgpr']}->{rc['sgpr']} {rb['scratch']}->{rc['scratch']} "
              f"{rb['spill']}->{rc['spill']} | {len(ib)}->{len(ic)} | {sum(hb.values())}->{sum(hc.values())}  "
              + ("ok" if good else "FAIL"))
        if hb != hc:
            print("    histogram differs:", {k: (hb[k], hc[k]) for k in sorted(set(hb) | set(hc)) if hb[k] != hc[k]})
    new = sorted(set(cand) - set(base) - set(RENAMED.values()))
    if new:
        print("new kernels (not compared):", new)
    print("all checks hold" if ok else "A CHECK FAILS")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
