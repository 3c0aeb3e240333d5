#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of csrc/ks_kernels.hip (hipcc -O3 -std=c++17 -ffp-contract=off
--offload-arch=gfx950 -S --cuda-device-only, the line of tools/ks_isa_mix.py): the check of a change that must leave the
generated code alone.  The sub-step loop is delimited as in ks_isa_mix.py: the last loop header up to its branch.
That is the sub-step loop of ks_rk4_fused; in ks_rk4_lds it is only the copy of the new state and in
ks_reward_rows_kernel a tail loop, so for these two the loop columns say nothing about the arithmetic and (b) rests on the
register, scratch and spill counts.

  (a) the functions whose mangled names start with _ZN2ks: the same names in both
  (b) every ks_rk4_fused / ks_rk4_lds / ks_reward_rows_kernel: VGPRs, SGPRs, scratch bytes and spills not above the
      baseline's; in the loop the histogram of v_* and ds_* opcodes equal and the issued instructions not more
  (c) every fast-mode ks_rk4_fused with P >= 2: the loop's instruction sequence identical once labels and scalar
      register numbers are normalised

usage: tools/ks_isa_diff.py BASELINE.s CANDIDATE.s > profiles/NAME.txt   (exit status 1 if a check fails)"""
import collections
import re
import sys


def parse(path):
    lines = open(path).read().splitlines()
    syms = {}
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN2ks\w+):", l)
        if m:
            syms[m.group(1)] = i
    return lines, syms


def resources(lines, sym):
    i = next(i for i, l in enumerate(lines) if l.strip() == f".amdhsa_kernel {sym}")
    blk = lines[i:next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])]
    get = lambda key: int(next(l.split()[-1] for l in blk if l.strip().startswith(key)))
    j = next(j for j, l in enumerate(lines) if l.split() == [".name:", sym])
    meta = dict(l.split() for l in lines[j:j + 12] if len(l.split()) == 2)
    return {"vgpr": get(".amdhsa_next_free_vgpr"), "sgpr": get(".amdhsa_next_free_sgpr"),
            "scratch": get(".amdhsa_private_segment_fixed_size"),
            "spill": int(meta[".vgpr_spill_count:"]) + int(meta[".sgpr_spill_count:"])}


def loop(lines, start):
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    heads = [i for i, l in enumerate(body) if "Loop Header" in l]
    lo = heads[-1]
    hi = next(i for i in range(lo, len(body)) if "s_cbranch" in body[i])
    out = []
    for l in body[lo + 1:hi + 1]:
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    return out


def normalise(ins):
    t = re.sub(r"\.?LBB\d+_\d+", "L", ins)
    t = re.sub(r"s\[\d+:\d+\]", "s[]", t)
    return re.sub(r"\bs\d+\b", "s", t)


def main():
    (bl, bs), (cl, cs) = parse(sys.argv[1]), parse(sys.argv[2])
    ok = True
    print("device assembly of csrc/ks_kernels.hip, hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -S "
          "--cuda-device-only: baseline -> candidate; loop = the last loop header of a kernel up to its branch "
          "(tools/ks_isa_mix.py): the sub-step loop of ks_rk4_fused, but in ks_rk4_lds only the copy of the new state and in "
          "ks_reward_rows_kernel a tail loop -- for these two the loop columns do not cover the arithmetic")
    print(f"(a) _ZN2ks functions: baseline {len(bs)}, candidate {len(cs)}, missing {sorted(set(bs) - set(cs))}, "
          f"new {sorted(set(cs) - set(bs))}")
    ok &= set(bs) == set(cs)
    kernels = [s for s in bs if re.match(r"_ZN2ks(12ks_rk4_fused|10ks_rk4_lds|21ks_reward_rows_kernel)", s) and s in cs]
    print(f"(b), (c) {len(kernels)} kernels; columns: VGPR SGPR scratch spills | loop: issued, VALU, LDS  (baseline -> candidate)")
    n_c = n_c_ok = 0
    for sym in sorted(kernels):
        rb, rc = resources(bl, sym), resources(cl, sym)
        lb, lc = loop(bl, bs[sym]), loop(cl, cs[sym])
        hist = lambda ins: collections.Counter(i.split()[0] for i in ins if i.startswith(("v_", "ds_")))
        hb, hc = hist(lb), hist(lc)
        b_ok = all(rc[k] <= rb[k] for k in rb) and hb == hc and len(lc) <= len(lb)
        verdict = "(b) ok" if b_ok else "(b) FAIL"
        m = re.match(r"_ZN2ks12ks_rk4_fusedILi(\d+)ELi\d+ELi\d+ELb0E", sym)
        if m and int(m.group(1)) >= 2:
            n_c += 1
            same = [normalise(i) for i in lb] == [normalise(i) for i in lc]
            n_c_ok += same
            verdict += ", (c) identical" if same else ", (c) FAIL"
            ok &= same
        ok &= b_ok
        cnt = lambda ins, p: sum(i.startswith(p) for i in ins)
        print(f"{sym}\n    {rb['vgpr']}->{rc['vgpr']} {rb['sgpr']}->{rc['sgpr']} {rb['scratch']}->{rc['scratch']} "
              f"{rb['spill']}->{rc['spill']} | {len(lb)}->{len(lc)}, {cnt(lb, 'v_')}->{cnt(lc, 'v_')}, "
              f"{cnt(lb, 'ds_')}->{cnt(lc, 'ds_')}  {verdict}")
        if hb != hc:
            print("    histogram differs:", {k: (hb[k], hc[k]) for k in set(hb) | set(hc) if hb[k] != hc[k]})
    print(f"(c) fast-mode ks_rk4_fused with P >= 2: {n_c_ok} of {n_c} loops identical")
    print("all checks hold" if ok else "A CHECK FAILS")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
