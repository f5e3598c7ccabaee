#!/usr/bin/env python3
"""VALU instructions per wave of A1 (cape_cell_moments_kernel) by region and by issue class, from the gfx950 ISA.

valu_issue.py prices the kernel as row loop + one lump "tail"; this cuts finer, to show where the instructions that are not
the per-pixel arithmetic sit (profiles/a1_instruction_inventory.txt):

  prologue          kernel entry up to the first depth load (index math, the column factors)
  first trips       the peeled first trip (two groups of two rows), up to the loop header
  loop trip         one rolled trip of the row loop = 4 rows = 4 float4 per lane (x3 per wave at 20 rows)
  last trips        the peeled last trip
  partial store     the per-thread sums into LDS, up to the barrier
  reduce wave       5 partials -> one cell, stores of cell_sums (runs on wave 4 only)
  scan waves        the continuity cross scans up to the second cross-lane read (waves 0..3)
  scan f64 redo     the f64 scan that runs only when a wave's f32 scan could not decide a step (absent before the diet)
  aux store         exactness guard + CellAux store (16 lanes of waves 0..3)

usage: a1_inventory.py [--asm listing.s]     (default: compile the working tree's csrc/cape_cell_moments.hip with the Makefile's flags)
Classes and prices are valu_issue.py's (profiles/r02_valu_rates.txt)."""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from valu_issue import CSRC, RATE_NS, classify  # noqa: E402

SYMBOLS = (("f32", "_ZN4cape24cape_cell_moments_kernelILb0EEEvNS_12StageAParamsE"),
           ("u16", "_ZN4cape24cape_cell_moments_kernelILb1EEEvNS_12StageAParamsE"))
ORDER = ("prologue", "first trips", "loop trip", "last trips", "partial store", "reduce wave", "scan waves", "scan f64 redo", "aux store")
# how many times a wave runs the region, averaged over the workgroup's five waves
WEIGHT = {"prologue": 1, "first trips": 1, "loop trip": 3, "last trips": 1, "partial store": 1, "reduce wave": 0.2, "scan waves": 0.8,
          "scan f64 redo": 0.0, "aux store": 0.8}


def find(body, lo, pred):
    return next(i for i in range(lo, len(body)) if pred(body[i]))


def regions(asm, symbol):
    start = next(i for i, ln in enumerate(asm) if ln.startswith(symbol + ":"))
    end = find(asm, start, lambda ln: "s_endpgm" in ln)
    body = asm[start + 1:end + 1]
    is_depth_load = lambda ln: re.search(r"global_load_dwordx[24] .* nt$", ln.rstrip()) is not None  # noqa: E731
    first_load = find(body, 0, is_depth_load)
    head = find(body, 0, lambda ln: "Loop Header" in ln)
    label = body[head].split(":")[0]
    loop_end = find(body, head, lambda ln: re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", ln) is not None)
    skip = re.search(r"s_cbranch_execz\s+(\S+)", body[find(body, 0, lambda ln: "s_cbranch_execz" in ln)]).group(1)
    join = find(body, loop_end, lambda ln: ln.startswith(skip + ":"))
    barrier = find(body, join, lambda ln: "s_barrier" in ln)
    out = {"prologue": body[:first_load], "first trips": body[first_load:head], "loop trip": body[head:loop_end + 1],
           "last trips": body[loop_end + 1:join], "partial store": body[join:barrier + 1]}
    # behind the barrier: two arms, split at the target of the first branch
    br = find(body, barrier, lambda ln: re.search(r"s_cbranch_\w+\s+\.LBB", ln) is not None)
    target = re.search(r"(\.LBB\w+)", body[br]).group(1)
    split = find(body, br, lambda ln: ln.startswith(target + ":"))
    arms = [body[barrier + 1:split], body[split:]]
    reduce_arm = next(a for a in arms if any("global_store_dwordx2" in ln for ln in a))
    scan_arm = next(a for a in arms if a is not reduce_arm)
    out["reduce wave"] = reduce_arm
    last_perm = max(i for i, ln in enumerate(scan_arm) if "ds_bpermute_b32" in ln)
    scan, redo = scan_arm[:last_perm + 1], []
    for i, ln in enumerate(scan):
        m = re.search(r"s_cbranch_vccz\s+(\.LBB\w+)", ln)
        if m:
            j = find(scan, i, lambda x: x.startswith(m.group(1) + ":"))
            if any(re.search(r"v_cmp_\w+_f64", x) for x in scan[i:j]):
                scan, redo = scan[:i + 1] + scan[j:], scan[i + 1:j]
                break
    out["scan waves"], out["scan f64 redo"], out["aux store"] = scan, redo, scan_arm[last_perm + 1:]
    return out


def count(lines):
    c = {"f64": 0, "double_rate": 0, "other": 0}
    for ln in lines:
        m = re.match(r"\s+(v_\w+)", ln)
        if m:
            c[classify(m.group(1))] += 1
    return c


def inventory(asm):
    res = {}
    for variant, symbol in SYMBOLS:
        res[variant] = {name: count(lines) for name, lines in regions(asm, symbol).items()}
    return res


def priced(c):
    return sum(c[k] * RATE_NS[k] for k in RATE_NS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="")
    args = ap.parse_args()
    path = args.asm
    if not path:
        path = "/tmp/cape_cell_moments.inventory.s"
        flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-o", path, os.path.join(CSRC, "cape_cell_moments.hip")],
                              stderr=subprocess.DEVNULL)
    inv = inventory(open(path).read().splitlines())
    for variant, regs in inv.items():
        print(f"{variant}   VALU instructions as listed                      f64-rate  double-rate  other   total   runs/wave   issue ns/wave")
        tot_n = tot_ns = 0.0
        for name in ORDER:
            c = regs[name]
            n = c["f64"] + c["double_rate"] + c["other"]
            ns = priced(c) * WEIGHT[name]
            tot_n += n * WEIGHT[name]
            tot_ns += ns
            print(f"  {name:<48} {c['f64']:8d} {c['double_rate']:12d} {c['other']:6d} {n:7d} {WEIGHT[name]:11.1f} {ns:15.1f}")
        print(f"  {'per wave, weighted':<48} {'':8} {'':12} {'':6} {tot_n:7.0f} {'':11} {tot_ns:15.1f}")


if __name__ == "__main__":
    main()
