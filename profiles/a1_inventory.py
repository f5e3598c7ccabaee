#!/usr/bin/env python3
"""VALU instructions per wave of A1 (cape_cell_moments_kernel, the lane-per-cell instance) by region and by issue class, from the
gfx950 ISA.  A wave is 64 cells, a lane sums one cell of 400 pixels, and every wave runs every region (no barrier, no block
that belongs to a subset of the waves); valu_issue.py cuts the regions, this prints them (profiles/a1_instruction_inventory.txt):

  prologue          kernel entry up to the first row loop: wave / cell index math, the 20 column factors, the descriptors, row 0's loads
  rows 0..9         one trip of the first row loop = one row = 20 pixels per lane + the vertical scan's step (x10)
  row 10            the peeled centre row: 20 pixels, the vertical step and the horizontal scan's 19 steps
  rows 11..18       one trip of the second row loop (x8)
  tail              row 19 (no loads, no step), the exactness guard, the stores of cell_aux and cell_sums
  scan f64 redo     the f64 form of the scan steps, run only for a step some lane of the wave cannot decide in f32 (weight 0)

usage: a1_inventory.py [--asm listing.s]     (default: compile the working tree's csrc/cape_cell_moments.hip with the Makefile's flags)
Classes and prices are valu_issue.py's (profiles/r02_valu_rates.txt)."""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from valu_issue import CSRC, RATE_NS, classify, kernel_regions  # noqa: E402

SYMBOLS = (("f32", "_ZN4cape24cape_cell_moments_kernelILb0ELb1EEEvNS_12StageAParamsEi"),
           ("u16", "_ZN4cape24cape_cell_moments_kernelILb1ELb1EEEvNS_12StageAParamsEi"))
NAMES = {"prologue": "prologue", "loop_rows_0_9": "rows 0..9, one trip", "row_10": "row 10", "loop_rows_11_18": "rows 11..18, one trip",
         "tail": "tail", "fit_edges_writes": "fit + edges + stores (listed once)", "redo_listed": "scan f64 redo"}
ORDER = tuple(NAMES)
# how many times a wave runs the region
WEIGHT = {"prologue": 1, "loop_rows_0_9": 10, "row_10": 1, "loop_rows_11_18": 8, "tail": 1, "fit_edges_writes": 1, "redo_listed": 0}


def count(ops):
    c = {"f64": 0, "double_rate": 0, "other": 0}
    for op in ops:
        if op.startswith("v_"):
            c[classify(op)] += 1
    return c


def inventory(asm):
    return {variant: {name: count(ops) for name, ops in kernel_regions(asm, symbol)} for variant, symbol in SYMBOLS}


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
            print(f"  {NAMES[name]:<48} {c['f64']:8d} {c['double_rate']:12d} {c['other']:6d} {n:7d} {WEIGHT[name]:11.1f} {ns:15.1f}")
        print(f"  {'per wave (64 cells), weighted':<48} {'':8} {'':12} {'':6} {tot_n:7.0f} {'':11} {tot_ns:15.1f}")
        print(f"  {'per 80 pixels per lane (the band instance: 2 790)':<48} {'':8} {'':12} {'':6} {tot_n / 5:7.0f} {'':11} {tot_ns / 5:15.1f}")


if __name__ == "__main__":
    main()
