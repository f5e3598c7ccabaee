#!/usr/bin/env python3
"""The VALU-issue roofline of A1 (cape_cell_moments_kernel) from the ISA of the binary that ships -- VERDICT r4 item 3.

A1 moves 1.0001 x its algorithmic bytes at ~0.49 of the HBM peak: it is bound by the ONE VALU port of a SIMD, not by memory.
This script makes that number reproducible instead of prose:

  1. compiles csrc/cape_cell_moments.hip to gfx950 assembly with the Makefile's flags (hipcc -S, no GPU needed);
  2. cuts the kernel (the FUSED lane-per-cell instance, the one a 640x480 batch runs) into its regions -- prologue, a trip of each
     of the two row loops, row 10 with the horizontal scan, the tail up to the aux record's store, and "fit + edges + stores":
     the cell's plane fit, the barrier, the edge predicates and the stores behind it -- and classifies every vector instruction by the issue cost MEASURED on gfx950
     (csrc/microbench/valu_rates.hip, profiles/r02_valu_rates.txt): f64-rate (v_*_f64, conversions from / to f64),
     double-rate (v_mul/add/sub_f32, v_add/sub_u32, v_and_b32, v_mov_b32: ~2.3 cycles), every other vector op (~4.3 cycles);
  3. prices one launch: instructions per wave x waves per SIMD x ns per wave-instruction;
  4. cross-checks the static count against the dynamic one of a rocprofv3 --pmc SQ_INSTS_VALU pass on the same binary
     (profiles/pmc_sq.sh), when its csv is given, and prices the dynamic count (every wave runs every region once, so the two
     differ only by the f64 form of the scan steps, which is listed apart and not run on the benchmark's frames -- and by the
     fit region, whose branches depend on the cells: it is LISTED once, every loop body and both sides of every branch, the in-order
     redo included, so only the counter pass says what a launch runs of it).

usage: valu_issue.py [--pmc profiles/r05_pmc_sq_insts.csv] [--frames 4096] [--out profiles/valu_issue.json]
bench.py reads the json (like profiles/traffic.json) and puts `roofline.valu_issue` in its line, with
frac_of_issue_floor = floor_ms / the launch time measured by that run."""
import argparse
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-d-slam_amd", "csrc")

# ns per wave-instruction per SIMD, profiles/r02_valu_rates.txt (valu_rates.exe on MI355X; 2.4 GHz shader clock)
RATE_NS = {"f64": 1.95, "other": 1.85, "double_rate": 0.95}
DOUBLE_RATE = {"v_mul_f32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_mov_b32"}


def classify(op):
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if "f64" in base or base.endswith("_b64") and base.startswith("v_mov"):
        return "f64"
    if base in DOUBLE_RATE:
        return "double_rate"
    return "other"


def kernel_regions(asm_lines, symbol):
    """[(region name, [opcodes])] of the lane-per-cell kernel: prologue, one trip of the first row loop (rows 0..9), row 10 with the
    horizontal scan, one trip of the second row loop (rows 11..18), tail (row 19, guard, the aux record's 16-B store) and what
    follows it: the fit, the barrier, the edge predicates and the stores of the fused instance (the five stores of the sums in the
    split one).  A loop is a backward branch; the row loops are the first two, every later one belongs to the fit.  (The aux
    record needs the count and the z range but none of the sums, so the compiler sinks row 19's f64 adds behind its store: they are
    listed with the fit.)
    The f64 form of a scan step sits behind an `s_cbranch_vccz` that skips it unless a lane of the wave is unsure of its f32
    verdict (which the benchmark's frames never are: the counter pass agrees with the count without it), so the instructions
    between such a branch and its target are left out and listed on their own as `redo_listed`."""
    start = next(i for i, ln in enumerate(asm_lines) if ln.startswith(symbol + ":"))
    end = next(i for i in range(start, len(asm_lines)) if "s_endpgm" in asm_lines[i])
    body = asm_lines[start + 1:end + 1]
    label_at = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    loops = []
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and label_at.get(m.group(1), len(body)) < i:
            loops.append((label_at[m.group(1)], i))
    loops.sort()
    assert len(loops) >= 2, "two row loops"
    redo = []

    def ops(lo, hi):
        out, skip_to = [], None
        for ln in body[lo:hi]:
            if skip_to is not None:
                if ln.startswith(skip_to + ":"):
                    skip_to = None
                else:
                    m = re.match(r"\s+([vs]_\w+)", ln)
                    if m:
                        redo.append(m.group(1))
                    continue
            m = re.match(r"\s+([vs]_\w+|ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)", ln)
            if m:
                out.append(m.group(1))
                v = re.match(r"\s+s_cbranch_vccz\s+(\.LBB\d+_\d+)", ln)
                if v:
                    skip_to = v.group(1)
        return out

    (h1, e1), (h2, e2) = loops[:2]
    aux = next(i for i in range(e2 + 1, len(body)) if "global_store_dwordx4" in body[i])
    regions = [("prologue", ops(0, h1)), ("loop_rows_0_9", ops(h1, e1 + 1)), ("row_10", ops(e1 + 1, h2)), ("loop_rows_11_18", ops(h2, e2 + 1)),
               ("tail", ops(e2 + 1, aux + 1)), ("fit_edges_writes", ops(aux + 1, len(body)))]
    return regions + [("redo_listed", redo)]


def count(ops):
    c = {"f64": 0, "double_rate": 0, "other": 0, "salu": 0, "lds": 0, "vmem": 0}
    for op in ops:
        if op.startswith("v_"):
            c[classify(op)] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["vmem"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pmc", default="")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valu_issue.json"))
    args = ap.parse_args()

    asm_path = "/tmp/cape_cell_moments.gfx950.s"
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-o", asm_path, os.path.join(CSRC, "cape_cell_moments.hip")],
                          stderr=subprocess.DEVNULL)
    asm = open(asm_path).read().splitlines()
    # launch shape (cape_cell_moments.hip, the lane-per-cell instance): a wave = 64 consecutive cells of a frame, a lane = one cell of
    # 20 rows x 20 pixels: ten trips of the first row loop, row 10, eight trips of the second, row 19 in the tail
    cell = 20
    cells = (args.height // cell) * (args.width // cell)
    waves_per_launch = args.frames * ((cells + 63) // 64)
    out = {"kernel": "cape_cell_moments_kernel", "frames_per_launch": args.frames, "width": args.width, "height": args.height,
           "waves_per_launch": waves_per_launch, "simds": args.simds, "rate_ns_per_wave_instruction": RATE_NS,
           "rates_from": "profiles/r02_valu_rates.txt (csrc/microbench/valu_rates.hip on MI355X)", "variants": {}}
    for variant, symbol in (("f32", "_ZN4cape24cape_cell_moments_kernelILb0ELb1EEEvNS_12StageAParamsEi"),
                            ("u16", "_ZN4cape24cape_cell_moments_kernelILb1ELb1EEEvNS_12StageAParamsEi")):
        regs = dict(kernel_regions(asm, symbol))
        c = {k: count(v) for k, v in regs.items()}
        weights = {"prologue": 1, "loop_rows_0_9": cell // 2, "row_10": 1, "loop_rows_11_18": cell // 2 - 2, "tail": 1, "fit_edges_writes": 1}
        per_wave = {k: sum(c[r][k] * w for r, w in weights.items()) for k in ("f64", "double_rate", "other", "salu", "lds", "vmem")}
        static_valu = per_wave["f64"] + per_wave["double_rate"] + per_wave["other"]
        v = {"static_per_wave": {"all_rows": per_wave, "per_region": {r: c[r] for r in weights}, "redo_listed_not_run": c["redo_listed"],
                                 "per_20_pixels_row_trip": c["loop_rows_0_9"]}}
        valu = static_valu
        if args.pmc:
            for row in csv.DictReader(open(args.pmc)):
                if ("cell_moments_kernel<false, true>" if variant == "f32" else "cell_moments_kernel<true, true>") in row["kernel"] and row["counter"] == "SQ_INSTS_VALU":
                    dyn = float(row["avg_value"])
                    v["pmc"] = {"SQ_INSTS_VALU_per_launch": dyn, "per_wave": dyn / waves_per_launch, "static_per_wave": static_valu,
                                "source": os.path.relpath(args.pmc, ROOT)}
                    valu = dyn / waves_per_launch
        # every wave runs every region once (no block belongs to a subset of the waves), so the static count IS the dynamic one up
        # to the row-dependent selects; a counter pass replaces it where given, priced at the static mix
        mix = {k: per_wave[k] / max(1, static_valu) for k in RATE_NS}
        per_wave_ns = valu * sum(mix[k] * RATE_NS[k] for k in RATE_NS)
        floor_ms = per_wave_ns * waves_per_launch / args.simds * 1e-6
        f64_ns = valu * mix["f64"] * RATE_NS["f64"]
        v.update({"valu_per_wave": valu, "issue_ns_per_wave": per_wave_ns, "floor_ms": floor_ms,
                  "f64_rate_share_of_floor": f64_ns / per_wave_ns,
                  "f64_rate_insts_per_launch": valu * mix["f64"] * waves_per_launch,
                  "other_insts_per_launch": valu * (1.0 - mix["f64"]) * waves_per_launch})
        out["variants"][variant] = v
        print(f"{variant}: per wave (64 cells) f64-rate {per_wave['f64']}, double-rate {per_wave['double_rate']}, other {per_wave['other']} "
              f"= {static_valu} listed, {valu:.0f} priced ({valu / 5:.0f} per 80 pixels per lane); issue floor {floor_ms:.3f} ms per {args.frames} frames "
              f"({100 * f64_ns / per_wave_ns:.0f} % of it the f64-rate instructions the reference's operand types dictate)", file=sys.stderr)
    json.dump(out, open(args.out, "w"), indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
