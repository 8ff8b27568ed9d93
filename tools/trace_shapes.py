#!/usr/bin/env python
"""Per-(kernel, grid) table of a rocprofv3 --kernel-trace CSV: launches, mean and total time -- the per-shape view the
--stats table (one row per kernel name) does not give (developer tool).

    python tools/trace_shapes.py OUT_DIR [--steps N] [--top K]

--steps N divides counts and totals by N traced steps."""
import csv
import glob
import os
import re
import sys
from collections import defaultdict


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)[:72]


def main():
    out = sys.argv[1]
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 1
    top = int(sys.argv[sys.argv.index("--top") + 1]) if "--top" in sys.argv else 60
    files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {out}")
    rows = defaultdict(lambda: [0, 0.0])
    for f in files:
        for r in csv.DictReader(open(f)):
            key = (short(r["Kernel_Name"]), int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])),
                   int(r.get("Grid_Size_Y", 1)) // max(1, int(r.get("Workgroup_Size_Y", 1))), int(r["Workgroup_Size_X"]))
            e = rows[key]
            e[0] += 1
            e[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    total = sum(e[1] for e in rows.values())
    print(f"{'kernel':72s} {'groups':>12s} {'wg':>5s} {'calls/step':>10s} {'avg us':>9s} {'ms/step':>9s}")
    for key, e in sorted(rows.items(), key=lambda kv: -kv[1][1])[:top]:
        print(f"{key[0]:72s} {str(key[1]) + 'x' + str(key[2]):>12s} {key[3]:5d} {e[0] / steps:10.1f} {e[1] / e[0] * 1e3:9.1f} {e[1] / steps:9.3f}")
    print(f"{'all kernels':72s} {'':>12s} {'':>5s} {sum(e[0] for e in rows.values()) / steps:10.1f} {'':>9s} {total / steps:9.3f}")


if __name__ == "__main__":
    main()
