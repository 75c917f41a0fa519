#!/usr/bin/env python3
"""The kernel launches of a rocprofv3 --kernel-trace run in dispatch order, one per line (kernel, grid, workgroup,
LDS, scratch): two builds that launch the same work print the same list.
    python scripts/launch_list.py <..._kernel_trace.csv> [step]
With `step`, only the last training step: after the next-to-last adamw_update_kernel up to the last one."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
if len(sys.argv) > 2:
    ends = [i for i, r in enumerate(rows) if "adamw_update_kernel" in r["Kernel_Name"]]
    rows = rows[ends[-2] + 1: ends[-1] + 1]
for r in rows:
    grid = ",".join(r["Grid_Size_" + a] for a in "XYZ")
    wg = ",".join(r["Workgroup_Size_" + a] for a in "XYZ")
    print(f'{r["Kernel_Name"]} grid=({grid}) wg=({wg}) lds={r["LDS_Block_Size"]} scratch={r["Scratch_Size"]}')
