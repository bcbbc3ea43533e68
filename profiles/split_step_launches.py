"""Kernel means of one `rocprofv3 --kernel-trace` run of the bench command, with the launches of the step kernel split into
"the launch right after a list build" and "every other launch" (the first one carries what a rebuild leaves to it).
usage: split_step_launches.py X_kernel_trace.csv   ->  one JSON object {kernel: {launches, mean_us}}"""
import csv
import json
import re
import sys

WATCH = ("k_permute", "k_permute_v", "k_scan_local4", "k_scan_add4", "k_scan_local", "k_scan_add", "k_scatter", "k_sort_cells", "k_wrap_bin",
         "k_bond_table", "k_build_neigh", "k_step")
rows = []
for r in csv.DictReader(open(sys.argv[1])):
    m = re.search(r"\b(k_[a-z0-9_]+)", r["Kernel_Name"])
    if m:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1), r["Kernel_Name"]))
rows.sort()
acc = {}


def add(name, ns):
    a = acc.setdefault(name, [0, 0])
    a[0] += 1
    a[1] += ns


after_build = False
for t0, t1, name, full in rows:
    if name not in WATCH:
        continue
    add(name, t1 - t0)
    if name == "k_build_neigh":
        after_build = True
    elif name == "k_step":
        add("k_step_after_build" if after_build else "k_step_plain", t1 - t0)
        head = full.split("(")[0].rstrip()          # the eleventh template argument: velocities handed over by a rebuild
        if head.endswith("true>") and head.count(",") == 10:
            add("k_step_velocity_hand_over", t1 - t0)
        after_build = False
print(json.dumps({k: {"launches": n, "mean_us": round(ns / n / 1000.0, 2)} for k, (n, ns) in acc.items()}, indent=1))
