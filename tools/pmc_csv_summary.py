#!/usr/bin/env python3
"""Summarise a ``rocprofv3 --pmc ... --output-format csv`` run
(``*_counter_collection.csv``): per kernel, the counter totals per
dispatch, averaged over dispatches (the csv twin of pmc_summary.py, for
counter-only runs that write no rocpd database).

Usage: python tools/pmc_csv_summary.py <counter_collection.csv> [...] [--skip 3]
"""
import argparse
import collections
import csv
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--skip", type=int, default=0, help="drop each kernel's first N dispatches")
    a = ap.parse_args()
    for path in a.paths:
        per = collections.defaultdict(lambda: collections.defaultdict(float))
        with open(path) as f:
            for r in csv.DictReader(f):
                m = re.search(r"(k_[a-z0-9_]+)", r["Kernel_Name"])
                if m:
                    per[(m.group(1), int(r["Dispatch_Id"]))][r["Counter_Name"]] += float(r["Counter_Value"])
        byk = collections.defaultdict(list)
        for (k, _), cv in sorted(per.items()):
            byk[k].append(cv)
        print("##", path)
        for k, rows in byk.items():
            rows = rows[a.skip:]
            if rows:
                print(f"{k:24s} n={len(rows):4d}  " +
                      "  ".join(f"{c}={sum(r[c] for r in rows) / len(rows):.5g}" for c in sorted(rows[0])))


if __name__ == "__main__":
    main()
