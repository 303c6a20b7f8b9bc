"""Which shipped kernel instantiations a profiled run launched: reads the kernel-stats CSV(s) of a
`rocprofv3 --kernel-trace --stats` run and prints the instantiations of profiles/kernel_isa_baseline.json that never
launched, then a count.  Names are normalised as tools/kernel_isa_counts.demangle does: strip "void bkd::", cut at "(".

usage: python scripts/kernel_coverage.py KERNEL_STATS.csv [more.csv ...]     (exit status 1 when one never launched)
"""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")


def normalise(name):
    return re.sub(r"^void bkd::", "", name.strip()).split("(")[0].strip()


def launched(paths):
    """{normalised kernel name: calls} over the stats CSVs (column "Name", calls from "Calls" where present)"""
    out = {}
    for p in paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name")
                if not name:
                    continue
                k = normalise(name)
                out[k] = out.get(k, 0) + int(float(row.get("Calls") or 1))
    return out


def main(argv):
    if not argv:
        print(__doc__.strip())
        return 2
    with open(BASELINE) as f:
        kernels = sorted(json.load(f)["kernels"])
    seen = launched(argv)
    never = [k for k in kernels if k not in seen]
    for k in never:
        print(f"never launched: {k}")
    print(f"{len(kernels) - len(never)} of {len(kernels)} baseline instantiations launched; {len(never)} never launched")
    return 1 if never else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
