#!/usr/bin/env python3
"""Summarise rocprofv3 --pmc passes per kernel:
   python3 tools/pmc_summary.py gpurun_out/pmc_fetch gpurun_out/pmc_write [...] > profiles/rNN_pmc.json
Each directory is one pass (its own `rocprofv3 --pmc <counters> --kernel-trace --output-format csv`
run of the same command).  Per kernel family: launches, mean counter value per launch, and the
HBM traffic estimate the MI355X guide prescribes for gfx950: FETCH_SIZE counts 64 B per 128-B
request of a wide coalesced read, so read bytes <= 2 x FETCH_SIZE x 1024; WRITE_SIZE x 1024 is exact."""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict


def family(name):
    m = re.search(r"k_gemm_nt_sub<(\w+), (true|false), (\d)>", name)
    if m:
        return "k_gemm_nt_sub<%s,%s,%s-tile>" % (m.group(1), "lower" if m.group(2) == "true" else "rect", 32 * int(m.group(3)))
    m = re.search(r"k_gemm_nt_pers<(\w+), (true|false)(?:, \d+)?(?:, (?:true|false))?>", name)
    if m:
        return "k_gemm_nt_pers<%s,%s>" % (m.group(1), "lower" if m.group(2) == "true" else "rect")
    # the RBF Gram kernels: k_gram*<T, 0, ..> (COV = 0), k_rbf_gram*<T, ..> in profiles from before the COV parameter
    m = re.search(r"k_(?:rbf_)?gram_lower_wide<(\w+),(?: 0,)? (\d)>", name)      # round 5: the lower triangle in 64 x 128 tiles
    if m:
        return "k_rbf_gram<%s,symmetric,d=%s>" % (m.group(1), m.group(2))
    m = re.search(r"k_(?:rbf_)?gram<(\w+),(?: 0,)? (true|false), (\d)>", name)
    if m:
        return "k_rbf_gram<%s,%s,d=%s>" % (m.group(1), "symmetric" if m.group(2) == "true" else "cross", m.group(3))
    m = re.search(r"(k_\w+)<(\w+)", name)
    if m:
        return "%s<%s>" % (m.group(1), m.group(2))
    m = re.search(r"(k_\w+)", name)
    return m.group(1) if m else None


def main():
    out = defaultdict(lambda: defaultdict(list))
    for root in sys.argv[1:]:
        files = glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            raise SystemExit("no *counter_collection.csv under " + root)
        per_dispatch = defaultdict(float)
        names = {}
        with open(sorted(files)[-1]) as fh:
            for r in csv.DictReader(fh):
                key = (r["Dispatch_Id"], r["Counter_Name"])
                per_dispatch[key] += float(r["Counter_Value"])
                names[r["Dispatch_Id"]] = r["Kernel_Name"]
        for (disp, counter), value in per_dispatch.items():
            fam = family(names[disp])
            if fam:
                out[fam][counter].append(value)
    summary = {}
    for fam, counters in sorted(out.items()):
        rec = {}
        for counter, vals in counters.items():
            rec[counter] = dict(launches=len(vals), mean=sum(vals) / len(vals), max=max(vals), total=sum(vals))
        if "FETCH_SIZE" in rec and "WRITE_SIZE" in rec:
            rec["hbm_bytes_per_launch_upper"] = (2 * rec["FETCH_SIZE"]["mean"] + rec["WRITE_SIZE"]["mean"]) * 1024
            rec["hbm_write_bytes_per_launch"] = rec["WRITE_SIZE"]["mean"] * 1024
        summary[fam] = rec
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
