#!/usr/bin/env python3
"""SQ_INSTS_VALU (or any counter) per launch of the frame's k_pool kernel from a counters-only rocprofv3 --pmc pass:

    python tools/pmc_kpool.py OUTPUT_DIR [TAG]

Prints every launch of the kernel with the largest sum (the fast kernel; the adopting EXACT launch is small) and the mean
and spread over the launches after the first (the warm-up frame).
"""
import collections, csv, glob, sys
out, tag = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
per = collections.defaultdict(lambda: collections.defaultdict(lambda: collections.defaultdict(float)))
for f in glob.glob(out + "/**/*_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_pool<" in r["Kernel_Name"]:
            per[r["Kernel_Name"]][r["Counter_Name"]][int(r["Dispatch_Id"])] += float(r["Counter_Value"])
for c in sorted({c for k in per for c in per[k]}):
    best = max((k for k in per if c in per[k]), key=lambda k: sum(per[k][c].values()))
    v = [per[best][c][d] for d in sorted(per[best][c])][1:]
    mean = sum(v) / len(v)
    print("%-8s %s per k_pool launch: mean %.5e  min %.5e  max %.5e  spread %.3f %%  (%d launches: %s)" % (
        tag, c, mean, min(v), max(v), 100.0 * (max(v) - min(v)) / mean, len(v), " ".join("%.5e" % x for x in v)))
