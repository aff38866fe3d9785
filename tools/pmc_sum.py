"""Counters of rocprofv3 --pmc runs per kernel: python tools/pmc_sum.py [--kernel=SUBSTRING] DIR...  (default: the inflate kernels).
A dispatch may have several rows per counter (one per instance); they are summed per dispatch, then averaged over the dispatches."""
import csv, glob, collections, sys
want = "inflate"
for d in sys.argv[1:]:
    if d.startswith("--kernel="):
        want = d.split("=", 1)[1]
        continue
    for f in glob.glob(d + "/*/*counter_collection.csv"):
        agg = collections.defaultdict(lambda: collections.defaultdict(float))
        for row in csv.DictReader(open(f)):
            agg[(row["Kernel_Name"].split("(")[0], row["Counter_Name"])][row.get("Dispatch_Id", "")] += float(row["Counter_Value"])
        for (k, c), per in sorted(agg.items()):
            v = list(per.values())
            if want in k: print("%-28s %-22s n=%d avg=%.4g max=%.4g" % (k[:28], c, len(v), sum(v)/len(v), max(v)))
