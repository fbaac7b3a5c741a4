"""median and quartiles of the duration per kernel of a rocprofv3 kernel trace (csv), as JSON:
python tools/kernel_quartiles.py trace.csv [--min-us X] [name substring ...]     (--min-us: only the launches longer than X, e.g. 8 for the useful ones inside PCG)"""
import collections
import csv
import json
import sys

import numpy as np


def main(argv):
    min_us = 0.0
    if "--min-us" in argv:
        i = argv.index("--min-us"); min_us = float(argv[i + 1]); del argv[i:i + 2]
    path, picks = argv[0], argv[1:]
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("poro::", "").split("(")[0]
        if picks and not any(p in k for p in picks):
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if us > min_us:
            acc[k].append(us)
    out = {}
    for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        out[k] = {"launches": len(v), "median_us": round(float(med), 2), "q1_us": round(float(q1), 2), "q3_us": round(float(q3), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "total_us": round(sum(v), 1)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
