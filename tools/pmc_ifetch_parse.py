"""Per-kernel instruction-fetch figures from the two rocprofv3 --pmc passes of
tools/pmc_ifetch.sh: every counter summed over a dispatch's rows (all XCDs / SEs /
instances) and averaged over the kernel's dispatches, plus the derived ratios

    icache_miss_rate   = SQC_ICACHE_MISSES / SQC_ICACHE_REQ
    wait_inst_fraction = SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES   (both in quad-cycles: the profiler's own ratio)

    python tools/pmc_ifetch_parse.py <dir with SQ/ and SQC/> <out.json>
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

KEEP = ("rcab_bwd_kernel", "conv64_kernel<48, 8, 8>", "wgrad48_kernel")


def collect(root):
    """kernel -> counter -> [per-dispatch sums]"""
    out = defaultdict(lambda: defaultdict(list))
    for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        per = defaultdict(lambda: defaultdict(float))
        names = {}
        for r in csv.DictReader(open(f)):
            key = r.get("Dispatch_Id") or r.get("Correlation_Id")
            per[key][r["Counter_Name"]] += float(r["Counter_Value"])
            names[key] = r["Kernel_Name"]
        for key, cs in per.items():
            for c, v in cs.items():
                out[names[key]][c].append(v)
    return out


def short(name):
    i = name.find("srmi::")
    name = name[i + 6:] if i >= 0 else name
    return name.split("(")[0].strip()


def main(root, out):
    res = {}
    for k, cs in collect(root).items():
        if not any(s.replace(" ", "") in k.replace(" ", "") for s in KEEP):
            continue
        rec = {c: round(sum(v) / len(v), 1) for c, v in sorted(cs.items())}
        rec["dispatches"] = max(len(v) for v in cs.values())
        if rec.get("SQC_ICACHE_REQ"):
            rec["icache_miss_rate"] = round(rec.get("SQC_ICACHE_MISSES", 0.0) / rec["SQC_ICACHE_REQ"], 5)
        if rec.get("SQ_WAVE_CYCLES"):
            rec["wait_inst_fraction"] = round(rec.get("SQ_WAIT_INST_ANY", 0.0) / rec["SQ_WAVE_CYCLES"], 4)
        res[short(k)] = rec
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
