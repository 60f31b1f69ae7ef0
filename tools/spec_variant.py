"""One line per profiler run of tools/spec_variant.sh: the broadphase and narrowphase kernels' time (trace) or the broadphase's
instructions per wave (pmc), with bench.py's value and parity of that run."""
import csv
import json
import sys
from collections import defaultdict

tag, mode, path, log, opts = sys.argv[1:6]
value = parity = None
for line in open(log, errors="replace"):
    if line.startswith("{"):
        d = json.loads(line)
        value, parity = d.get("value"), d.get("parity_vs_oracle")
head = f"{tag:28s} [{opts or 'no options'}]"
if mode == "trace":
    parts = []
    for r in csv.DictReader(open(path)):
        name = r["Name"].split("(")[0]
        if "k_broad" in name or "k_narrow" in name:
            parts.append(f"{name.split('::')[-1].split('<')[0]} {r['Calls']} calls {float(r['AverageNs']) / 1e3:.2f} / {float(r['MinNs']) / 1e3:.2f} / {float(r['MaxNs']) / 1e3:.2f}")
    print(head, "  ".join(parts), f"value(under the profiler) {value:.4g}" if value else "", str(parity)[:40])
else:
    v = defaultdict(lambda: defaultdict(list))
    grid = {}
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"].split("(")[0]
        if "k_broad" in k:
            v[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
            grid[k] = int(r["Grid_Size"])
    for k, c in v.items():
        waves = (grid[k] + 63) // 64
        m = lambda n: sum(c[n]) / len(c[n]) / waves if c[n] else float("nan")
        print(head, f"{k.split('::')[-1]}: {waves} waves (SQ_WAVES {m('SQ_WAVES') * waves:.0f}), per wave VALU {m('SQ_INSTS_VALU'):.1f} SALU {m('SQ_INSTS_SALU'):.1f} LDS {m('SQ_INSTS_LDS'):.1f}", str(parity)[:40])
