"""Per-build counter means of a rocprofv3 --pmc pass (rocpd sqlite) over tools/split_pmc.py with AZ_BENCH_LIBS: every build's kernels carry
the same name, so the dispatches of each kernel name are taken in dispatch order and cut into one group per build (launches per build
and kernel = dispatches / builds).
usage: python tools/pmc_groups.py <db> <label,label,...> [kernel pattern, default %conv3x3%]"""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
labels = sys.argv[2].split(",")
pat = sys.argv[3] if len(sys.argv) > 3 else "%conv3x3%"
cols = [d[1] for d in db.execute("pragma table_info(counters_collection)")]
order = next((c for c in ("dispatch_id", "start", "id") if c in cols), None)
if order is None or "counter_name" not in cols or "kernel_name" not in cols:
    print("columns:", cols)
    sys.exit(1)
rows = {}
for kn, cn, o, v in db.execute(f"select kernel_name, counter_name, {order}, value from counters_collection where kernel_name like ? order by {order}", (pat,)):
    rows.setdefault((kn, cn), {}).setdefault(o, 0.0)
    rows[(kn, cn)][o] += v  # (a counter reported per instance or dimension: summed per dispatch)
for (kn, cn), d in sorted(rows.items()):
    vals = [d[o] for o in sorted(d)]
    if len(vals) % len(labels):
        print("  ", kn[:70], cn, f"{len(vals)} dispatches do not divide into {len(labels)} builds")
        continue
    per = len(vals) // len(labels)
    for i, lab in enumerate(labels):
        g = vals[i * per:(i + 1) * per]
        print("  ", f"{lab:14s}", kn[:70], cn, "n=%d" % len(g), "mean=%.6g min=%.6g max=%.6g" % (sum(g) / len(g), min(g), max(g)))
