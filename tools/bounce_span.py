"""Per-bounce launch durations of a rocprofv3 kernel trace of the bench (fixed-spp traced configs), the
way tools/tail_span.py reduces the tail.  Per stream a batch is k_bounce<FIRST> (bounce 0), k_bounce
(bounces 1 .. T-1), k_tail, k_accumulate.  Reports, as medians over the trace's batches: the duration
of the launch at every bounce below the tail, the tail's duration, the batch's span, and the span of
the heavy phase (bounce 0's start to the end of bounce HEAVY, default 7) of a batch and of a batch pair
(the k-th batches of the two streams, which run side by side: first start to last end).
Launches are numbered in launch order.  With the fused first launch (OM_WF_FUSE_B1 = 1, the default)
entry 0 of `bounce_us` is bounces 0 and 1 together and entry k >= 1 is bounce k + 1 (pass FUSED = 1 and
the output says so in `launch_bounces`; HEAVY stays a launch index, so the heavy phase that ended with
bounce 7 is HEAVY = 6 there); a trace of a library built with OM_WF_FUSE_B1 = 0 reads as before.
    python tools/bounce_span.py run_kernel_trace.csv[.gz] [HEAVY [FUSED]]   -> one JSON line"""
import csv
import gzip
import json
import re
import statistics
import sys

path = sys.argv[1]
HEAVY = int(sys.argv[2]) if len(sys.argv) > 2 else 7
FUSED = len(sys.argv) > 3 and sys.argv[3] == "1"
f = gzip.open(path, "rt") if path.endswith(".gz") else open(path)
first = re.compile(r"k_bounce<\d+, \w+, \w+, true")
streams = {}
for r in csv.DictReader(f):
    n = r["Kernel_Name"]
    if "k_bounce<" in n or "k_tail<" in n:
        kind = "tail" if "k_tail<" in n else "first" if first.search(n) else "bounce"
        streams.setdefault((r["Queue_Id"], r["Stream_Id"]), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
per_stream = []
for rows in streams.values():
    rows.sort()
    batches, cur = [], None
    for s, e, kind in rows:
        if kind == "first":
            cur = [(s, e)]
        elif cur is not None and kind == "bounce":
            cur.append((s, e))
        elif cur is not None and kind == "tail":
            cur.append((s, e))
            batches.append(cur)
            cur = None
    if batches:
        per_stream.append(batches)
med = statistics.median
allb = [b for bs in per_stream for b in bs]
depth = min(len(b) for b in allb) - 1                      # launches below the tail
us = lambda ns: round(ns / 1e3, 1)
out = {"trace": path, "streams": len(per_stream), "batches": len(allb), "tail_from_bounce": depth,
       "bounce_us": [us(med(b[k][1] - b[k][0] for b in allb)) for k in range(depth)],
       "tail_us": us(med(b[-1][1] - b[-1][0] for b in allb)),
       "batch_span_us": us(med(b[-1][1] - b[0][0] for b in allb))}
if FUSED:
    out["launch_bounces"] = ["0+1"] + [str(k + 1) for k in range(1, depth)]
h = min(HEAVY, depth - 1)
out[f"heavy_span_bounce0_to_{h}_us"] = us(med(b[h][1] - b[0][0] for b in allb))
if len(per_stream) == 2:
    pairs = list(zip(*per_stream))
    out[f"pair_heavy_span_bounce0_to_{h}_us"] = us(med(max(b[h][1] for b in p) - min(b[0][0] for b in p) for p in pairs))
    out["pair_span_us"] = us(med(max(b[-1][1] for b in p) - min(b[0][0] for b in p) for p in pairs))
print(json.dumps(out))
