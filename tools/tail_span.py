"""The light phase of a batch from a rocprofv3 kernel trace of the bench (fixed-spp traced configs).
Per stream a batch is k_bounce<FIRST> (bounce 0), k_bounce (bounces 1 .. T-1), k_tail, k_accumulate.
Reports, as medians over the trace's batches: the span from the start of the first launch at
bounce >= FROM (default 8; the tail itself when T <= FROM) to the tail's end, the tail's duration,
the batch's span, and the bounce-family launches per batch.
    python tools/tail_span.py run_kernel_trace.csv[.gz] [FROM]   -> one JSON line"""
import csv
import gzip
import json
import re
import statistics
import sys

path = sys.argv[1]
FROM = int(sys.argv[2]) if len(sys.argv) > 2 else 8
f = gzip.open(path, "rt") if path.endswith(".gz") else open(path)
first = re.compile(r"k_bounce<\d+, \w+, \w+, true")
streams = {}
for r in csv.DictReader(f):
    n = r["Kernel_Name"]
    if "k_bounce<" in n or "k_tail<" in n or "k_accumulate<" in n:
        kind = "tail" if "k_tail<" in n else "acc" if "k_accumulate<" in n else "first" if first.search(n) else "bounce"
        streams.setdefault((r["Queue_Id"], r["Stream_Id"]), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
spans, tails, batches, launches, tail_at = [], [], [], [], []
for rows in streams.values():
    rows.sort()
    cur = None
    for s, e, kind in rows:
        if kind == "first":
            cur = [(s, e)]
        elif cur is not None and kind == "bounce":
            cur.append((s, e))
        elif cur is not None and kind == "tail":
            t = len(cur)                                   # the tail's first bounce
            start = cur[FROM][0] if t > FROM else s
            spans.append((e - start) / 1e3)
            tails.append((e - s) / 1e3)
            batches.append((e - cur[0][0]) / 1e3)
            launches.append(t + 1)
            tail_at.append(t)
            cur = None
med = statistics.median
print(json.dumps({"trace": path, "batches": len(spans), "tail_from_bounce": med(tail_at), "launches_per_batch": med(launches),
                  f"span_bounce{FROM}_to_tail_end_us": round(med(spans), 1), "tail_us": round(med(tails), 1),
                  "tail_us_min_max": [round(min(tails), 1), round(max(tails), 1)], "batch_span_us": round(med(batches), 1)}))
