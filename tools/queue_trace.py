#!/usr/bin/env python3
"""Which hardware queue each stream's kernels ran on, and how busy each queue was over the timed passes of a bench.py run, from a
rocprofv3 kernel trace (DESIGN.md sections 12 and 31):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 20 --warmup 3
    python tools/queue_trace.py DIR 20 [out.json]

The window is that of the last N passes: from the start of the earliest of their first launches to the end of the last box launch.
A pass is counted on the queue that ran its box launch."""
import csv
import glob
import json
import os
import sys

FIRST, LAST = "k_rle_erode_pack", "k_box_nms"      # a steady-state pass starts with the mask launch and ends with the boxes


def load(trace_dir):
    paths = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for r in csv.DictReader(open(paths[-1])):
        rows.append(dict(name=r["Kernel_Name"], q=int(r["Queue_Id"]), s=int(r.get("Stream_Id", -1) or -1),
                         t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r["t0"])
    return rows


def busy_ns(spans):
    total, end = 0, None
    for a, b in sorted(spans):
        if end is None or a > end:
            total += b - a
            end = b
        elif b > end:
            total += b - end
            end = b
    return total


def summarise(rows, n_passes):
    firsts = [r for r in rows if FIRST in r["name"]]
    lasts = [r for r in rows if LAST in r["name"]]
    if len(firsts) < n_passes or len(lasts) < n_passes:
        raise SystemExit(f"{len(firsts)} first launches, {len(lasts)} box launches: fewer than {n_passes} passes in the trace")
    w0, w1 = min(r["t0"] for r in firsts[-n_passes:]), max(r["t1"] for r in lasts[-n_passes:])
    inside = [r for r in rows if r["t0"] >= w0 and r["t1"] <= w1]
    queues = {}
    for r in inside:
        q = queues.setdefault(r["q"], dict(streams={}, dispatches=0, passes=0, spans=[], order=[]))
        q["streams"][str(r["s"])] = q["streams"].get(str(r["s"]), 0) + 1
        q["dispatches"] += 1
        q["spans"].append((r["t0"], r["t1"]))
        if LAST in r["name"]:
            q["passes"] += 1
        if FIRST in r["name"]:
            q["order"].append(r["s"])
    out = {}
    for k, q in sorted(queues.items()):
        b = busy_ns(q["spans"])
        # two batches' passes one behind the other on a queue show as first launches of more than one stream there
        out[str(k)] = dict(streams=q["streams"], dispatches=q["dispatches"], passes=q["passes"], busy_us=round(b / 1e3, 1),
                           busy_share_of_window=round(b / (w1 - w0), 3), streams_starting_passes=sorted(set(q["order"])))
    whole = {}
    for r in rows:
        s = whole.setdefault(str(r["s"]), {})
        s[str(r["q"])] = s.get(str(r["q"]), 0) + 1
    return dict(passes_in_window=n_passes, window_us=round((w1 - w0) / 1e3, 1), queues=out, stream_to_queue_whole_trace=whole)


if __name__ == "__main__":
    res = summarise(load(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
