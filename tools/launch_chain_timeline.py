#!/usr/bin/env python3
"""Where the streams' time goes in the main phase of a `rocprofv3 --kernel-trace --output-format csv` run of bench.py:
tools/launch_chain_timeline.py <kernel_trace.csv> [K [B [pool]]]      (K: the last K main launches are the window, default 400;
B, pool: instances per step and pool entries of the run, default 1024 and max(64, B / 8))

Per stream (the trace's Stream_Id where it has one, else Queue_Id) and per hardware queue: the share of the window spent in main
launches, resume passes, tail passes, the LPV kernels, and in no kernel at all (gap).  Then how many main launches -- and how many
solve-kernel launches of any class -- are executing at the same time, as a time-weighted histogram.  Classes by workgroups per launch:
`main` B or more (a main launch that carries riders has pool + B), `resume` exactly pool (a pass of the solve kernel over the pool),
`tail` the 512-thread kernel, `one` anything else (the set-up launches of one instance, with or without riders)."""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
POOL = int(sys.argv[4]) if len(sys.argv) > 4 else max(64, B // 8)
skey = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"


def cls(r):
    n = r["Kernel_Name"]
    if "admm_solve" in n:
        g, w = int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])
        if w == 512:
            return "tail"
        return "main" if g // w >= B else ("resume" if g // w == POOL else "one")
    return "lpv" if "lpv" in n else "other"


ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), cls(r), r[skey], r["Queue_Id"], int(r["Grid_Size_X"])) for r in rows)
mains = [e for e in ev if e[2] == "main"]
K = min(K, len(mains))
t0 = mains[-K][0]
t1 = max(e[1] for e in mains[-K:])
W = (t1 - t0) / 1e6
print("window: the last %d main launches, %.3f ms (first start to last end); streams by %s" % (K, W, skey))
print("main-launch grids in the window:", sorted({e[5] for e in mains[-K:]}))


def clip(s, e):
    return max(0, min(e, t1) - max(s, t0))


def union(iv):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return tot + (cur_e - cur_s if cur_e is not None else 0)


for name, idx in (("stream", 3), ("queue", 4)):
    by = defaultdict(lambda: defaultdict(int))
    iv = defaultdict(list)
    cnt = defaultdict(lambda: defaultdict(int))
    for e in ev:
        d = clip(e[0], e[1])
        if d > 0 and e[2] != "other":
            by[e[idx]][e[2]] += d
            cnt[e[idx]][e[2]] += 1
            iv[e[idx]].append((max(e[0], t0), min(e[1], t1)))
    print("\nper %s: share of the window (%%) and launches, by class; gap = no solve / LPV kernel of this %s executing" % (name, name))
    print("  %-8s %7s %7s %7s %7s %7s   launches" % (name, "main", "resume", "tail", "lpv", "gap"))
    for k in sorted(by, key=lambda x: -sum(by[x].values())):
        if by[k]["main"] == 0:
            continue
        busy = union(iv[k])
        print("  %-8s %7.1f %7.1f %7.1f %7.1f %7.1f   %s" % (k, *(100 * by[k][c] / (t1 - t0) for c in ("main", "resume", "tail", "lpv")),
                                                      100 * (1 - busy / (t1 - t0)), dict(cnt[k])))

for title, pick in (("main launches", ("main",)), ("solve-kernel launches of any class", ("main", "resume", "tail", "one"))):
    pts = []
    for e in ev:
        if e[2] in pick and clip(e[0], e[1]) > 0:
            pts.append((max(e[0], t0), 1)); pts.append((min(e[1], t1), -1))
    pts.sort()
    hist, n, last = defaultdict(int), 0, t0
    for t, d in pts:
        hist[n] += t - last
        n += d; last = t
    hist[n] += t1 - last
    tot = sum(hist.values())
    print("\n%s executing at once, share of the window: %s   (time-weighted mean %.2f)"
          % (title, "  ".join("%d: %.1f %%" % (k, 100 * v / tot) for k, v in sorted(hist.items()) if v), sum(k * v for k, v in hist.items()) / tot))

avg = defaultdict(list)
for e in ev:
    if clip(e[0], e[1]) > 0 and e[2] != "other":
        avg[(e[2], e[5])].append(e[1] - e[0])
print("\nclasses in the window: class, grid, launches, average us, total ms")
for (c, g), d in sorted(avg.items(), key=lambda kv: -sum(kv[1])):
    print("  %-6s %7d %5d %8.1f %9.3f" % (c, g, len(d), sum(d) / len(d) / 1e3, sum(d) / 1e6))
