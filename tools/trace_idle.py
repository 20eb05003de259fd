#!/usr/bin/env python3
"""Device idle time per replay iteration from a rocprofv3 kernel (+ memory copy) trace of bench.py:

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o k -- python3 bench.py --steps 20 --warmup 5
    python3 tools/trace_idle.py DIR 20

Over the last `iterations` iterations (from one k_gprop launch to the next): wall time, the sum of kernel and copy durations, the
difference (the device had nothing to run), the idle gap behind each of the four host looks (between the look's last kernel and the next
kernel that is not one of the runtime's copy kernels), every gap over 5 us by the kernels on either side, and per-kernel totals with
quoted names.  The runtime's blit copies (`__amd_rocclr_copyBuffer`) count as copies."""
import csv, glob, json, os, sys

def load(d):
    ops = []
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            nm = r["Kernel_Name"]
            ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), nm, "c" if "copyBuffer" in nm else "k"))
    for f in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy:" + r.get("Direction", "?"), "c"))
    ops.sort()
    return ops

def short(n):
    n = n.split("(")[0]
    return n.replace("void ", "")

def main():
    d, iters = sys.argv[1], int(sys.argv[2])
    ops = load(d)
    at = [k for k, o in enumerate(ops) if short(o[2]).startswith("k_gprop")]  # update_G's proposals: exactly one launch per iteration
    if len(at) < iters + 1:
        print("too few k_gprop launches:", len(at)); sys.exit(1)
    a, b = at[-iters - 1], at[-1]
    win = ops[a:b]
    wall = ops[b][0] - ops[a][0]
    busy_k = sum(o[1] - o[0] for o in win if o[3] == "k")
    busy_c = sum(o[1] - o[0] for o in win if o[3] == "c")
    # union of busy intervals (copies can overlap kernels)
    cover, cur_e = 0, ops[a][0]
    for s, e, _, _ in win:
        s = max(s, cur_e)
        if e > s:
            cover += e - s
            cur_e = e
    res = {"iterations": iters, "wall_ms_per_iter": wall / iters / 1e6, "kernel_ms_per_iter": busy_k / iters / 1e6, "copy_ms_per_iter": busy_c / iters / 1e6,
           "idle_ms_per_iter_wall_minus_sum": (wall - busy_k - busy_c) / iters / 1e6, "idle_ms_per_iter_uncovered": (wall - cover) / iters / 1e6,
           "kernels_per_iter": sum(1 for o in win if o[3] == "k") / iters, "copies_per_iter": sum(1 for o in win if o[3] == "c") / iters}
    # the gap behind each look: idle between the anchor kernel's end and the next KERNEL's start, copies subtracted
    anchors = {"update_P (after k_pdirich_at)": "k_pdirich_at", "update_G (after k_loglik_int<256, true>)": "k_loglik_int<256, true>",
               "update_ZQ (after k_zq_at)": "k_zq_at", "update_alpha (after k_alpha_ratios)": "k_alpha_ratios"}
    gaps = {}
    for label, key in anchors.items():
        g = []
        for k in range(a, b):
            if ops[k][3] == "k" and short(ops[k][2]).startswith(key.split("<")[0]) and (key.find("<") < 0 or key in ops[k][2]):
                end = ops[k][1]
                j = k + 1
                cp = 0
                while j < len(ops) and ops[j][3] != "k":
                    cp += ops[j][1] - max(ops[j][0], end)
                    j += 1
                if j < len(ops):
                    g.append((ops[j][0] - end - cp, short(ops[j][2])))
        if g:
            vals = sorted(x[0] for x in g)
            gaps[label] = {"n": len(g), "median_us": vals[len(vals) // 2] / 1e3, "mean_us": sum(vals) / len(vals) / 1e3, "next": g[len(g) // 2][1]}
    res["look_gaps"] = gaps
    # all gaps > 5 us in the window, by (previous kernel -> next kernel)
    big = {}
    prev = None
    for o in win:
        if o[3] != "k":
            continue
        if prev is not None:
            gp = o[0] - prev[1]
            if gp > 5000:
                key = short(prev[2])[:40] + " -> " + short(o[2])[:40]
                e = big.setdefault(key, [0, 0])
                e[0] += 1; e[1] += gp
        prev = o
    res["gaps_over_5us_ms_per_iter"] = {k: {"n_per_iter": v[0] / iters, "ms_per_iter": v[1] / iters / 1e6} for k, v in sorted(big.items(), key=lambda kv: -kv[1][1])[:25]}
    # per-kernel totals
    per = {}
    for o in win:
        e = per.setdefault(short(o[2]) if o[3] == "k" else o[2], [0, 0])
        e[0] += 1; e[1] += o[1] - o[0]
    res["per_kernel"] = {'"%s"' % k: {"n_per_iter": v[0] / iters, "ms_per_iter": v[1] / iters / 1e6} for k, v in sorted(per.items(), key=lambda kv: -kv[1][1])}
    print(json.dumps(res, indent=1))

main()
