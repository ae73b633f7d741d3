"""Wave 0 of the receive window in a rocprofv3 kernel trace (dev tool): per timed round the start and end of every
wave-0 kernel relative to the round's first k_route, averaged over the rounds.

    wave0_trace.py <dir with *kernel_trace.csv> <warmup> <steps>

Rounds are delimited by k_round_end, waves by k_route (prof_summary.py).  Wave 0 = the dispatches from the round's
first k_route up to its second.  With the KnownPeers launch split wave 0 holds two k_kp and two
k_proc dispatches; `overlap` is then how long the first k_proc ran before the longer k_kp ended.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prof_summary import bench_name, rows, timed_window  # noqa: E402


def main(d, warmup, steps):
    tr = rows(os.path.join(d, "**", "*kernel_trace.csv"))
    lo, hi = timed_window(tr, warmup, steps, "Dispatch_Id")
    tr = sorted((r for r in tr if lo < int(r["Dispatch_Id"]) <= hi), key=lambda r: int(r["Dispatch_Id"]))
    rounds, cur = [], []
    for r in tr:
        cur.append(r)
        if bench_name(r["Kernel_Name"]) == "k_round_end":
            rounds.append(cur)
            cur = []
    acc, spans, kp_long, kp_short, proc0, overlap, nkp = {}, [], [], [], [], [], []
    for rd in rounds:
        routes = [k for k, r in enumerate(rd) if bench_name(r["Kernel_Name"]) == "k_route"]
        if len(routes) < 2:
            continue
        w0 = rd[routes[0]:routes[1]]
        t0 = int(w0[0]["Start_Timestamp"])
        seen = {}
        for r in w0:
            n = bench_name(r["Kernel_Name"])
            seen[n] = seen.get(n, 0) + 1
            key = n if seen[n] == 1 else f"{n}#{seen[n]}"
            a, b = (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3
            e = acc.setdefault(key, [0, 0.0, 0.0, r.get("Grid_Size", r.get("Grid_Size_X", ""))])
            e[0] += 1
            e[1] += a
            e[2] += b
        spans.append(max(int(r["End_Timestamp"]) for r in w0) - t0)
        kps = [r for r in w0 if bench_name(r["Kernel_Name"]) == "k_kp"]
        pcs = [r for r in w0 if bench_name(r["Kernel_Name"]) == "k_proc"]
        dur = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in kps)
        nkp.append(len(kps))
        kp_long.append(dur[-1])
        kp_short.append(dur[0] if len(dur) > 1 else 0)
        proc0.append(int(pcs[0]["End_Timestamp"]) - int(pcs[0]["Start_Timestamp"]))
        longest = max(kps, key=lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        overlap.append(max(0, min(int(longest["End_Timestamp"]), int(pcs[0]["End_Timestamp"])) -
                           max(int(longest["Start_Timestamp"]), int(pcs[0]["Start_Timestamp"]))))
    n = len(spans)
    avg = lambda v: round(sum(v) / len(v) / 1e3, 2)
    out = {"rounds": n, "warmup": warmup, "steps": steps, "unit": "us, averages over the timed rounds",
           "wave0_span_us": avg(spans), "wave0_span_min_max_us": [round(min(spans) / 1e3, 2), round(max(spans) / 1e3, 2)],
           "k_kp_launches_in_wave0": round(sum(nkp) / n, 2), "k_kp_longest_us": avg(kp_long), "k_kp_other_us": avg(kp_short),
           "k_proc_first_us": avg(proc0), "k_proc_overlaps_longest_k_kp_us": avg(overlap),
           "kernels_rel_first_k_route": {k: {"seen_in_rounds": e[0], "start_us": round(e[1] / e[0], 2),
                                             "end_us": round(e[2] / e[0], 2), "grid": e[3]}
                                         for k, e in sorted(acc.items(), key=lambda kv: kv[1][1] / kv[1][0])}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
