"""The stretch between k_set_cap and the receive window in a rocprofv3 kernel trace (dev tool): per timed round the
start and end of every kernel from k_set_cap up to the round's first k_route, relative to k_set_cap's start, averaged
over the rounds (the Join responses around A2).

    resp_trace.py <dir with *kernel_trace.csv> <warmup> <steps>

Rounds are delimited by k_round_end (prof_summary.py).  A kernel launched twice in the stretch (the two phases of
k_resp_wave and k_resp_node) is listed as name and name#2 in launch order.
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
    acc, spans = {}, []
    for rd in rounds:
        names = [bench_name(r["Kernel_Name"]) for r in rd]
        if "k_set_cap" not in names or "k_route" not in names:
            continue
        a, b = names.index("k_set_cap"), names.index("k_route")
        t0 = int(rd[a]["Start_Timestamp"])
        seen = {}
        for r in rd[a:b]:
            n = bench_name(r["Kernel_Name"])
            seen[n] = seen.get(n, 0) + 1
            key = n if seen[n] == 1 else f"{n}#{seen[n]}"
            e = acc.setdefault(key, [0, 0.0, 0.0, r.get("Grid_Size", r.get("Grid_Size_X", ""))])
            e[0] += 1
            e[1] += (int(r["Start_Timestamp"]) - t0) / 1e3
            e[2] += (int(r["End_Timestamp"]) - t0) / 1e3
        spans.append((int(rd[b]["Start_Timestamp"]) - t0) / 1e3)
    n = len(spans)
    out = {"rounds": n, "warmup": warmup, "steps": steps, "unit": "us, averages over the timed rounds",
           "k_set_cap_start_to_first_k_route_start_us": round(sum(spans) / n, 2),
           "min_max_us": [round(min(spans), 2), round(max(spans), 2)],
           "kernels_rel_k_set_cap_start": {k: {"seen_in_rounds": e[0], "start_us": round(e[1] / e[0], 2),
                                               "end_us": round(e[2] / e[0], 2), "dur_us": round((e[2] - e[1]) / e[0], 2),
                                               "grid": e[3]}
                                           for k, e in sorted(acc.items(), key=lambda kv: kv[1][1] / kv[1][0])}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
