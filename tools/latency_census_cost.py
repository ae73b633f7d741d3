"""What a latency census costs: milliseconds per kb_sim_latency_census on the flagship state
(configs[2] after the bench's 25 rounds), and the bandwidth the pass achieves over the table's bytes, beside
k_rowpass's and the view census's on the same machine in the same run.

Each figure is the median of 30 calls after 5 warm-up calls; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the census's kernel and the clearing
of its scratch by HIP events (kb_sim_latency_census_device_ms); `wall_ms` adds the copies to the host and the O(ids)
summary.  The table's bytes are capacity columns x lat_stride(rows) cells x 2 bytes: what the pass has to read of
Dev::lat (the member bits it reads besides are not counted: the figure is the table's bytes per second).

    python tools/latency_census_cost.py [--out profiles/latency_census_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import kaboodle_amd  # noqa: E402
from kaboodle_amd._ffi import KT_ROWPASS  # noqa: E402

WARM, REPS = 5, 30


def timed(call, device_ms) -> dict:
    for _ in range(WARM):
        call()
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(device_ms())
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "device_ms_median": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "repeats": REPS}


def gbs(nbytes: int, ms: float):
    return round(nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latency_census_cost.json"))
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "20", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    if not cfg.track_latency:
        raise SystemExit("the flagship config does not track latency")
    res = {"tool": "tools/latency_census_cost.py",
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {b.warmup + b.steps} rounds"}
    with kaboodle_amd.Mesh(cfg) as m:
        m.step(b.warmup)
        m.reset_kernel_time()
        m.step(b.steps)
        ms, n = m.kernel_time(KT_ROWPASS)
        by = m.kernel_bytes(KT_ROWPASS)
        res["k_rowpass_same_run"] = {"launches": n, "avg_launch_ms": round(ms / max(n, 1), 4),
                                     "algorithmic_bytes_per_launch": by // max(n, 1), "achieved_GBs": gbs(by, ms)}
        c = m.latency_census()
        vc = m.census()
        res["summary"] = c.summary
        res["view_census_summary"] = vc.summary
        # hearsay: entries of the views that no exchange of the observer's own backs
        res["hearsay"] = {"pairs": vc.summary["pairs"], "measured": c.summary["measured"],
                          "hearsay_share": round(1 - c.summary["measured"] / max(vc.summary["pairs"], 1), 6),
                          "ids_all_hearsay": int(((c.measured_by == 0) & (vc.known_by > 0)).sum()),
                          "measured_by_max": int(c.measured_by.max()), "measured_per_row_max": int(c.measured.max()),
                          "measured_per_row_mean": round(float(c.measured[c.measured > 0].mean()), 2) if c.measured.any() else 0}
        rows_stride = (m.capacity + 7) // 8 * 8
        table = 2 * m.capacity * rows_stride
        res["table_bytes"] = table
        res["summary_only"] = timed(lambda: m.latency_census(arrays=False), m.latency_census_device_ms)
        res["with_arrays"] = timed(lambda: m.latency_census(), m.latency_census_device_ms)
        res["achieved_GBs"] = gbs(table, res["summary_only"]["device_ms_median"])
        vt = timed(lambda: m.census(arrays=False), m.census_device_ms)
        vbytes = vc.summary["observers"] * (-(-m.capacity // 8192) * 8192) // 8
        res["view_census_same_run"] = {**vt, "algorithmic_bytes": vbytes, "achieved_GBs": gbs(vbytes, vt["device_ms_median"])}
        rp = res["k_rowpass_same_run"]["achieved_GBs"]
        res["GBs_over_k_rowpass"] = round(res["achieved_GBs"] / rp, 3) if rp else None
        res["GBs_over_view_census"] = round(res["achieved_GBs"] / res["view_census_same_run"]["achieved_GBs"], 3)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
