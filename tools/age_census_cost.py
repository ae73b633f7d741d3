"""What a contact-age census costs: milliseconds per kb_sim_age_census over sparse rows at 262,144
peers (socket_faithful, loss 0.05, after 20 rounds), beside the view census's device time on the same state in the
same run.

Each figure is the median of 30 calls after 5 warm-up calls; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the census's kernels (the view
census's sparse pass it reuses included) and the clearing of its scratch by HIP events
(kb_sim_age_census_device_ms); `wall_ms` adds the copies to the host and the O(ids) summary.

    python tools/age_census_cost.py [--out profiles/age_census_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kaboodle_amd  # noqa: E402
from kaboodle_amd._ffi import (KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED,  # noqa: E402
                               KB_VARIANT_SPARSE_ROWS, SimConfig)

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


def short(summary: dict) -> dict:
    """The summary with the histogram cut after its last nonzero bucket."""
    h = summary["hist"]
    last = max((k for k, v in enumerate(h) if v), default=-1)
    return {**summary, "hist": h[: last + 1]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "age_census_cost.json"))
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    res = {"tool": "tools/age_census_cost.py"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    n = 262144
    sc = SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=0.05, seed=9,
                   failed_mode=KB_FAILED_SOCKET_FAITHFUL, variant=KB_VARIANT_SPARSE_ROWS, sparse_row_cap=2048)
    with kaboodle_amd.Mesh(sc) as m:
        for _ in range(4):
            m.step(5)
            print(f"sparse: round {m.stats()['round']}", flush=True)
        c = m.age_census()
        res["sparse_256k"] = {"handle": "sparse rows, 262,144 peers, socket_faithful, loss 0.05, 20 rounds",
                              "summary": short(c.summary),
                              "summary_only": timed(lambda: m.age_census(arrays=False), m.age_census_device_ms),
                              "with_arrays": timed(lambda: m.age_census(), m.age_census_device_ms),
                              "view_census_same_run": timed(lambda: m.census(arrays=False), m.census_device_ms)}
    print(json.dumps({"sparse_256k": res["sparse_256k"]}), flush=True)
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
