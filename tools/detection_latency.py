"""Per-failure detection latency and per-join dissemination latency on the flagship workload.

configs[2] (65,536 peers, converged start, 1 % loss, 0.1 %/round churn) runs with a census after every round fed to
the Tracker (kaboodle_amd/census.py): for every peer that left, the rounds until the first view dropped it
(`first_dropped`) and until no view held it (`gone`); for every peer that joined, the rounds until every view
held it (`everywhere`).  Faults stop after --fault-rounds so the open records can complete during the quiet tail.
Both readings of Failed are measured.  The reference claims a failed peer is detected within
2·N ticks (src/kaboodle.rs:656-660: every peer is pinged once per sweep of the map); the distributions are set
beside that bound.

    python tools/detection_latency.py [--out profiles/detection_latency.json] [--rounds 200] [--fault-rounds 120]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kaboodle_amd  # noqa: E402
from kaboodle_amd._ffi import (KB_FAILED_SIM_SENDER, KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED,  # noqa: E402
                               KB_VARIANT_EXACT_LRU, SimConfig)
from kaboodle_amd.census import Tracker  # noqa: E402


def dist(x: np.ndarray) -> dict:
    if not len(x):
        return {"n": 0}
    return {"n": int(len(x)), "min": int(x.min()), "median": float(np.median(x)), "p90": float(np.percentile(x, 90)),
            "p99": float(np.percentile(x, 99)), "max": int(x.max()), "mean": round(float(x.mean()), 2)}


def measure(mode: int, a) -> dict:
    n = a.nodes
    reserve = max(8192, int(n * a.churn * (a.fault_rounds + 8) * 1.5))
    cfg = SimConfig(capacity=n + reserve, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=a.loss, churn=a.churn,
                    fault_end_round=a.fault_rounds, seed=a.seed, failed_mode=mode, track_latency=0,
                    variant=KB_VARIANT_EXACT_LRU)
    t = Tracker()
    census_ms = []
    with kaboodle_amd.Mesh(cfg) as m:
        t.update(m.census())
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            m.step(1)
            t1 = time.perf_counter()
            c = m.census()
            census_ms.append((time.perf_counter() - t1) * 1e3)
            t.update(c)
        wall = time.perf_counter() - t0
        last, st = c.summary, m.stats()
    lat, hist = t.latencies(), t.histogram()
    return {"capacity": cfg.capacity, "rounds": a.rounds, "fault_rounds": a.fault_rounds,
            "left": len(t.stopped), "joined": len(t.started),
            "detection_first_dropped": dist(lat["first_dropped"]), "detection_gone": dist(lat["gone"]),
            "dissemination_everywhere": dist(lat["everywhere"]),
            "open_gone": lat["open_gone"], "open_everywhere": lat["open_everywhere"], "histogram": hist,
            "reference_bound_ticks": 2 * n,
            "final_census": last, "final_agree": [st["agree"], st["alive"]],
            "wall_seconds": round(wall, 2), "census_with_arrays_and_scalars_ms_median": round(float(np.median(census_ms)), 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detection_latency.json"))
    ap.add_argument("--nodes", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--fault-rounds", type=int, default=120)
    ap.add_argument("--loss", type=float, default=0.01)
    ap.add_argument("--churn", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    res = {"tool": "tools/detection_latency.py",
           "workload": f"configs[2]: {a.nodes} peers, converged start, {a.loss:.0%} loss, {a.churn:.1%}/round churn for "
                       f"{a.fault_rounds} rounds, {a.rounds} rounds in all, a census every round",
           "latency_unit": "rounds from the census that first shows the change",
           "reference_claim": "src/kaboodle.rs:656-660: detection within 2*N ticks"}
    for name, mode in (("sim_sender", KB_FAILED_SIM_SENDER), ("socket_faithful", KB_FAILED_SOCKET_FAITHFUL)):
        res[name] = measure(mode, a)
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "histogram"}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
