"""Per-(observer, leaver) detection latency, false drops and ghost adds on the flagship workload.

The workload of tools/detection_latency.py: configs[2] (65,536 peers, converged start, 1 % loss, 0.1 %/round churn),
faults for --fault-rounds rounds and a quiet tail, both readings of Failed.  A delta census with
KB_DELTA_ADVANCE after every round feeds a PairTracker (kaboodle_amd/delta.py): for every leaver, how many observers
removed it how many rounds after it stopped, and how many re-inserted it; per round, how often a running peer was
dropped from a view (false drops) and a dead one re-inserted (ghost adds).

    python tools/pair_detection.py [--out profiles/pair_detection.json] [--rounds 200] [--fault-rounds 120]
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
from kaboodle_amd._ffi import (KB_FAILED_SIM_SENDER, KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED,  # noqa: E402
                               KB_VARIANT_EXACT_LRU, SimConfig)
from kaboodle_amd.delta import PairTracker  # noqa: E402


def measure(mode: int, a) -> dict:
    n = a.nodes
    reserve = max(8192, int(n * a.churn * (a.fault_rounds + 8) * 1.5))
    cfg = SimConfig(capacity=n + reserve, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=a.loss, churn=a.churn,
                    fault_end_round=a.fault_rounds, seed=a.seed, failed_mode=mode, track_latency=0,
                    variant=KB_VARIANT_EXACT_LRU)
    t = PairTracker()
    dev_ms, wall_ms, per_round = [], [], []
    with kaboodle_amd.Mesh(cfg) as m:
        m.delta_mark()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            m.step(1)
            t1 = time.perf_counter()
            d = m.delta_census(advance=True)
            wall_ms.append((time.perf_counter() - t1) * 1e3)
            dev_ms.append(m.delta_census_device_ms())
            t.update(d, m.scalars()[:, 0] != 0)
            s = d.summary
            per_round.append([s["round"], s["continuing"], s["new_rows"], s["ended_rows"], s["detections"], s["false_drops"],
                              s["ghost_adds"], s["learned"], s["top_false_drop_by"]])
        wall = time.perf_counter() - t0
        st = m.stats()
    lat = t.latencies()
    faulty = [r for r in per_round if r[0] <= a.fault_rounds]
    quiet = [r for r in per_round if r[0] > a.fault_rounds]
    tot = lambda rows, k: int(sum(r[k] for r in rows))
    return {"capacity": cfg.capacity, "rounds": a.rounds, "fault_rounds": a.fault_rounds, "left": lat["stopped_ids"],
            "pair_detection": {"removals": lat["removals"], "relearned": lat["relearned"], "quantiles_rounds": lat["quantiles"],
                               "detect_hist": lat["detect_hist"], "relearn_hist": lat["relearn_hist"]},
            "totals": {"faulty_rounds": {"detections": tot(faulty, 4), "false_drops": tot(faulty, 5), "ghost_adds": tot(faulty, 6),
                                         "learned": tot(faulty, 7)},
                       "quiet_rounds": {"detections": tot(quiet, 4), "false_drops": tot(quiet, 5), "ghost_adds": tot(quiet, 6),
                                        "learned": tot(quiet, 7)},
                       "last_10_rounds": {"detections": tot(per_round[-10:], 4), "false_drops": tot(per_round[-10:], 5),
                                          "ghost_adds": tot(per_round[-10:], 6), "learned": tot(per_round[-10:], 7)}},
            "removed_counters": {"removed_timeout": st["removed_timeout"], "removed_failed": st["removed_failed"]},
            "per_round_columns": ["round", "continuing", "new_rows", "ended_rows", "detections", "false_drops", "ghost_adds",
                                  "learned", "top_false_drop_by"],
            "per_round": per_round, "final_agree": [st["agree"], st["alive"]], "wall_seconds": round(wall, 2),
            "delta_census_device_ms_median": round(statistics.median(dev_ms), 4),
            "delta_census_with_arrays_wall_ms_median": round(statistics.median(wall_ms), 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_detection.json"))
    ap.add_argument("--nodes", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--fault-rounds", type=int, default=120)
    ap.add_argument("--loss", type=float, default=0.01)
    ap.add_argument("--churn", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    res = {"tool": "tools/pair_detection.py",
           "workload": f"configs[2]: {a.nodes} peers, converged start, {a.loss:.0%} loss, {a.churn:.1%}/round churn for "
                       f"{a.fault_rounds} rounds, {a.rounds} rounds in all, an advancing delta census every round",
           "latency_unit": "rounds from the census that first shows the leaver stopped to the census whose interval holds the "
                           "removal; a pair is counted once per removal (PairTracker)"}
    for name, mode in (("sim_sender", KB_FAILED_SIM_SENDER), ("socket_faithful", KB_FAILED_SOCKET_FAITHFUL)):
        res[name] = measure(mode, a)
        print(name, json.dumps({k: v for k, v in res[name].items() if k != "per_round"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
