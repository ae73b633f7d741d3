"""What an island census costs: milliseconds per kb_sim_islands on the flagship state (configs[2],
sim_sender, after 20 rounds), and on the same state as 8 in-process row shards, beside the view census (kb_sim_census)
on the same state in the same run.

Every call is synchronous (it returns after its copies), so the wall time is a synchronised time.  `device_ms` is the
span from the first kernel of the call to the last by HIP events (kb_sim_islands_device_ms): it holds the host's
4-byte read of the `changed` word between two sweeps; `wall_ms` adds the download of the labels and the O(ids)
summary.  The census is read-only, so it is repeated on one state: the median of REPS calls after WARM warm-up calls.
A sweep streams the running rows x W/8 bytes twice (pull, then push: the second read comes from the cache the first
filled); `bytes_streamed_once` is one such read per sweep, and the achieved GB/s is over it.  `sweeps` is what the
call reported: a property of the execution, recorded, not asserted.

    python tools/islands_cost.py [--out profiles/islands_cost.json] [--skip-shards]
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

HBM_PEAK_GBS = 8000.0
WARM, REPS = 5, 30


def repeated(fn, ms) -> dict:
    for _ in range(WARM):
        fn()
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms())
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "device_ms_median": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "repeats": REPS}


def figures(cfg, rounds: int, shards: int) -> dict:
    with kaboodle_amd.Mesh(cfg, shards=shards) as m:
        m.step(rounds)
        first = m.islands()
        view = repeated(lambda: m.census(arrays=False), m.census_device_ms)
        sweeps = []

        def summary_only():
            sweeps.append(m.islands(arrays=False).summary["sweeps"])

        so = repeated(summary_only, m.islands_device_ms)
        wa = repeated(lambda: m.islands(arrays=True), m.islands_device_ms)
        width = -(-m.capacity // 8192) * 8192
        once = first.summary["observers"] * width // 8
        so["sweeps_median"], so["sweeps_min"], so["sweeps_max"] = int(statistics.median(sweeps)), min(sweeps), max(sweeps)
        so["bytes_streamed_once"] = once * so["sweeps_median"]
        so["achieved_GBs"] = round(so["bytes_streamed_once"] / (so["device_ms_median"] * 1e-3) / 1e9, 1)
        so["frac_of_8TBs"] = round(so["achieved_GBs"] / HBM_PEAK_GBS, 4)
        so["device_ms_per_sweep"] = round(so["device_ms_median"] / so["sweeps_median"], 4)
        return {"summary": first.summary, "row_bytes_per_sweep": once, "view_census_same_state": view, "summary_only": so,
                "with_arrays": wa, "same_answer_every_call": not m.islands().same_as(first),
                "device_ms_over_view_census": round(so["device_ms_median"] / view["device_ms_median"], 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "islands_cost.json"))
    ap.add_argument("--skip-shards", action="store_true")
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "15", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    rounds = b.warmup + b.steps
    res = {"tool": "tools/islands_cost.py", "hbm_peak_GBs": HBM_PEAK_GBS, "warm_up_calls": WARM,
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {rounds} rounds"}
    res["dense"] = figures(cfg, rounds, 0)
    print(json.dumps(res["dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if not a.skip_shards:
        res["dense_8_local_shards"] = figures(cfg, rounds, 8)
        res["dense_8_local_shards"]["summary_equals_unsharded"] = (
            {k: v for k, v in res["dense_8_local_shards"]["summary"].items() if k != "sweeps"}
            == {k: v for k, v in res["dense"]["summary"].items() if k != "sweeps"})
        print(json.dumps(res["dense_8_local_shards"]), flush=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
