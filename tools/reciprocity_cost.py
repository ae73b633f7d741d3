"""What a reciprocity census costs: milliseconds per kb_sim_reciprocity on the flagship state and
on the same state as 8 in-process row shards, beside the view census's device time on the same state in the same
run (the census reads the same member bits once, so it is the yardstick).

Each figure is the median of repeated calls after warm-up; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the kernels and the clearing of the
scratch by HIP events (kb_sim_reciprocity_device_ms); `wall_ms` adds the copies to the host, the O(ids) summary
and the sort of the pair list.  The pass reads rows x W/8 algorithmic bytes (the member bits of the running rows,
every block once); its achieved bandwidth is set beside the HBM peak used throughout (8 TB/s).

    python tools/reciprocity_cost.py [--out profiles/reciprocity_cost.json] [--skip-shards]
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


def figures(mesh, label: str) -> dict:
    r = mesh.reciprocity()
    rows, width = r.summary["observers"], -(-mesh.capacity // 8192) * 8192
    nbytes = rows * width // 8
    out = {"state": label, "summary": r.summary, "algorithmic_bytes": nbytes,
           "summary_only": timed(lambda: mesh.reciprocity(arrays=False), mesh.reciprocity_device_ms),
           "with_arrays_and_pairs": timed(mesh.reciprocity, mesh.reciprocity_device_ms),
           "census_summary_only_same_state": timed(lambda: mesh.census(arrays=False), mesh.census_device_ms)}
    ms, cs = out["summary_only"]["device_ms_median"], out["census_summary_only_same_state"]["device_ms_median"]
    out["achieved_GBs"] = round(nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
    out["frac_of_8TBs"] = round(out["achieved_GBs"] / HBM_PEAK_GBS, 4) if ms > 0 else None
    out["device_ms_over_census"] = round(ms / cs, 3) if cs > 0 else None
    c = mesh.census()
    out["identities_hold"] = bool(((r.mutual + r.lacks) == c.missing).all() and int(r.lacks.sum()) == int(r.lacked_by.sum())
                                  and int(r.mutual.sum()) == 2 * r.summary["mutual_pairs"])
    return out


def dump(path: str, res: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reciprocity_cost.json"))
    ap.add_argument("--skip-shards", action="store_true")
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "20", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    res = {"tool": "tools/reciprocity_cost.py", "hbm_peak_GBs": HBM_PEAK_GBS,
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {b.warmup + b.steps} rounds"}
    with kaboodle_amd.Mesh(cfg) as m:
        m.step(b.warmup + b.steps)
        res["dense"] = figures(m, "unsharded")
    print(json.dumps(res["dense"]), flush=True)
    dump(a.out, res)
    if not a.skip_shards:
        with kaboodle_amd.Mesh(cfg, shards=8) as m:
            m.step(b.warmup + b.steps)
            res["dense_8_local_shards"] = figures(m, "8 in-process row shards, one device")
            res["dense_8_local_shards"]["summary_equals_unsharded"] = bool(
                res["dense_8_local_shards"]["summary"] == res["dense"]["summary"])
        print(json.dumps(res["dense_8_local_shards"]), flush=True)
        dump(a.out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
