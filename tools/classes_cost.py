"""What a fingerprint-class census costs: milliseconds per kb_sim_fp_classes on the flagship state,
beside the view census's device time on the same state in the same run and beside the host alternative on the
same state: one fingerprints() download plus np.unique, wall clock.

Each figure is the median of repeated calls after warm-up; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the kernels and the clearing of the
scratch by HIP events (kb_sim_fp_classes_device_ms); `wall_ms` adds the refresh of out-of-date fingerprints, the
running set's fingerprint and the copies to the host.

    python tools/classes_cost.py [--out profiles/classes_cost.json]
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
from kaboodle_amd.classes import fp_classes_ref  # noqa: E402

WARM, REPS = 5, 30


def timed(call, device_ms=None) -> dict:
    for _ in range(WARM):
        call()
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        if device_ms:
            dev.append(device_ms())
    out = {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "repeats": REPS}
    if dev:
        out.update(device_ms_median=round(statistics.median(dev), 4), device_ms_min=round(min(dev), 4))
    return out


def host_alternative(mesh):
    import numpy as np
    fps = mesh.fingerprints()
    return np.unique(fps[fps != 0], return_counts=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_cost.json"))
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "20", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    res = {"tool": "tools/classes_cost.py",
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {b.warmup + b.steps} rounds"}
    with kaboodle_amd.Mesh(cfg) as m:
        m.step(b.warmup + b.steps)
        r = m.fp_classes(top=8)
        res["summary"] = r.summary
        res["top_classes"] = r.classes.tolist()
        res["equals_numpy_reference"] = not m.fp_classes(top=16).same_as(fp_classes_ref(m, top=16))
        res["summary_only"] = timed(lambda: m.fp_classes(top=0, arrays=False), m.fp_classes_device_ms)
        res["summary_and_top_16"] = timed(lambda: m.fp_classes(top=16, arrays=False), m.fp_classes_device_ms)
        res["top_1024_and_arrays"] = timed(lambda: m.fp_classes(top=1024), m.fp_classes_device_ms)
        res["census_summary_only_same_state"] = timed(lambda: m.census(arrays=False), m.census_device_ms)
        res["host_fingerprints_plus_unique_same_state"] = timed(lambda: host_alternative(m))
        ms = res["summary_and_top_16"]["device_ms_median"]
        cs = res["census_summary_only_same_state"]["device_ms_median"]
        res["device_ms_over_census"] = round(ms / cs, 3) if cs > 0 else None
        res["host_wall_over_call_wall"] = round(res["host_fingerprints_plus_unique_same_state"]["wall_ms_median"] /
                                                res["summary_and_top_16"]["wall_ms_median"], 3)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
