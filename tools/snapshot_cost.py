"""What a snapshot and a restore cost: on sparse rows at 262,144 peers (socket_faithful, loss 0.05,
after 20 rounds, the state of tools/age_census_cost.py) the snapshot's bytes beside the 4·C·ESTR bytes the entry
table is allocated with, the device time of the pack and of the unpack, the wall time of snapshot() and restore(),
and one round's step time for scale.

Each figure is the median of 30 calls after 5 warm-up calls; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the scan and the entry kernel by HIP
events (kb_sim_snapshot_device_ms); `wall_ms` adds the copies, the host's assembly and the checksum (restore: the
validation and the creation of the handle).  Reported, not gated.

    python tools/snapshot_cost.py [--out profiles/snapshot_cost.json]
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
from kaboodle_amd import snapshot  # noqa: E402
from kaboodle_amd._ffi import (KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED,  # noqa: E402
                               KB_VARIANT_SPARSE_ROWS, Sim, SimConfig)

WARM, REPS = 5, 30


def timed(call) -> dict:
    """call() -> the device ms of that call."""
    for _ in range(WARM):
        call()
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        d = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(d)
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "device_ms_median": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "repeats": REPS}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_cost.json"))
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    lib = kaboodle_amd.lib()
    n, cap = 262144, 2048
    sc = SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=0.05, seed=9,
                   failed_mode=KB_FAILED_SOCKET_FAITHFUL, variant=KB_VARIANT_SPARSE_ROWS, sparse_row_cap=cap)
    with kaboodle_amd.Mesh(sc) as m:
        for _ in range(4):
            m.step(5)
            print(f"sparse: round {m.stats()['round']}", flush=True)
        blob = m.snapshot()
        info = snapshot.info(blob, lib)

        def snap() -> float:
            m.snapshot()
            return m.snapshot_device_ms()

        def rest() -> float:
            with Sim.restore(lib, blob) as b:
                return b.snapshot_device_ms()

        res = {"tool": "tools/snapshot_cost.py",
               "handle": "sparse rows, 262,144 peers, socket_faithful, loss 0.05, 20 rounds, sparse_row_cap 2048",
               "snapshot_bytes": len(blob), "entries": info["entries"], "entry_bytes": 4 * info["entries"],
               "entry_table_allocated_bytes": 4 * n * ((cap + 3) // 4 * 4),
               "snapshot": timed(snap), "restore": timed(rest)}
        with Sim.restore(lib, blob) as b:
            res["fixed_point"] = b.snapshot() == blob
        step = []
        for _ in range(WARM + REPS):
            t0 = time.perf_counter()
            m.step(1)
            step.append((time.perf_counter() - t0) * 1e3)
        res["step_ms_median"] = round(statistics.median(step[WARM:]), 4)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
