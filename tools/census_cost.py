"""What a view census costs: milliseconds per kb_sim_census on the flagship state, on the same
state as 8 in-process row shards, and on 4M peers of sparse rows.

Each figure is the median of repeated calls after warm-up; every call is synchronous (it returns after its
copies), so the wall time is a synchronised time.  `device_ms` is the time of the census's kernels and the
clearing of its scratch by HIP events (kb_sim_census_device_ms); `wall_ms` adds the copies to the host and the
O(ids) summary.  The dense pass reads rows x W/8 algorithmic bytes (the member bits of the running rows); its
achieved bandwidth is set beside k_rowpass's on the same run (the project's best streaming kernel over these
tables) and beside the HBM peak used throughout (8 TB/s).  The only alternative before the census — row()
downloads and a numpy count — is timed on a 2,048-row sample and SCALED to all rows.

    python tools/census_cost.py [--out profiles/census_cost.json] [--skip-4m] [--skip-shards]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import kaboodle_amd  # noqa: E402
from kaboodle_amd._ffi import (KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED, KB_STAT_NO_SF_FAILED_DROPS,  # noqa: E402
                               KB_VARIANT_SPARSE_ROWS, KT_ROWPASS, SimConfig)

HBM_PEAK_GBS = 8000.0
WARM, REPS = 5, 30


def timed(mesh, arrays: bool) -> dict:
    for _ in range(WARM):
        mesh.census(arrays=arrays)
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        mesh.census(arrays=arrays)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(mesh.census_device_ms())
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "device_ms_median": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "repeats": REPS}


def dense_figures(mesh, label: str) -> dict:
    c = mesh.census()
    rows, width = c.summary["observers"], -(-mesh.capacity // 8192) * 8192
    nbytes = rows * width // 8
    out = {"state": label, "summary": c.summary, "algorithmic_bytes": nbytes,
           "summary_only": timed(mesh, False), "with_arrays": timed(mesh, True)}
    ms = out["summary_only"]["device_ms_median"]
    out["achieved_GBs"] = round(nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
    out["frac_of_8TBs"] = round(out["achieved_GBs"] / HBM_PEAK_GBS, 4) if ms > 0 else None
    return out


def row_download_alternative(mesh, sample: int = 2048) -> dict:
    """The host-side count through row(): timed on `sample` running rows, scaled to every running row."""
    running = np.flatnonzero(mesh.scalars()[:, 0] != 0)
    ids = running[np.linspace(0, len(running) - 1, sample).astype(np.int64)]
    t0 = time.perf_counter()
    kb = np.zeros(mesh.capacity, dtype=np.uint32)
    for i in ids:
        kb += mesh.row(int(i)) != 0
    dt = time.perf_counter() - t0
    return {"sampled_rows": sample, "sample_seconds": round(dt, 3),
            "scaled_to_all_rows_seconds": round(dt * len(running) / sample, 1), "scaled": True}


def dump(path: str, res: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_cost.json"))
    ap.add_argument("--skip-4m", action="store_true")
    ap.add_argument("--skip-shards", action="store_true")
    ap.add_argument("--nodes-4m", type=int, default=4 * 1024 * 1024)
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "20", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    res = {"tool": "tools/census_cost.py", "hbm_peak_GBs": HBM_PEAK_GBS,
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {b.warmup + b.steps} rounds"}

    with kaboodle_amd.Mesh(cfg) as m:
        m.step(b.warmup)
        m.reset_kernel_time()
        m.step(b.steps)
        ms, n = m.kernel_time(KT_ROWPASS)
        by = m.kernel_bytes(KT_ROWPASS)
        res["k_rowpass_same_run"] = {"launches": n, "avg_launch_ms": round(ms / max(n, 1), 4),
                                     "algorithmic_bytes_per_launch": by // max(n, 1),
                                     "achieved_GBs": round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
        res["dense"] = dense_figures(m, "unsharded")
        res["dense"]["rows_per_wave_env"] = os.environ.get("KB_CENSUS_RPW")
        res["row_download_alternative"] = row_download_alternative(m)
        st = m.stats()
        res["round_ms_same_run"] = None
        t0 = time.perf_counter()
        m.step(5)
        res["round_ms_same_run"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        res["alive"] = st["alive"]
    print(json.dumps({k: res[k] for k in ("k_rowpass_same_run", "dense", "row_download_alternative")}), flush=True)
    dump(a.out, res)

    if not a.skip_shards:
        with kaboodle_amd.Mesh(cfg, shards=8) as m:
            m.step(b.warmup + b.steps)
            res["dense_8_local_shards"] = dense_figures(m, "8 in-process row shards, one device")
            same = m.census().summary == res["dense"]["summary"]
            res["dense_8_local_shards"]["summary_equals_unsharded"] = bool(same)
        print(json.dumps(res["dense_8_local_shards"]), flush=True)
        dump(a.out, res)

    if not a.skip_4m:
        n = a.nodes_4m
        # (a) configs[4]'s mesh (§8: 5 % loss, socket_faithful, the Failed lists' drops not counted) a few rounds in:
        #     every row holds a handful of explicit stamps and exceptions
        scfg = SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=0.05, seed=9,
                         failed_mode=KB_FAILED_SOCKET_FAITHFUL, stat_flags=KB_STAT_NO_SF_FAILED_DROPS,
                         variant=KB_VARIANT_SPARSE_ROWS, sparse_row_cap=2048)
        with kaboodle_amd.Mesh(scfg) as m:
            m.step(3)
            lossy = {"state": "configs[4]'s mesh (5 % loss, socket_faithful) after 3 rounds",
                     "summary": m.census(arrays=False).summary, "footprint": m.sparse_footprint(),
                     "summary_only": timed(m, False), "with_arrays": timed(m, True)}
        res["sparse_4m"] = {"peers": n, "lossy": lossy}
        dump(a.out, res)
        # (b) the one-address case: no loss, Failed honoured (sim_sender); two peers stop, are detected and their
        #     Failed broadcasts make every row drop them, so every row holds the same two exceptions
        hcfg = SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, seed=9,
                         variant=KB_VARIANT_SPARSE_ROWS, sparse_row_cap=2048)
        with kaboodle_amd.Mesh(hcfg) as m:
            m.step(2)
            quiet = {"state": "no loss, 2 rounds after a converged start: no exceptions at all",
                     "summary": m.census(arrays=False).summary, "footprint": m.sparse_footprint(),
                     "summary_only": timed(m, False), "with_arrays": timed(m, True)}
            left = [1000, n // 2 + 7]
            for j in left:
                m.stop_node(j)
            m.step(12)
            c = m.census()
            hot = {"state": f"12 rounds after ids {left} stopped: an exception for them in every row that dropped them",
                   "known_by_of_stopped": [int(c.known_by[j]) for j in left], "summary": c.summary,
                   "footprint": m.sparse_footprint(), "summary_only": timed(m, False), "with_arrays": timed(m, True)}
        res["sparse_4m"].update({"quiet": quiet, "after_leaves": hot})
        print(json.dumps(res["sparse_4m"]), flush=True)

    dump(a.out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
