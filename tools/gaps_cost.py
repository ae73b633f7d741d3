"""What the gap list and the holders query cost: milliseconds per kb_sim_gaps and kb_sim_holders on
the flagship state (configs[2], sim_sender, after the bench horizon of 20 rounds), beside the view census
(kb_sim_census) on the same state in the same run.

Every call is synchronous (it returns after its copies), so the wall time is a synchronised time.  `device_ms` is the
HIP-event time of the call's kernels (kb_sim_gaps_device_ms / kb_sim_holders_device_ms: the count and scan span plus
the listing span; the host's read of the totals between the two is not in it); `wall_ms` adds that read, the download
of the lists and the copies into the caller's arrays.  The calls are read-only, so each is repeated on one state: the
median of REPS calls after WARM warm-up calls.

gaps, three modes: totals only (no list asked for), both lists written (capacities = the totals), and both lists asked
for with capacities one below the totals (counted, not written).  holders: 1, 64 and 1,024 ids (the ghost ids first,
then running ids, ascending), rows written.

Algorithmic bytes of each pass (`bytes`): the count reads every observer's row once, observers x W / 8; the scan reads
4 and writes 8 bytes per row and list; the listing reads the rows that have a cell again (at most the count's bytes)
and writes 8 bytes per pair; the column pass touches one 4-byte word per (observer row, id): a 64-byte line each when
the ids are far apart, and writes ids x ceil(C / 64) x 8 bytes.

    python tools/gaps_cost.py [--out profiles/gaps_cost.json]
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
LIST_MAX = 1 << 25              # pairs: a longer list (256 MiB) is counted here, not written


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


def main() -> int:
    import ctypes as C
    import numpy as np
    from kaboodle_amd._ffi import KbGaps
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaps_cost.json"))
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "15", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    rounds = b.warmup + b.steps
    res = {"tool": "tools/gaps_cost.py", "hbm_peak_GBs": HBM_PEAK_GBS, "warm_up_calls": WARM,
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {rounds} rounds"}
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    with kaboodle_amd.Mesh(cfg) as m:
        m.step(rounds)
        cap = m.capacity
        width = -(-cap // 8192) * 8192
        cen = m.census()
        first = m.gaps(max_pairs=0)
        nm, ns, obs = first["missing"], first["stale"], first["observers"]
        res["summary"] = {k: v for k, v in first.items() if not k.endswith("_pairs")}
        res["census_summary"] = cen.summary
        res["totals_equal_census"] = (nm, ns) == (cen.summary["missing"], cen.summary["stale"])
        row_bytes = obs * width // 8
        view = repeated(lambda: m.census(arrays=False), m.census_device_ms)
        res["view_census_same_state"] = view
        out = KbGaps()
        lm, ls = (n if n <= LIST_MAX else 0 for n in (nm, ns))         # what the "both lists" mode asks for
        res["list_max_pairs"] = LIST_MAX
        bm, bs = np.zeros((max(lm, 1), 2), dtype=np.uint32), np.zeros((max(ls, 1), 2), dtype=np.uint32)

        def gaps(cm: int, cs: int):
            m.lib.call("sim_gaps", m.h, C.byref(out), p32(bm) if cm else None, cm, p32(bs) if cs else None, cs)

        modes = {"totals_only": (0, 0), "both_lists": (lm, ls), "lists_over_their_caps": (max(nm - 1, 0), max(ns - 1, 0))}
        res["gaps"] = {}
        for name, (cm, cs) in modes.items():
            f = repeated(lambda: gaps(cm, cs), m.gaps_device_ms)
            f["listed"] = [int(out.missing_listed), int(out.stale_listed)]
            listed = 8 * (f["listed"][0] + f["listed"][1])
            f["bytes"] = {"count_read": row_bytes, "scan": 2 * 12 * cap, "list_read_at_most": row_bytes if listed else 0,
                          "list_written": listed}
            f["count_achieved_GBs_at_most"] = round(row_bytes / (f["device_ms_median"] * 1e-3) / 1e9, 1)
            f["device_ms_over_view_census"] = round(f["device_ms_median"] / view["device_ms_median"], 3)
            f["wall_ms_over_view_census"] = round(f["wall_ms_median"] / view["wall_ms_median"], 3)
            res["gaps"][name] = f
        gaps(lm, ls)
        once = (bm.tobytes(), bs.tobytes())
        bm[:], bs[:] = 0, 0
        gaps(lm, ls)
        res["same_answer_every_call"] = once == (bm.tobytes(), bs.tobytes())
        for kind, buf, n, arr in (("missing", bm, lm, cen.missing), ("stale", bs, ls, cen.stale)):
            if n:                                                      # the listed rows' counts are the census's
                res[kind + "_rows_equal_census"] = bool(np.array_equal(np.bincount(buf[:n, 0], minlength=cap), arr))
        running = cen.running
        ghosts = np.flatnonzero(~running & (cen.known_by > 0))
        pool = np.concatenate([ghosts, np.flatnonzero(running)]).astype(np.uint32)
        res["holders"] = {}
        for n in (1, 64, 1024):
            ids = np.ascontiguousarray(pool[:n])
            total = int(cen.known_by[ids].sum())
            off, rows, got = np.zeros(n + 1, dtype=np.uint64), np.empty(max(total, 1), dtype=np.uint32), C.c_uint64(0)

            def holders():
                m.lib.call("sim_holders", m.h, p32(ids), n, off.ctypes.data_as(C.POINTER(C.c_uint64)), p32(rows), len(rows),
                           C.byref(got))

            f = repeated(holders, m.holders_device_ms)
            f["rows_listed"] = int(got.value)
            f["lengths_equal_known_by"] = bool(np.array_equal(np.diff(off).astype(np.uint32), cen.known_by[ids]))
            f["bytes"] = {"column_words_read": 4 * n * obs, "column_lines_touched_at_most": 64 * n * obs,
                          "table_written": n * -(-cap // 64) * 8, "rows_written": 4 * total}
            f["device_ms_over_view_census"] = round(f["device_ms_median"] / view["device_ms_median"], 3)
            f["wall_ms_over_view_census"] = round(f["wall_ms_median"] / view["wall_ms_median"], 3)
            res["holders"][f"ids_{n}"] = f
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
