"""What a view-delta census costs: milliseconds per kb_sim_delta_census on the flagship state, and on
the same state as 8 in-process row shards, for a one-round delta and a 25-round delta, with and without
KB_DELTA_ADVANCE, beside the view census (kb_sim_census) on the same state in the same run.

Every call is synchronous (it returns after its copies), so the wall time is a synchronised time.  `device_ms` is
the time of the pass's kernels and the clearing of its scratch by HIP events (kb_sim_delta_device_ms); `wall_ms` adds
the copies to the host, the refresh of the running-set copy under ADVANCE and the O(ids) summary.  A read-only census
is repeated on one state (median of REPS after warm-up).  An advancing census changes its own baseline, so it cannot
be repeated on one state: the one-round figures are the median over ROUNDS consecutive rounds (one advancing call
each), the 25-round figure is a single call and is marked so.  The pass reads continuing rows x W/8 bytes from each
of the two tables; an advancing pass also stores the 8-byte groups that differ and copies the rows that began to run
(both bounded from the census's own counts).  Achieved GB/s is over the bytes read.

    python tools/delta_census_cost.py [--out profiles/delta_census_cost.json] [--skip-shards]
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
WARM, REPS, ROUNDS = 3, 20, 10


def once(fn, ms) -> tuple:
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3, ms()


def repeated(fn, ms) -> dict:
    for _ in range(WARM):
        fn()
    got = [once(fn, ms)[1:] for _ in range(REPS)]
    wall, dev = [g[0] for g in got], [g[1] for g in got]
    return {"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
            "device_ms_median": round(statistics.median(dev), 4), "device_ms_min": round(min(dev), 4), "repeats": REPS}


def traffic(mesh, summary: dict, arrays_sum: int) -> dict:
    width = -(-mesh.capacity // 8192) * 8192
    read = 2 * summary["continuing"] * width // 8
    return {"bytes_read": read, "advance_store_bytes_at_most": 8 * arrays_sum + summary["new_rows"] * width // 8,
            "advance_copy_read_bytes": summary["new_rows"] * width // 8}


def with_rate(fig: dict, nbytes: int) -> dict:
    ms = fig["device_ms_median"]
    fig["achieved_GBs"] = round(nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
    fig["frac_of_8TBs"] = round(fig["achieved_GBs"] / HBM_PEAK_GBS, 4) if ms > 0 else None
    return fig


def figures(cfg, rounds: int, shards: int) -> dict:
    """The state after `rounds` rounds: a one-round delta (mark after rounds - 1) with the view census as yardstick,
    then ROUNDS further rounds with one advancing census each; on a second mesh a delta over all `rounds` rounds."""
    out = {}
    dms = lambda m: m.delta_census_device_ms
    with kaboodle_amd.Mesh(cfg, shards=shards) as m:
        m.step(rounds - 1)
        m.delta_mark()
        m.step(1)
        d = m.delta_census(advance=False)
        tr = traffic(m, d.summary, int(d.gained.sum() + d.lost.sum()))
        view = repeated(lambda: m.census(arrays=False), m.census_device_ms)
        out["view_census_same_state"] = with_rate(view, tr["bytes_read"] // 2)
        ro = {"summary": d.summary, **tr, "summary_only": with_rate(repeated(lambda: m.delta_census(False, False), dms(m)), tr["bytes_read"]),
              "with_arrays": repeated(lambda: m.delta_census(False, True), dms(m))}
        ro["device_ms_over_view_census"] = round(ro["summary_only"]["device_ms_median"] / view["device_ms_median"], 3)
        out["one_round_read_only"] = ro
        wall, dev, read, changed = [], [], [], []
        for _ in range(ROUNDS):
            d, w, t = once(lambda: m.delta_census(True, True), dms(m))
            wall.append(w), dev.append(t), changed.append(int(d.gained.sum() + d.lost.sum()))
            read.append(traffic(m, d.summary, changed[-1])["bytes_read"])
            m.step(1)
        adv = {"rounds": ROUNDS, "changed_entries_median": int(statistics.median(changed)),
               "bytes_read_median": int(statistics.median(read)),
               "with_arrays": {"wall_ms_median": round(statistics.median(wall), 4), "device_ms_median": round(statistics.median(dev), 4),
                               "device_ms_min": round(min(dev), 4)}}
        with_rate(adv["with_arrays"], adv["bytes_read_median"])
        adv["device_ms_over_view_census"] = round(adv["with_arrays"]["device_ms_median"] / view["device_ms_median"], 3)
        out["one_round_advance"] = adv
    with kaboodle_amd.Mesh(cfg, shards=shards) as m:
        m.delta_mark()
        m.step(rounds)
        d = m.delta_census(advance=False)
        tr = traffic(m, d.summary, int(d.gained.sum() + d.lost.sum()))
        lr = {"summary": d.summary, **tr, "summary_only": with_rate(repeated(lambda: m.delta_census(False, False), dms(m)), tr["bytes_read"]),
              "with_arrays": repeated(lambda: m.delta_census(False, True), dms(m))}
        lr["device_ms_over_view_census"] = round(lr["summary_only"]["device_ms_median"] / out["view_census_same_state"]["device_ms_median"], 3)
        out[f"{rounds}_round_read_only"] = lr
        d2, w, t = once(lambda: m.delta_census(True, True), dms(m))
        out[f"{rounds}_round_advance"] = {"single_call": True, "wall_ms": round(w, 4), "device_ms": round(t, 4),
                                           "equals_read_only": not d2.same_as(d)}
        z = m.delta_census(advance=False)
        out[f"{rounds}_round_advance"]["then_zero"] = z.summary["changed_ids"] == 0 and z.summary["round_base"] == z.summary["round"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delta_census_cost.json"))
    ap.add_argument("--skip-shards", action="store_true")
    a = ap.parse_args()
    kaboodle_amd.require_gpu()
    b = bench.parse(["--steps", "20", "--warmup", "5"])
    cfg = bench.rank_config(b, 0, 1, 0)
    rounds = b.warmup + b.steps
    res = {"tool": "tools/delta_census_cost.py", "hbm_peak_GBs": HBM_PEAK_GBS, "rows_per_wave_env": os.environ.get("KB_DELTA_RPW"),
           "workload": f"configs[2]: {b.nodes} peers, capacity {cfg.capacity}, after {rounds} rounds"}
    res["dense"] = figures(cfg, rounds, 0)
    print(json.dumps(res["dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if not a.skip_shards:
        res["dense_8_local_shards"] = figures(cfg, rounds, 8)
        res["dense_8_local_shards"]["one_round_summary_equals_unsharded"] = (
            res["dense_8_local_shards"]["one_round_read_only"]["summary"] == res["dense"]["one_round_read_only"]["summary"])
        print(json.dumps(res["dense_8_local_shards"]), flush=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
