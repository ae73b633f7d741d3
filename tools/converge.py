"""Rounds to fingerprint convergence of the bench workload (BASELINE.json metric, second half).

    python tools/converge.py [--mode sim|sock] [--nodes 65536] [--faults 25] [--cap-factor 2] [--out FILE]

Runs configs[2] exactly as bench.py does (converged start, 1 % loss, 0.1 %/round churn, faults until
round F = 25 = warmup + steps of the driver's bench), then keeps stepping the quiescent tail (no loss,
no churn) on the GPU until every live peer's fingerprint equals the fingerprint of the true live set
(kb_stats.agree == alive) or the cap of cap_factor * N rounds.  Every 256 tail rounds it
records the agreement and the mean view-size gap |known_i| - live into the trajectory and prints a
progress line.  `--mode sock` = failed_mode socket_faithful (Failed never honoured, as over real
sockets: src/networking.rs:44-55); `sim` = sim_sender (honoured).

A run that ends without agreement (the cap or the budget), or any run with --reciprocity, records the reciprocity
census of its last state (include/kaboodle_reciprocity.h) in the result: the summary and, when it
fits --max-pairs, the list of mutual pairs — the gaps that can never heal — in place of the eight hand-sampled
views earlier records carry, and beside it the view census's summary, which keeps what those
views also showed: the stale entries and the ghosts (non-running ids some view still holds).  Beside the two it
records the fingerprint-class census (include/kaboodle_classes.h): its summary and the 8 largest
classes as (fp, size, rep).  With --track-latency the mesh keeps PeerInfo.latency and the record carries the latency
census's summary too (include/kaboodle_latency.h).  The island census's summary
(include/kaboodle_islands.h) goes with them: whether the camps the classes show can still merge (one
island) or are sealed off from each other (several).  Last come the cells themselves (include/kaboodle_gaps.h,
DESIGN.md §21): the gap lists, each when it is at most 65,536 pairs, and the rows that still hold the top ghost.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kb_src_sha16():
    """the sources the in-tree library is built from (None for an A/B build loaded through KB_LIB_PATH)"""
    import kaboodle_amd
    from kaboodle_amd import build as kb_build
    return kb_build.src_sha16() if os.path.abspath(kaboodle_amd.LIB_PATH) == os.path.abspath(kb_build.OUT) else None


def lib_sha16() -> str:
    """the library build this record was made with (bench.py attaches a tail record only when it matches)"""
    import hashlib
    import kaboodle_amd
    return hashlib.sha256(open(kaboodle_amd.LIB_PATH, "rb").read()).hexdigest()[:16]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("sim", "sock"), default="sim")
    ap.add_argument("--nodes", type=int, default=65536)
    ap.add_argument("--faults", type=int, default=25)
    ap.add_argument("--cap-factor", type=float, default=2.0)
    ap.add_argument("--every", type=int, default=256)
    ap.add_argument("--budget-s", type=float, default=1e9, help="stop early after this many seconds")
    ap.add_argument("--lru", choices=("window", "exact"), default="window",
                    help="A3's order: the 1-byte stamp window with the sweep front (declared), or the exact instants "
                         "(KB_VARIANT_EXACT_LRU, src/kaboodle.rs:662-675)")
    ap.add_argument("--reciprocity", action="store_true",
                    help="record the reciprocity census of the last state even when the run converged")
    ap.add_argument("--max-pairs", type=int, default=65536, help="mutual pairs listed in the result at most")
    ap.add_argument("--track-latency", action="store_true",
                    help="keep PeerInfo.latency (track_latency 1) and record the latency census beside the others")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import kaboodle_amd
    from kaboodle_amd._ffi import (KB_FAILED_SIM_SENDER, KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED, KB_VARIANT_EXACT_LRU,
                                   SimConfig)
    kaboodle_amd.require_gpu()
    n, F = a.nodes, a.faults
    cfg = SimConfig(capacity=n + max(4096, int(n * 0.001 * (F + 8) * 1.5)), initial_nodes=n,
                    init_mode=KB_INIT_CONVERGED, loss=0.01, churn=0.001, fault_end_round=F, seed=1,
                    failed_mode=KB_FAILED_SOCKET_FAITHFUL if a.mode == "sock" else KB_FAILED_SIM_SENDER,
                    variant=KB_VARIANT_EXACT_LRU if a.lru == "exact" else 0, track_latency=int(a.track_latency))
    cap = int(a.cap_factor * n)
    t0 = time.time()
    traj = []

    def sample(m, r):
        st = m.stats()
        sc = m.scalars()
        live = sc[:, 0] != 0
        gap = sc[live, 1].astype(np.int64) - int(live.sum())
        rec = {"round": r, "agree": st["agree"], "alive": st["alive"], "agree_frac": round(st["agree"] / max(st["alive"], 1), 6),
               "view_gap_mean": round(float(np.abs(gap).mean()), 2), "view_gap_signed_mean": round(float(gap.mean()), 2),
               "view_exact_frac": round(float((gap == 0).mean()), 6), "wall_s": round(time.time() - t0, 1)}
        traj.append(rec)
        return st

    conv = None
    with kaboodle_amd.Mesh(cfg) as m:
        m.step(F)
        st = sample(m, F - 1)
        print(f"[converge {a.mode}] faults over at round {F}: agree {st['agree']}/{st['alive']}", flush=True)
        r = F
        while r < F + cap and time.time() - t0 < a.budget_s:
            m.step(1)
            s = m.stats()
            if s["alive"] and s["agree"] == s["alive"]:
                conv = r
                sample(m, r)
                break
            r += 1
            if (r - F) % a.every == 0:
                st = sample(m, r - 1)
                print(f"[converge {a.mode}] round {r - 1}: agree {st['agree']}/{st['alive']}, "
                      f"mean view gap {traj[-1]['view_gap_mean']}, {time.time() - t0:.0f} s", flush=True)
        if conv is None:
            sample(m, r - 1)
        recip = None
        if conv is None or a.reciprocity:
            # what is left: how much of the disagreement is permanent (mutual gaps never heal) and
            # between which pairs
            rc = m.reciprocity(max_pairs=a.max_pairs)
            recip = {"summary": rc.summary, "census": m.census(arrays=False).summary, "mutual_pairs": rc.pairs.tolist(),
                     "rows_lacked_by": int((rc.lacked_by > 0).sum()), "device_ms": round(m.reciprocity_device_ms(), 4)}
            print(f"[converge {a.mode}] reciprocity: {json.dumps(rc.summary)}", flush=True)
            print(f"[converge {a.mode}] census: {json.dumps(recip['census'])}", flush=True)
            # and which camps the views fall into: one second fingerprint shared by the stragglers, or each alone
            fc = m.fp_classes(top=8, arrays=False)
            recip["fp_classes"] = {"summary": fc.summary, "top_classes": fc.classes.tolist(),
                                   "device_ms": round(m.fp_classes_device_ms(), 4)}
            print(f"[converge {a.mode}] fp classes: {json.dumps(recip['fp_classes'])}", flush=True)
            # and whether those camps can still reach each other: one island can converge, several cannot
            recip["islands"] = {"summary": m.islands(arrays=False).summary, "device_ms": round(m.islands_device_ms(), 4)}
            print(f"[converge {a.mode}] islands: {json.dumps(recip['islands'])}", flush=True)
            # and the cells themselves (include/kaboodle_gaps.h): which row lacks which running id and
            # still holds which dead one, each list when it is at most 65,536 pairs, and who holds the top ghost
            gp = m.gaps(max_pairs=65536)
            pairs = {k: None if gp[k] is None else gp[k].tolist() for k in ("missing_pairs", "stale_pairs")}
            recip["gaps"] = {"summary": {k: v for k, v in gp.items() if k not in pairs}, **pairs,
                             "device_ms": round(m.gaps_device_ms(), 4)}
            ghost = recip["census"]["top_ghost"]
            if ghost != 0xFFFFFFFF:                                    # KB_CENSUS_NONE: no dead id is held
                recip["gaps"]["top_ghost_holders"] = {"id": ghost, "rows": m.holders([ghost])[1].tolist(),
                                                      "device_ms": round(m.holders_device_ms(), 4)}
            print(f"[converge {a.mode}] gaps: {json.dumps(recip['gaps']['summary'])}", flush=True)
            if cfg.track_latency:
                recip["latency_census"] = {"summary": m.latency_census(arrays=False).summary,
                                           "device_ms": round(m.latency_census_device_ms(), 4)}
                print(f"[converge {a.mode}] latency census: {json.dumps(recip['latency_census'])}", flush=True)
    out = {"workload": f"configs[2]: {n} peers, converged start, 1% loss, 0.1%/round churn, faults until round {F}",
           "failed_mode": "socket_faithful" if a.mode == "sock" else "sim_sender", "fault_end_round": F,
           "a3_order": a.lru,
           "converged_round": conv, "tail_rounds_to_converge": None if conv is None else conv - F + 1,
           "tail_rounds_run": traj[-1]["round"] - F + 1, "cap_rounds": cap,
           "stopped_by": "converged" if conv is not None else ("cap" if traj[-1]["round"] >= F + cap - 1 else "budget"),
           "wall_s": round(time.time() - t0, 1), "lib_sha16": lib_sha16(), "lib_src_sha16": kb_src_sha16(), "reciprocity": recip,
           "trajectory": traj}
    txt = json.dumps(out)
    print(json.dumps({k: v for k, v in out.items() if k not in ("trajectory", "reciprocity")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
