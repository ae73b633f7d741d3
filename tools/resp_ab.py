"""One timed run of bench.py's workload with debug flags (dev tool; bench.py has no route for them): one JSON line.

    resp_ab.py FLAGS [DUMP_DIR|-] [bench.py options, e.g. --failed-mode socket_faithful]

The mesh is built by bench.rank_config (--gpus 1 --steps 20 --warmup 5 unless overridden) with debug_flags = FLAGS and
timed by bench.timed_rounds.  An A/B alternates fresh processes of this script: KB_LIB_PATH=<parent library> with
FLAGS 0, this library with FLAGS 0, this library with KB_DBG_RESP_SERIAL (2048); profiles/r08a_ab_resp_overlap.txt.
Fields: round_gpu_ms = the round's device time (events on the main stream); ms_per_step = wall time per step;
kernel_ms_per_round = each listed kernel's summed launch time per timed round (two launches of k_resp_wave and of
k_resp_node per round when the responses are split around A2; kernels on different streams overlap, so
these do not add up to the round); launches_per_round; paths = kb_sim_debug_paths.  DUMP_DIR: bench.py's --dump-outputs
arrays."""
import json
import os
import sys
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

KERNELS = ("k_rowpass", "k_resp_wave", "k_resp_node", "k_tick_scan", "k_tick_pre", "k_fold", "k_a3_exact", "k_fp_rows")


def main(argv):
    flags = int(argv[0], 0)
    dump = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"] + argv[2:])
    import torch
    import kaboodle_amd
    mesh = kaboodle_amd.Mesh(replace(bench.rank_config(a, 0, 1, 0), debug_flags=flags))
    mesh.step(a.warmup)
    torch.cuda.synchronize()
    mesh.reset_kernel_time()
    dt, _, _, st = bench.timed_rounds(mesh, a.steps, 1)
    ms, n = mesh.kernel_time(bench.KT_ROUND)
    bd = mesh.kernel_breakdown()
    if dump:
        bench.dump_outputs(mesh, st, dump)
    print(json.dumps({"flags": flags, "round_gpu_ms": ms / max(n, 1), "ms_per_step": dt / a.steps * 1e3,
                      "kernel_ms_per_round": {k: round(bd[k]["ms"] / a.steps, 4) for k in KERNELS if k in bd},
                      "launches_per_round": {k: bd[k]["launches"] / a.steps for k in KERNELS if k in bd},
                      "paths": mesh.debug_paths()}))


if __name__ == "__main__":
    main(sys.argv[1:])
