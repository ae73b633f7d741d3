"""CPU checks of bench.py's workload set-up (no GPU): the configuration the driver's command builds is the
one the full-size GPU parity test runs, and capacity does not depend on the step count."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _cfg(argv):
    return bench.rank_config(bench.parse(argv), 0, 1, 0)


def test_driver_config_is_the_parity_config():
    from test_gpu_fullsize import BENCH_CFG
    cfg = _cfg(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    for f in ("capacity", "initial_nodes", "init_mode", "loss", "churn", "fault_end_round", "seed", "failed_mode",
              "track_latency", "max_waves", "id_len", "variant"):
        assert getattr(cfg, f) == getattr(BENCH_CFG, f), f


def test_capacity_independent_of_steps():
    caps = {_cfg(["--steps", str(k), "--warmup", "5"]).capacity for k in (5, 20, 50)}
    assert caps == {65536 + bench.CHURN_RESERVE}


def test_plain_run_is_the_default():
    """--full is off unless asked for, and changes nothing about the timed workload."""
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    full = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert plain.full is False and plain.dump_outputs is None and full.full is True
    assert bench.rank_config(plain, 0, 1, 0) == bench.rank_config(full, 0, 1, 0)


def test_seeded_sample_is_fixed():
    import numpy as np
    assert np.array_equal(bench.seeded_sample(5, 8), np.arange(5))
    s = bench.seeded_sample(73728, 142)
    assert len(s) == 142 and len(np.unique(s)) == 142 and s.min() >= 0 and s.max() < 73728
    assert np.array_equal(s, np.sort(s)) and np.array_equal(s, bench.seeded_sample(73728, 142))


def test_dump_outputs_files(tmp_path):
    """--dump-outputs writes float arrays of the state after the last step; here through the oracle, which
    implements the same ABI (the GPU run of the same code: tests/test_gpu_bench.py)."""
    import numpy as np
    import parity
    from kaboodle_amd._ffi import KB_INIT_CONVERGED, Sim, SimConfig
    cfg = SimConfig(capacity=96, initial_nodes=64, init_mode=KB_INIT_CONVERGED, loss=0.02, churn=0.01, seed=3)
    with Sim(parity.oracle_lib(), cfg) as o:
        o.step(4)
        st = o.stats()
        bench.dump_outputs(o, st, str(tmp_path / "out"))
        got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in
               ("stats", "peers_index", "fingerprints", "scalars", "rows_index", "rows_sample")}
        assert all(v.dtype in (np.float32, np.float64) for v in got.values())
        assert np.array_equal(got["stats"], [st[k] for k in st]) and got["stats"][0] == 4       # round
        assert np.array_equal(got["peers_index"], np.arange(96)) and np.array_equal(got["rows_index"], np.arange(96))
        assert np.array_equal(got["fingerprints"], o.fingerprints())
        assert np.array_equal(got["scalars"], o.scalars())
        assert np.array_equal(got["rows_sample"], o.rows())


def test_dump_outputs_size_bound():
    """Under 64 MB in all at the benched size and at configs[3]'s 1M ids."""
    for cap in (65536 + bench.CHURN_RESERVE, 1 << 20):
        peers = len(bench.seeded_sample(cap, bench.DUMP_PEERS))
        rows = len(bench.seeded_sample(cap, max(1, bench.DUMP_ROW_BYTES // (4 * cap))))
        assert 8 * 40 + peers * 8 * 6 + rows * 8 + rows * cap * 4 < 64 << 20


def test_records_match_by_binary_or_sources(tmp_path, monkeypatch):
    """bench.py attaches a PMC or convergence record made with this library: the same binary, or (hipcc's output
    is not byte-reproducible) the same build inputs; a change to any input changes the source identity."""
    import pytest
    import kaboodle_amd
    from kaboodle_amd import build as kb_build
    if not os.path.exists(kaboodle_amd.LIB_PATH):
        pytest.skip("library not built")
    src = kb_build.src_sha16()
    assert src == kb_build.src_sha16() and len(src) == 16
    assert bench.same_build({"lib_sha16": bench.lib_sha16()})
    assert bench.same_build({"lib_sha16": "0" * 16, "lib_src_sha16": src})
    assert not bench.same_build({"lib_sha16": "0" * 16, "lib_src_sha16": "0" * 16})
    assert not bench.same_build({"lib_sha16": "0" * 16})
    dep = tmp_path / "kb_extra.h"
    dep.write_text("// a build input\n")
    monkeypatch.setattr(kb_build, "deps", lambda: [kb_build.SRC, str(dep)])
    a = kb_build.src_sha16()
    dep.write_text("// a build input, changed\n")
    assert kb_build.src_sha16() != a
