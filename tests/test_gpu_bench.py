"""bench.py end to end on an MI355X at a small size (2,048 peers, in this process): what a plain run and a
--full run put on the result line, and that --dump-outputs writes the same state from run to run."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--nodes", "2048"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config")
FULL_ONLY = ("convergence", "cpu_baseline", "modes", "seeds")
NAMES = ("stats", "peers_index", "fingerprints", "scalars", "rows_index", "rows_sample")


def _run(extra):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert bench.main(SMALL + extra) == 0
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return tmp_path_factory.mktemp("bench_dumps")


@pytest.fixture(scope="module")
def plain(dumps):
    """One plain run, shared: its result line (its outputs are under dumps/a)."""
    return _run(["--dump-outputs", str(dumps / "a")])


def test_plain_run(plain, dumps):
    out = plain
    assert all(k in out for k in HEADLINE)
    assert out["full"] is False and all(out[k] is None for k in FULL_ONLY)
    assert out["steps"] == 3 and out["warmup"] == 2 and out["unit"] == "peer-rounds/s" and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    a = _load(str(dumps / "a"))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["stats"][0] == 5                                       # kb_stats.round after 2 + 3 steps
    assert a["fingerprints"].shape == (out["config"]["capacity"],)
    assert a["scalars"].shape == (out["config"]["capacity"], 4)
    assert a["rows_sample"].shape == (len(a["rows_index"]), out["config"]["capacity"])
    assert a["rows_sample"].any() and a["fingerprints"].any()
    assert sum(os.path.getsize(os.path.join(dumps / "a", f)) for f in os.listdir(dumps / "a")) < 64 << 20


def test_dump_is_repeatable(plain, dumps):
    """The same arguments give the same outputs, array for array."""
    _run(["--dump-outputs", str(dumps / "b")])
    a, b = _load(str(dumps / "a")), _load(str(dumps / "b"))
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n


def test_full_run(plain, dumps):
    """--full adds the further measurements and leaves the timed path's outputs as a plain run's (the dump is
    taken before the convergence tail steps the mesh on)."""
    out = _run(["--full", "--cpu-seconds", "0.2", "--cpu1-seconds", "0", "--conv-cap", "4", "--seeds", "2",
                "--dump-outputs", str(dumps / "c")])
    assert all(k in out for k in HEADLINE) and out["full"] is True
    assert all(out[k] is not None for k in FULL_ONLY)
    assert out["cpu_baseline"]["value"] > 0 and set(out["seeds"]) == {"2"}
    assert {"socket_faithful", "window"} <= set(out["modes"])
    assert "k_proc" in out["kernels"]                               # from the profiled replay only
    a, c = _load(str(dumps / "a")), _load(str(dumps / "c"))
    for n in NAMES:
        assert np.array_equal(a[n], c[n]), n
