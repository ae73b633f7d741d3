"""The latency census on the GPU (kb_sim_latency_census, include/kaboodle_latency.h; kernel in
kaboodle_amd/csrc/kb_latcensus.h): the streaming pass over the latency table against the CPU oracle's reference
census every round, under every variant that shares the table, as row shards, on crafted tables past 32-bit sums and
65,536 rows, and read-only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_INIT_CONVERGED, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_EXACT_LRU, KB_VARIANT_SPARSE_ROWS, KbError, KbLatCensus, Sim, SimConfig,
                               latency_census_of, rccl_unique_id)
from kaboodle_amd.latency import KB_CENSUS_NONE, KB_LAT_HIST, latency_census_of_arrays

pytestmark = pytest.mark.gpu

NONE = KB_CENSUS_NONE
L = 0xFFFF
STD = {n: (c, r) for n, c, r in parity.standard_cases()}
# capacity 2,100: ids past the first 2,048, five peer slabs, two row tiles, churn
BIG = ({"cfg": SimConfig(capacity=2100, initial_nodes=2000, init_mode=KB_INIT_CONVERGED, loss=0.02, churn=0.01,
                         seed=21)}, 6)
NAMES = ("config1_2x2", "join_loss_300_ids", "churn_loss_512", "socket_faithful", "partition_heal", "stop_start",
         "fresh_ids")
CASES = {**{n: STD[n] for n in NAMES}, "churn_2100": BIG}


def tracked(case: dict, **kw) -> dict:
    return parity.with_cfg(case, track_latency=1, **kw)


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def has_kernel(lib) -> None:
    assert "sim_latency_census" in lib.fn               # the numpy fallback cannot stand in for the kernel


def test_library_exports_the_census(gpu):
    has_kernel(gpu)
    assert "sim_latency_census_device_ms" in gpu.fn and "latency_census_of" in gpu.fn


_ORACLE: dict = {}


def oracle_censuses(key: str, case: dict, rounds: int):
    """The oracle's reference census after every round of the case: computed once, shared, never changed."""
    if key not in _ORACLE:
        out = []
        with Sim(parity.oracle_lib(omp=case["cfg"].capacity >= 2048), case["cfg"]) as o:
            assert "sim_latency_census" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.latency_census())
        _ORACLE[key] = out
    return _ORACLE[key]


def run_against(gpu, key: str, case: dict, rounds: int, gcase: dict | None = None, shards: int = 0):
    """GPU latency_census() == the oracle's (summary and the six arrays) and orphans == 0 after every round; gcase =
    the case as the GPU runs it when only flags the oracle ignores differ."""
    has_kernel(gpu)
    want = oracle_censuses(key, case, rounds)
    gc = gcase or case
    assert gc["cfg"].track_latency == 1
    measured = 0
    with Sim(gpu, gc["cfg"], shards=shards) as g:
        parity.setup(g, gc)
        for r in range(rounds):
            parity.apply_events((g,), gc, r)
            g.step(1)
            c = g.latency_census()
            assert c.summary["orphans"] == 0, f"{key} round {r}: {c.summary['orphans']} orphans"
            d = c.same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
            measured += c.summary["measured"]
    assert measured > 0, key                             # the case exercises the table at all


@pytest.mark.parametrize("name", list(CASES))
def test_latency_census_equals_oracle_every_round(gpu, name):
    case, rounds = CASES[name]
    run_against(gpu, "lat:" + name, tracked(case), rounds)


def test_latency_census_exact_lru(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "lat-lru:churn_loss_512", tracked(case, variant=KB_VARIANT_EXACT_LRU), rounds)


def test_latency_census_wide_row_flags(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "lat:churn_loss_512", tracked(case), rounds, gcase=tracked(case, debug_flags=KB_DBG_ALL))


def test_latency_census_three_shards(gpu):
    case, rounds = STD["churn_loss_512"]                 # 640 ids: 214 rows a shard, stride 216 (2 padding rows)
    run_against(gpu, "lat:churn_loss_512", tracked(case), rounds, shards=3)


def test_latency_census_two_shards_of_two_rows(gpu):
    case, rounds = STD["config1_2x2"]
    run_against(gpu, "lat:config1_2x2", tracked(case), rounds, shards=2)


def test_latency_census_is_read_only(gpu):
    has_kernel(gpu)
    case, rounds = STD["churn_loss_512"]
    case = tracked(case)
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as a, Sim(gpu, case["cfg"]) as b:
        for r in range(rounds):
            a.step(1)
            b.step(1)
            a.latency_census()
            a.latency_census(arrays=False)
            assert a.stats() == b.stats(), f"round {r}: kb_stats differ"
            d = parity.diff_states(parity.state_of(a), parity.state_of(b))
            if not d and (r % 8 == 7 or r == rounds - 1):
                d = parity.diff_peer_states(b, a, range(cap))
            assert not d, f"round {r}: " + "; ".join(d[:6])


# ---- kb_latency_census_of on crafted tables ----------------------------------------------------------------
def check_of(gpu, lat, member, running):
    """The kernel's census of the arrays == the numpy reference's, with and without the arrays."""
    has_kernel(gpu)
    got = latency_census_of(gpu, lat, member, running)
    want = latency_census_of_arrays(lat, member, running)
    d = got.same_as(want)
    assert not d, "; ".join(d[:6])
    assert latency_census_of(gpu, lat, member, running, arrays=False).summary == want.summary
    return got


def test_of_sums_past_32_bits_and_rows_past_65536(gpu):
    n_ids, n_rows = 2, 70000
    lat = np.full((n_ids, n_rows), 65534, dtype=np.uint16)
    c = check_of(gpu, lat, np.ones((n_rows, n_ids), dtype=np.uint8), np.ones(n_rows, dtype=np.uint8))
    s = c.summary
    assert c.sum_ms.tolist() == [4587380000, 4587380000] and c.measured_by.tolist() == [70000, 70000]
    assert s["measured"] == 140000 and s["hist"][16] == 140000 and sum(s["hist"]) == 140000
    assert s["sum_ms"] == 2 * 4587380000 and (s["min_ms"], s["max_ms"], s["max_peer"]) == (65534, 65534, 0)
    assert (c.row_sum_ms == 131068).all() and (c.measured == 2).all() and s["orphans"] == 0


def test_of_orphans_are_counted_nowhere_else(gpu):
    rng = np.random.default_rng(5)
    n_ids, n_rows = 140, 77
    lat = rng.integers(0, 3000, size=(n_ids, n_rows)).astype(np.uint16)
    lat[rng.random((n_ids, n_rows)) < 0.5] = L
    member = (rng.random((n_rows, n_ids)) < 0.6).astype(np.uint8)
    run = np.ones(n_rows, dtype=np.uint8)
    c = check_of(gpu, lat, member, run)
    orphans = int(((lat != L) & (member.T == 0)).sum())
    assert c.summary["orphans"] == orphans > 0
    assert c.summary["measured"] == int(((lat != L) & (member.T != 0)).sum()) == int(c.measured_by.sum())
    # a table of orphans alone: everything else stays empty
    e = check_of(gpu, lat, np.zeros_like(member), run)
    assert e.summary["orphans"] == int((lat != L).sum()) and e.summary["measured"] == 0
    assert e.summary["hist"] == [0] * KB_LAT_HIST and not e.measured.any() and (e.min_ms == NONE).all()


def test_of_rows_that_do_not_run_are_ignored(gpu):
    n_ids, n_rows = 40, 530
    lat = np.full((n_ids, n_rows), 7, dtype=np.uint16)
    member = np.ones((n_rows, n_ids), dtype=np.uint8)
    member[:, ::3] = 0                                   # values under clear bits too: not orphans of a stopped row
    run = np.zeros(n_rows, dtype=np.uint8)
    c = check_of(gpu, lat, member, run)
    assert c.summary["observers"] == 0 and c.summary["measured"] == 0 and c.summary["orphans"] == 0
    run[[0, 7, 8, 511, 512, 529]] = 1                    # lane, wave and padding boundaries
    c = check_of(gpu, lat, member, run)
    assert c.summary["observers"] == 6 and np.flatnonzero(c.measured).tolist() == [0, 7, 8, 511, 512, 529]
    assert c.summary["orphans"] == 6 * len(range(0, n_ids, 3))


def test_of_an_all_none_table(gpu):
    n_ids, n_rows = 33, 9
    c = check_of(gpu, np.full((n_ids, n_rows), L, dtype=np.uint16), np.ones((n_rows, n_ids), dtype=np.uint8),
                 np.ones(n_rows, dtype=np.uint8))
    s = c.summary
    assert (s["min_ms"], s["max_ms"], s["max_peer"], s["measured"], s["measured_ids"]) == (NONE, 0, NONE, 0, 0)
    assert (c.min_ms == NONE).all() and not c.max_ms.any() and s["observers"] == n_rows


@pytest.mark.parametrize("n_ids", [1, 33, 2049])
@pytest.mark.parametrize("n_rows", [1, 7, 9, 513])
def test_of_sizes_off_every_multiple(gpu, n_ids, n_rows):
    rng = np.random.default_rng(n_ids * 1000 + n_rows)
    lat = rng.integers(0, 65535, size=(n_ids, n_rows)).astype(np.uint16)
    lat[rng.random((n_ids, n_rows)) < 0.7] = L
    member = (rng.random((n_rows, n_ids)) < 0.8).astype(np.uint8)
    run = (rng.random(n_rows) < 0.85).astype(np.uint8)
    run[-1] = 1                                          # the last row before the padding counts
    member[-1, -1] = 1
    lat[-1, -1] = 65534                                  # ... and so does the last id before the padding columns
    c = check_of(gpu, lat, member, run)
    assert c.max_ms[-1] == 65534 and c.measured[-1] >= 1


def test_of_one_value_per_bucket_edge(gpu):
    vals = sorted({0, 1, 65534} | {v for k in range(1, 16) for v in ((1 << k) - 1, 1 << k)})
    n_ids, n_rows = len(vals), 3
    lat = np.full((n_ids, n_rows), L, dtype=np.uint16)
    lat[np.arange(n_ids), np.arange(n_ids) % n_rows] = vals
    c = check_of(gpu, lat, np.ones((n_rows, n_ids), dtype=np.uint8), np.ones(n_rows, dtype=np.uint8))
    assert c.summary["hist"] == [1, 1] + [2] * 15 and c.max_ms.tolist() == vals
    assert (c.summary["min_ms"], c.summary["max_peer"]) == (0, n_ids - 1)


# ---- refusals and sizes ------------------------------------------------------------------------------------
def test_handles_that_keep_no_table_refuse(gpu):
    has_kernel(gpu)
    cfg = STD["stop_start"][0]["cfg"]
    from dataclasses import replace
    handles = {
        "sparse": lambda: Sim(gpu, replace(cfg, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0)),
        "untracked": lambda: Sim(gpu, replace(cfg, track_latency=0)),
        "rank": lambda: Sim(gpu, replace(cfg, track_latency=1), rank=0, world=1, uid=rccl_unique_id(gpu)),
    }
    for name, make in handles.items():
        with make() as g:
            g.step(1)
            out = KbLatCensus()
            rc = gpu.fn["sim_latency_census"](g.h, C.byref(out), None, None, None, None, 0, None, None, 0)
            assert rc == KB_INVALID_OPERATION, name
            assert gpu.fn["last_error"](), name          # a non-empty kb_last_error text
            with pytest.raises(KbError) as e:
                g.latency_census()
            assert e.value.code == KB_INVALID_OPERATION, name


def test_census_arguments(gpu):
    has_kernel(gpu)
    case, rounds = STD["stop_start"]
    case = tracked(case)
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as g:
        g.step(rounds)
        full = g.latency_census()
        assert full.summary["measured"] > 0
        assert g.latency_census(arrays=False).summary == full.summary      # all arrays NULL: the summary alone
        assert 0.0 < g.latency_census_device_ms() < 1000.0
        out = KbLatCensus()
        b32, b64 = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64)
        p32, p64 = b32.ctypes.data_as(C.POINTER(C.c_uint32)), b64.ctypes.data_as(C.POINTER(C.c_uint64))
        g.lib.call("sim_latency_census", g.h, C.byref(out), None, None, None, p32, cap, None, None, 0)   # max_ms alone
        assert np.array_equal(b32, full.max_ms)
        g.lib.call("sim_latency_census", g.h, C.byref(out), None, None, None, None, 0, None, p64, cap)   # row sums alone
        assert np.array_equal(b64, full.row_sum_ms)
        short = ((p32, None, None, None, cap - 1, None, None, 0), (None, p64, None, None, cap - 1, None, None, 0),
                 (None, None, None, p32, cap - 1, None, None, 0), (None, None, None, None, 0, p32, None, cap - 1),
                 (None, None, None, None, 0, None, p64, cap - 1))
        for args in short:
            with pytest.raises(KbError) as e:
                g.lib.call("sim_latency_census", g.h, C.byref(out), *args)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:
            g.lib.call("sim_latency_census", g.h, None, None, None, None, None, 0, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
