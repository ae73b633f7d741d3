"""The view census on the GPU (kb_sim_census, include/kaboodle_census.h; kernels in kaboodle_amd/csrc/kb_census.h):
the dense engine's bit-sliced column count and the sparse rows' exception count against the CPU oracle's
census every round, under every variant that shares the tables, past 16-bit counts, and read-only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_FAILED_SOCKET_FAITHFUL, KB_INIT_CONVERGED, KB_INVALID_ARGUMENT,
                               KB_VARIANT_EXACT_LRU, KB_VARIANT_SPARSE_ROWS, KbCensus, KbError, Sim, SimConfig,
                               rccl_unique_id)
from kaboodle_amd.census import census_ref

pytestmark = pytest.mark.gpu

STD = {n: (c, r) for n, c, r in parity.standard_cases()}
# capacity 2,100: ids past the first 2,048, rows that span several fold periods of the column counters, churn
BIG = ({"cfg": SimConfig(capacity=2100, initial_nodes=2000, init_mode=KB_INIT_CONVERGED, loss=0.02, churn=0.01,
                         seed=21)}, 6)
DENSE_CASES = {**{n: STD[n] for n in ("config1_2x2", "join_loss_300_ids", "churn_loss_512", "stop_start",
                                      "partition_heal", "fresh_ids")}, "churn_2100": BIG}
SPARSE_CASES = {n: DENSE_CASES[n] for n in DENSE_CASES if n != "churn_2100"}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    lib = parity.gpu_lib()
    return lib


def has_kernel(lib) -> None:
    assert "sim_census" in lib.fn                       # the numpy fallback cannot stand in for the kernel


def sparse(case: dict, **kw) -> dict:
    return parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0, **kw)


_ORACLE: dict = {}


def oracle_censuses(key: str, case: dict, rounds: int, first: int = 0):
    """The oracle's census after every round >= first of the case: computed once, shared, never changed."""
    if key not in _ORACLE:
        out = []
        with Sim(parity.oracle_lib(omp=case["cfg"].capacity >= 2048), case["cfg"]) as o:
            assert "sim_census" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.census() if r >= first else None)
        _ORACLE[key] = out
    return _ORACLE[key]


def run_against(gpu, key: str, case: dict, rounds: int, gcase: dict | None = None, shards: int = 0, first: int = 0,
                handle: Sim | None = None):
    """GPU census() == oracle census() (summary and the three arrays) after every round >= first; gcase = the case
    as the GPU runs it when only flags the oracle ignores differ."""
    has_kernel(gpu)
    want = oracle_censuses(key, case, rounds, first)
    gc = gcase or case
    g = handle if handle is not None else Sim(gpu, gc["cfg"], shards=shards)
    parity.setup(g, gc)
    for r in range(rounds):
        parity.apply_events((g,), gc, r)
        g.step(1)
        if r >= first:
            d = g.census().same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
    g.close()


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_census_equals_oracle_every_round(gpu, name):
    case, rounds = DENSE_CASES[name]
    run_against(gpu, "dense:" + name, case, rounds)


def test_dense_census_exact_lru(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "dense-lru:churn_loss_512", parity.with_cfg(case, variant=KB_VARIANT_EXACT_LRU), rounds)


def test_dense_census_wide_row_flags(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "dense:churn_loss_512", case, rounds, gcase=parity.with_cfg(case, debug_flags=KB_DBG_ALL))


def test_dense_census_three_shards(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "dense:churn_loss_512", case, rounds, shards=3)


@pytest.mark.parametrize("shards", [0, 3], ids=["unsharded", "shards3"])
@pytest.mark.parametrize("name", list(SPARSE_CASES))
def test_sparse_census_equals_oracle_every_round(gpu, name, shards):
    case, rounds = SPARSE_CASES[name]
    if shards and case["cfg"].capacity < shards * 2:
        shards = 2                                       # config1_2x2: 4 ids make 2 shards of 2 rows
    run_against(gpu, "sparse:" + name, sparse(case), rounds, shards=shards)


def partition_case(n: int, every: int, seed: int = 9) -> dict:
    """configs[4]'s scenario at n peers (as tests/test_gpu_sparse.py builds it): converged start, 5 % loss, two
    halves cut off for rounds 3-11, healed at round 12 by every `every`-th peer pinging the other half."""
    cfg = SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, loss=0.05, partition_groups=2,
                    partition_start=3, partition_end=12, seed=seed, failed_mode=KB_FAILED_SOCKET_FAITHFUL,
                    variant=KB_VARIANT_SPARSE_ROWS)
    return {"cfg": cfg, "events": {12: [("ping", i, [(i + n // 2) % n]) for i in range(0, n, every)]}}


def test_sparse_census_across_the_heal(gpu):
    run_against(gpu, "sparse:partition_2048", partition_case(2048, 64), 17, first=10)


def test_sparse_counts_past_16_bits(gpu):
    has_kernel(gpu)
    n = 66000
    with Sim(gpu, SimConfig(capacity=n, initial_nodes=n, init_mode=KB_INIT_CONVERGED, variant=KB_VARIANT_SPARSE_ROWS)) as g:
        g.step(1)
        c = g.census()
        assert (c.known_by == n).all() and not c.missing.any() and not c.stale.any()
        s = c.summary
        assert s["observers"] == s["running"] == s["exact_views"] == s["full_ids"] == n
        assert s["pairs"] == n * n and s["ghost_ids"] == 0


def test_dense_counts_past_16_bits(gpu):
    """The one full-size case: 65,536 observers is the smallest mesh where a 16-bit partial count would wrap."""
    has_kernel(gpu)
    n = 65536
    with Sim(gpu, SimConfig(capacity=69632, initial_nodes=n, init_mode=KB_INIT_CONVERGED, track_latency=0)) as g:
        g.step(1)
        c = g.census()
        assert (c.known_by[:n] == n).all() and not c.known_by[n:].any()
        assert not c.missing.any() and not c.stale.any()
        s = c.summary
        assert s["observers"] == s["running"] == s["exact_views"] == s["full_ids"] == n
        assert s["pairs"] == n * n and s["ghost_ids"] == 0 and (s["least_known"], s["least_known_by"]) == (0, n)


@pytest.mark.parametrize("variant", [0, KB_VARIANT_SPARSE_ROWS], ids=["dense", "sparse"])
def test_census_is_read_only(gpu, variant):
    has_kernel(gpu)
    case, rounds = STD["churn_loss_512"]
    case = sparse(case) if variant else case
    a, b = Sim(gpu, case["cfg"]), Sim(gpu, case["cfg"])
    for r in range(rounds):
        a.step(1)
        b.step(1)
        a.census()
        d = parity.diff_states(parity.state_of(a), parity.state_of(b))
        assert not d, f"round {r}: " + "; ".join(d[:6])
    a.close()
    b.close()


def test_dense_census_self_consistent(gpu):
    has_kernel(gpu)
    case, rounds = BIG
    with Sim(gpu, case["cfg"]) as g:
        g.step(rounds)
        c = g.census()
        d = c.same_as(census_ref(g))
        assert not d, "; ".join(d[:6])
        assert int(c.known_by.sum(dtype=np.uint64)) == c.summary["pairs"]
        assert int(c.missing.sum(dtype=np.uint64)) == c.summary["missing"] > 0
        assert int(c.stale.sum(dtype=np.uint64)) == c.summary["stale"] > 0
        assert g.census(arrays=False).summary == c.summary          # NULL arrays: the summary alone
        assert 0.0 < g.census_device_ms() < 1000.0                  # the measurement hook reports the last census


def test_census_arguments(gpu):
    has_kernel(gpu)
    case, rounds = STD["stop_start"]
    want = oracle_censuses("dense:stop_start", case, rounds)
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as g:
        out = KbCensus()
        buf = np.zeros(cap, dtype=np.uint32)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        g.lib.call("sim_census", g.h, C.byref(out), None, 0, None, None, 0)                 # every array NULL
        g.lib.call("sim_census", g.h, C.byref(out), None, 0, None, ptr, cap)                # stale alone
        for args in ((ptr, cap - 1, None, None, 0), (None, 0, ptr, None, cap - 1), (None, 0, None, ptr, cap - 1)):
            with pytest.raises(KbError) as e:
                g.lib.call("sim_census", g.h, C.byref(out), *args)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:
            g.lib.call("sim_census", g.h, None, None, 0, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
    # a rank-style handle of a one-rank world answers as the unsharded mesh does
    run_against(gpu, "dense:stop_start", case, rounds,
                handle=Sim(gpu, case["cfg"], rank=0, world=1, uid=rccl_unique_id(gpu)))
    assert want is _ORACLE["dense:stop_start"]
