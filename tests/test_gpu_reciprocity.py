"""The reciprocity census on the GPU (kb_sim_reciprocity, include/kaboodle_reciprocity.h; kernels in
kaboodle_amd/csrc/kb_recip.h): the blocked transpose-and-count pass against the CPU oracle's numpy count every
round, under every variant that shares the member bits, past one row stride, past 32-bit totals, and read-only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_INIT_CONVERGED, KB_INIT_JOIN, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_EXACT_LRU, KB_VARIANT_SPARSE_ROWS, KbError, KbReciprocity, Sim, SimConfig,
                               rccl_unique_id)

pytestmark = pytest.mark.gpu

STD = {n: (c, r) for n, c, r in parity.standard_cases()}
# capacity 2,100 (as tests/test_gpu_census.py defines it): ids past the first 2,048, several row blocks, churn
BIG = ({"cfg": SimConfig(capacity=2100, initial_nodes=2000, init_mode=KB_INIT_CONVERGED, loss=0.02, churn=0.01,
                         seed=21)}, 6)
# past one 8,192-id row stride (W = 16,384): the block and W-stride edges, off-diagonal blocks in both orders
STRIDE = ({"cfg": SimConfig(capacity=8300, initial_nodes=8200, init_mode=KB_INIT_CONVERGED, loss=0.02, churn=0.01,
                            seed=23)}, 3)
CASES = {**{n: STD[n] for n in ("config1_2x2", "join_loss_300_ids", "churn_loss_512", "stop_start", "partition_heal",
                                "fresh_ids")}, "churn_2100": BIG, "stride_8300": STRIDE}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def has_kernel(lib) -> None:
    assert "sim_reciprocity" in lib.fn                  # the numpy fallback cannot stand in for the kernel


_ORACLE: dict = {}


def oracle_results(key: str, case: dict, rounds: int):
    """The oracle's reciprocity census after every round of the case: computed once, shared, never changed."""
    if key not in _ORACLE:
        out = []
        with Sim(parity.oracle_lib(omp=case["cfg"].capacity >= 2048), case["cfg"]) as o:
            assert "sim_reciprocity" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.reciprocity())
        _ORACLE[key] = out
    return _ORACLE[key]


def run_against(gpu, key: str, case: dict, rounds: int, gcase: dict | None = None, shards: int = 0):
    """GPU reciprocity() == oracle reciprocity() (summary, the three arrays, the pair list) after every round;
    gcase = the case as the GPU runs it when only flags the oracle ignores differ."""
    has_kernel(gpu)
    want = oracle_results(key, case, rounds)
    gc = gcase or case
    with Sim(gpu, gc["cfg"], shards=shards) as g:
        parity.setup(g, gc)
        for r in range(rounds):
            parity.apply_events((g,), gc, r)
            g.step(1)
            d = g.reciprocity().same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
    return want


def test_has_kernel(gpu):
    has_kernel(gpu)


@pytest.mark.parametrize("name", list(CASES))
def test_reciprocity_equals_oracle_every_round(gpu, name):
    case, rounds = CASES[name]
    want = run_against(gpu, "std:" + name, case, rounds)
    if name in ("churn_loss_512", "churn_2100", "stride_8300"):      # not vacuous: gaps of both kinds
        assert any(w.summary["mutual_pairs"] for w in want) and any(w.summary["oneway_pairs"] for w in want)


def test_reciprocity_exact_lru(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "lru:churn_loss_512", parity.with_cfg(case, variant=KB_VARIANT_EXACT_LRU), rounds)


def test_reciprocity_wide_row_flags(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "std:churn_loss_512", case, rounds, gcase=parity.with_cfg(case, debug_flags=KB_DBG_ALL))


def test_reciprocity_three_shards(gpu):
    case, rounds = STD["churn_loss_512"]                 # 640 rows in shards of 214: no boundary on a tile
    run_against(gpu, "std:churn_loss_512", case, rounds, shards=3)


def test_reciprocity_eight_shards_equal_the_unsharded_handle(gpu):
    """The row table at its last entry: 8 shards of 8 rows (fresh_ids, the smallest case here that 8 shards can split)
    against the unsharded handle, summary, arrays and pair list, every round."""
    has_kernel(gpu)
    case, rounds = CASES["fresh_ids"]
    assert min(c["cfg"].capacity for c, _ in CASES.values() if 7 * -(-c["cfg"].capacity // 8) < c["cfg"].capacity) == 64
    with Sim(gpu, case["cfg"]) as one, Sim(gpu, case["cfg"], shards=8) as grp:
        for g in (one, grp):
            parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((one, grp), case, r)
            one.step(1)
            grp.step(1)
            d = grp.reciprocity().same_as(one.reciprocity())
            assert not d, f"round {r}: " + "; ".join(d[:6])


def test_counts_past_32_bits_closed_form(gpu):
    """The one full-size case: after the first round of a join start nobody knows anybody, so every pair of the
    66,000 observers is a mutual gap; their number is above 2^31 and every row's count above 2^16."""
    has_kernel(gpu)
    n = 66000
    with Sim(gpu, SimConfig(capacity=69632, initial_nodes=n, init_mode=KB_INIT_JOIN, track_latency=0)) as g:
        g.step(1)
        r = g.reciprocity()
        assert (r.mutual[:n] == n - 1).all() and not r.mutual[n:].any()
        assert not r.lacks.any() and not r.lacked_by.any()
        s = r.summary
        assert s["observers"] == n and s["mutual_pairs"] == n * (n - 1) // 2 > 2**31
        assert s["oneway_pairs"] == 0 and s["rows_mutual"] == n and s["rows_oneway"] == 0
        assert (s["max_mutual_row"], s["max_mutual"]) == (0, n - 1)
        assert s["pairs_listed"] == 0 and len(r.pairs) == 0          # above the default max_pairs: nothing listed


def test_reciprocity_is_read_only(gpu):
    has_kernel(gpu)
    case, rounds = STD["churn_loss_512"]
    a, b = Sim(gpu, case["cfg"]), Sim(gpu, case["cfg"])
    for r in range(rounds):
        a.step(1)
        b.step(1)
        a.reciprocity()
        d = parity.diff_states(parity.state_of(a), parity.state_of(b))
        assert not d, f"round {r}: " + "; ".join(d[:6])
    a.close()
    b.close()


def test_reciprocity_arguments_and_refusals(gpu):
    has_kernel(gpu)
    case, rounds = STD["stop_start"]
    want = oracle_results("std:stop_start", case, rounds)
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
        out = KbReciprocity()
        buf = np.zeros(cap, dtype=np.uint32)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        g.lib.call("sim_reciprocity", g.h, C.byref(out), None, None, None, 0, None, 0)       # every array NULL
        got = out.as_dict()
        assert got == {**want[-1].summary, "pairs_listed": 0}
        assert g.reciprocity(arrays=False).summary == got
        assert 0.0 < g.reciprocity_device_ms() < 1000.0                 # the measurement hook reports the last call
        g.lib.call("sim_reciprocity", g.h, C.byref(out), None, None, ptr, cap, None, 0)      # lacked_by alone
        assert np.array_equal(buf, want[-1].lacked_by)
        for args in ((ptr, None, None), (None, ptr, None), (None, None, ptr)):               # a short cap_rows
            with pytest.raises(KbError) as e:
                g.lib.call("sim_reciprocity", g.h, C.byref(out), *args, cap - 1, None, 0)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:                                                    # out == NULL
            g.lib.call("sim_reciprocity", g.h, None, None, None, None, 0, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
        # the overflow rule on the device: one entry short lists nothing and still reports the total
        n = want[4].summary["mutual_pairs"]
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        for r in range(5):
            parity.apply_events((g,), case, r)
            g.step(1)
        assert n > 1
        short = g.reciprocity(max_pairs=n - 1)
        assert short.summary["mutual_pairs"] == n and short.summary["pairs_listed"] == 0 and len(short.pairs) == 0
        assert not g.reciprocity(max_pairs=n).same_as(want[4])
    # handles that cannot answer say so: sparse rows, and a rank handle (even of a one-rank world)
    with Sim(gpu, parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0)["cfg"]) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.reciprocity()
        assert e.value.code == KB_INVALID_OPERATION and "sparse" in str(e.value)
    with Sim(gpu, case["cfg"], rank=0, world=1, uid=rccl_unique_id(gpu)) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.reciprocity()
        assert e.value.code == KB_INVALID_OPERATION and "rank" in str(e.value)
