"""The fingerprint-class census on the GPU (kb_sim_fp_classes and kb_fp_classes_of, include/kaboodle_classes.h;
kernels in kaboodle_amd/csrc/kb_classes.h): the hash-table grouping against the CPU oracle every round on dense and
sparse rows, unsharded and sharded, and against numpy on arrays crafted for each mechanism of the kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION, KB_VARIANT_EXACT_LRU,
                               KB_VARIANT_SPARSE_ROWS, KbError, KbFpClass, KbFpClasses, Sim, fp_classes_of,
                               rccl_unique_id)
from kaboodle_amd.classes import KB_CENSUS_NONE, fp_classes_of_arrays

pytestmark = pytest.mark.gpu

STD = {n: (c, r) for n, c, r in parity.standard_cases()}
CASES = {n: STD[n] for n in ("config1_2x2", "join_loss_300_ids", "churn_loss_512", "stop_start", "partition_heal",
                             "fresh_ids")}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def has_kernel(lib) -> None:
    assert "sim_fp_classes" in lib.fn                   # the numpy fallback cannot stand in for the kernel
    assert "fp_classes_of" in lib.fn


def sparse(case: dict, **kw) -> dict:
    return parity.with_cfg(case, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0, **kw)


_ORACLE: dict = {}


def oracle_results(key: str, case: dict, rounds: int):
    """The oracle's class census after every round of the case: computed once, shared, never changed."""
    if key not in _ORACLE:
        out = []
        with Sim(parity.oracle_lib(), case["cfg"]) as o:
            assert "sim_fp_classes" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.fp_classes(top=16))
        _ORACLE[key] = out
    return _ORACLE[key]


def run_against(gpu, key: str, case: dict, rounds: int, gcase: dict | None = None, shards: int = 0):
    """GPU fp_classes(top=16) == oracle fp_classes(top=16) (summary, list, both arrays) after every round; gcase =
    the case as the GPU runs it when only flags the oracle ignores differ."""
    has_kernel(gpu)
    want = oracle_results(key, case, rounds)
    gc = gcase or case
    with Sim(gpu, gc["cfg"], shards=shards) as g:
        parity.setup(g, gc)
        for r in range(rounds):
            parity.apply_events((g,), gc, r)
            g.step(1)
            d = g.fp_classes(top=16).same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
    return want


def test_has_kernel(gpu):
    has_kernel(gpu)


@pytest.mark.parametrize("name", list(CASES))
def test_classes_equal_oracle_every_round(gpu, name):
    case, rounds = CASES[name]
    want = run_against(gpu, "std:" + name, case, rounds)
    if name in ("churn_loss_512", "partition_heal", "join_loss_300_ids"):      # not vacuous: camps and stragglers
        assert any(w.summary["classes"] > 1 for w in want) and any(w.summary["largest"] > 1 for w in want)


def test_classes_exact_lru(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "lru:churn_loss_512", parity.with_cfg(case, variant=KB_VARIANT_EXACT_LRU), rounds)


def test_classes_wide_row_flags(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "std:churn_loss_512", case, rounds, gcase=parity.with_cfg(case, debug_flags=KB_DBG_ALL))


def test_classes_three_shards(gpu):
    case, rounds = STD["churn_loss_512"]
    run_against(gpu, "std:churn_loss_512", case, rounds, shards=3)


@pytest.mark.parametrize("shards", [0, 3], ids=["unsharded", "shards3"])
@pytest.mark.parametrize("name", list(CASES))
def test_sparse_classes_equal_oracle_every_round(gpu, name, shards):
    case, rounds = CASES[name]
    if shards and case["cfg"].capacity < shards * 2:
        shards = 2                                       # config1_2x2: 4 ids make 2 shards of 2 rows
    run_against(gpu, "sparse:" + name, sparse(case), rounds, shards=shards)


# ---- kb_fp_classes_of on crafted arrays, against numpy -----------------------------------------------------
def check_arrays(gpu, fps, run, true_fp, top=16):
    has_kernel(gpu)
    got = fp_classes_of(gpu, fps, run, true_fp, top=top)
    want = fp_classes_of_arrays(fps, run, true_fp, top=top)
    d = got.same_as(want)
    assert not d, "; ".join(d[:6])
    return got


def mixed(n: int, seed: int):
    """n rows: about a third in one class, the others in classes of every size down to 1, one row in eight not
    running with a running row's key in its slot."""
    rng = np.random.default_rng(seed)
    fps = rng.integers(0, max(2, n // 3), size=n, dtype=np.uint32) * np.uint32(0x9E3779B1)
    fps[rng.random(n) < 0.34] = 0xC0FFEE
    run = (rng.random(n) >= 0.125).astype(np.uint8)
    return fps, run


# 1 .. 65: inside and across one wave; 1025: past the LDS table's 1,024 slots; 2049: past one workgroup's 2,048 rows;
# 4097: past one sorted tile of 4,096 table slots
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 2049, 4097])
def test_arrays_sizes(gpu, n):
    fps, run = mixed(n, n)
    check_arrays(gpu, fps, run, int(fps[0]))
    run[:] = 1                                           # every row running and every key distinct: n classes
    check_arrays(gpu, np.arange(n, dtype=np.uint32) * np.uint32(2654435761), run, 0, top=1024)


def test_arrays_one_class_of_70000(gpu):
    """The contention path and a count past 16 bits: every add to one slot."""
    n = 70000
    r = check_arrays(gpu, np.full(n, 0xABCD1234, dtype=np.uint32), np.ones(n, dtype=np.uint8), 0xABCD1234)
    assert r.classes.tolist() == [[0xABCD1234, n, 0]] and r.summary["size_hist"][16] == 1
    assert (r.summary["true_size"], r.summary["true_rank"]) == (n, 0)


def test_arrays_5000_distinct(gpu):
    """More classes than the list holds and every size tied: the order is the fingerprints' alone, and a
    workgroup's 2,048 distinct keys overflow its 1,024-slot LDS table."""
    n = 5000
    fps = np.random.default_rng(5).permutation(n).astype(np.uint32) * np.uint32(7919) + np.uint32(11)
    r = check_arrays(gpu, fps, np.ones(n, dtype=np.uint8), int(fps.max()), top=16)
    assert r.summary["classes"] == r.summary["singletons"] == n and r.summary["listed"] == 16
    assert r.summary["true_rank"] == n - 1               # the last in the order
    assert r.classes[:, 0].tolist() == np.sort(fps)[:16].tolist()


def test_arrays_keys_0_and_all_ones(gpu):
    fps = np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 5, 0, 0], dtype=np.uint32)
    run = np.array([1, 1, 1, 1, 1, 1, 0, 0], dtype=np.uint8)   # the last two: stopped rows with fingerprint 0
    r = check_arrays(gpu, fps, run, 0)
    assert r.classes.tolist() == [[0xFFFFFFFF, 3, 1], [0, 2, 0], [5, 1, 5]]
    assert r.rep.tolist() == [0, 1, 0, 1, 1, 5, KB_CENSUS_NONE, KB_CENSUS_NONE]
    check_arrays(gpu, fps, run, 0xFFFFFFFF)


def test_arrays_stopped_rows_hold_running_keys(gpu):
    rng = np.random.default_rng(8)
    fps = rng.integers(0, 40, size=3000, dtype=np.uint32)
    run = (rng.random(3000) < 0.5).astype(np.uint8)      # half the rows of every key are not running
    r = check_arrays(gpu, fps, run, 7)
    assert r.summary["observers"] == int(run.sum()) < 3000


@pytest.mark.parametrize("shift", [16, 0], ids=["low16_equal", "high16_equal"])
def test_arrays_keys_that_agree_in_16_bits(gpu, shift):
    """3,000 keys that agree in their low (or high) 16 bits: collisions for any hash or digit split that looks at
    one half only; each key twice, so the classes have two rows."""
    k = (np.arange(3000, dtype=np.uint32) << np.uint32(shift)) | np.uint32(0xBEEF << (16 - shift))
    fps = np.concatenate([k, k[::-1]])
    r = check_arrays(gpu, fps, np.ones(6000, dtype=np.uint8), int(k[1234]), top=1024)
    assert r.summary["classes"] == 3000 and r.summary["size_hist"][1] == 3000


def test_arrays_true_class_absent_first_last(gpu):
    fps = np.array([9] * 5 + [4] * 3 + [6] * 3 + [2], dtype=np.uint32)
    run = np.ones(12, dtype=np.uint8)
    assert check_arrays(gpu, fps, run, 1).summary["true_rank"] == KB_CENSUS_NONE
    assert check_arrays(gpu, fps, run, 9).summary["true_rank"] == 0
    assert check_arrays(gpu, fps, run, 6).summary["true_rank"] == 2
    assert check_arrays(gpu, fps, run, 2).summary["true_rank"] == 3
    run[11] = 0                                          # the 2 is now a stopped row's: no such class
    assert check_arrays(gpu, fps, run, 2).summary["true_size"] == 0


def test_arrays_list_capacities(gpu):
    fps, run = mixed(3000, 77)
    none = check_arrays(gpu, fps, run, 0xC0FFEE, top=0)
    one = check_arrays(gpu, fps, run, 0xC0FFEE, top=1)
    full = check_arrays(gpu, fps, run, 0xC0FFEE, top=1024)
    assert len(none.classes) == 0 and none.summary["listed"] == 0
    assert one.classes.tolist() == full.classes[:1].tolist() and one.classes[0, 0] == 0xC0FFEE
    assert full.summary["listed"] == min(1024, full.summary["classes"]) > 16
    with pytest.raises(KbError) as e:                    # above KB_FPC_LIST_MAX
        fp_classes_of(gpu, fps, run, 0, top=1025)
    assert e.value.code == KB_INVALID_ARGUMENT


# ---- the handle's call ----------------------------------------------------------------------------------------
def test_classes_are_read_only(gpu):
    has_kernel(gpu)
    case, rounds = STD["churn_loss_512"]
    a, b = Sim(gpu, case["cfg"]), Sim(gpu, case["cfg"])
    for r in range(rounds):
        a.step(1)
        b.step(1)
        a.fp_classes()
    d = parity.diff_states(parity.state_of(a), parity.state_of(b))
    assert not d, "; ".join(d[:6])
    assert a.stats() == b.stats()
    a.close()
    b.close()


def test_two_calls_are_identical(gpu):
    has_kernel(gpu)
    case, rounds = STD["partition_heal"]
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        for r in range(min(rounds, 8)):
            parity.apply_events((g,), case, r)
            g.step(1)
        first, second = g.fp_classes(top=1024), g.fp_classes(top=1024)
        assert not first.same_as(second)
        assert 0.0 < g.fp_classes_device_ms() < 1000.0    # the measurement hook reports the last call
    fps, run = mixed(20000, 3)
    assert not fp_classes_of(gpu, fps, run, 1, top=1024).same_as(fp_classes_of(gpu, fps, run, 1, top=1024))


def test_arguments_and_refusals(gpu):
    has_kernel(gpu)
    case, rounds = STD["stop_start"]
    want = oracle_results("std:stop_start", case, rounds)[-1]
    cap = case["cfg"].capacity
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
        out, n = KbFpClasses(), C.c_size_t(99)
        buf = np.zeros(cap, dtype=np.uint32)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        lst = (KbFpClass * 4)()
        g.lib.call("sim_fp_classes", g.h, C.byref(out), None, 0, C.byref(n), None, None, 0)   # the summary alone
        assert out.as_dict() == {**want.summary, "listed": 0, "listed_observers": 0} and n.value == 0
        assert g.fp_classes(top=0, arrays=False).summary == out.as_dict()
        g.lib.call("sim_fp_classes", g.h, C.byref(out), None, 0, None, None, ptr, cap)        # size alone
        assert np.array_equal(buf, want.size)
        g.lib.call("sim_fp_classes", g.h, C.byref(out), None, 0, None, ptr, None, cap)        # rep alone
        assert np.array_equal(buf, want.rep)
        for args in ((ptr, None), (None, ptr)):                                              # a short array
            with pytest.raises(KbError) as e:
                g.lib.call("sim_fp_classes", g.h, C.byref(out), None, 0, None, *args, cap - 1)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:                                                    # list NULL, cap_list > 0
            g.lib.call("sim_fp_classes", g.h, C.byref(out), None, 4, None, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:                                                    # above KB_FPC_LIST_MAX
            g.lib.call("sim_fp_classes", g.h, C.byref(out), lst, 1025, None, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:                                                    # out == NULL
            g.lib.call("sim_fp_classes", g.h, None, None, 0, None, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
    # a rank handle, even of a one-rank world, says that it cannot answer
    with Sim(gpu, case["cfg"], rank=0, world=1, uid=rccl_unique_id(gpu)) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.fp_classes()
        assert e.value.code == KB_INVALID_OPERATION and "rank" in str(e.value)
