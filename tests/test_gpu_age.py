"""The contact-age census on the GPU (kb_sim_age_census, include/kaboodle_age.h; kernel in
kaboodle_amd/csrc/kb_agecensus.h): the pass over sparse rows against the sparse CPU oracle's reference census every
round, unsharded and as row shards, against the view census, read-only, and the handles that refuse."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_INVALID_ARGUMENT, KB_INVALID_OPERATION, KB_VARIANT_SPARSE_ROWS, KbAgeCensus, KbError,
                               Sim, rccl_unique_id)
from kaboodle_amd.age import SHARE_AGE

pytestmark = pytest.mark.gpu

STD = {n: (c, r) for n, c, r in parity.standard_cases()}
SPARSE = {n: (parity.with_cfg(STD[n][0], variant=KB_VARIANT_SPARSE_ROWS), STD[n][1])
          for n in ("partition_heal", "churn_loss_512")}
SPARSE["churn_loss_512"] = (SPARSE["churn_loss_512"][0], 72)   # past round 64: the window's epoch shifts
CLASSES = ("suspects", "ancient", "windowed", "dead_windowed")


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def has_kernel(lib) -> None:
    assert "sim_age_census" in lib.fn                    # the numpy fallback cannot stand in for the kernel


def test_library_exports_the_census(gpu):
    has_kernel(gpu)
    assert "sim_age_census_device_ms" in gpu.fn


_ORACLE: dict = {}
_SEEN: dict = {}                                     # per case: the classes' totals over its unsharded run


def oracle_censuses(key: str, case: dict, rounds: int):
    """The sparse oracle's reference census after every round of the case: computed once, shared, never changed."""
    if key not in _ORACLE or len(_ORACLE[key]) < rounds:
        out = []
        with Sim(parity.oracle_lib(), case["cfg"]) as o:
            assert "sim_age_census" not in o.lib.fn
            parity.setup(o, case)
            for r in range(rounds):
                parity.apply_events((o,), case, r)
                o.step(1)
                out.append(o.age_census())
        _ORACLE[key] = out
    return _ORACLE[key][:rounds]


def run_against(gpu, key: str, case: dict, rounds: int, shards: int = 0):
    """GPU age_census() == the oracle's (summary and the nine arrays) after every round."""
    has_kernel(gpu)
    want = oracle_censuses(key, case, rounds)
    got = []
    with Sim(gpu, case["cfg"], shards=shards) as g:
        parity.setup(g, case)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
            c = g.age_census()
            d = c.same_as(want[r])
            assert not d, f"{key} round {r}: " + "; ".join(d[:6])
            if r == rounds - 1:
                assert g.age_census(arrays=False).summary == c.summary
            got.append(c)
    assert sum(c.summary["cells"] for c in got) > 0, key
    return got


@pytest.mark.parametrize("name", list(SPARSE))
def test_age_census_sparse_rows_equal_oracle_every_round(gpu, name):
    case, rounds = SPARSE[name]
    got = run_against(gpu, "age-sparse:" + name, case, rounds)
    _SEEN[name] = {k: sum(c.summary[k] for c in got) for k in CLASSES}


@pytest.mark.parametrize("name", list(SPARSE))
def test_age_census_sparse_rows_three_shards(gpu, name):
    case, rounds = SPARSE[name]
    run_against(gpu, "age-sparse:" + name, case, rounds, shards=3)


def test_every_class_was_exercised(gpu):
    """Each class is nonzero in at least one of the cases, counted over those cases' own unsharded runs."""
    has_kernel(gpu)
    for n, (case, rounds) in SPARSE.items():
        if n not in _SEEN:                               # run alone or out of order: that case first
            got = run_against(gpu, "age-sparse:" + n, case, rounds)
            _SEEN[n] = {k: sum(c.summary[k] for c in got) for k in CLASSES}
    for k in CLASSES:
        assert any(_SEEN[n][k] > 0 for n in SPARSE), (k, _SEEN)


def test_identities_against_the_view_census(gpu):
    has_kernel(gpu)
    case, rounds = SPARSE["churn_loss_512"]
    with Sim(gpu, case["cfg"]) as g:
        g.step(30)
        c, v = g.age_census(), g.census()
        running = g.scalars()[:, 0] != 0
        holds_self = np.zeros(g.capacity, dtype=np.uint32)
        view = np.zeros(g.capacity, dtype=np.uint32)
        for i in np.flatnonzero(running).tolist():
            row = g.row(i)
            holds_self[i], view[i] = row[i] != 0, (row != 0).sum()
        assert np.array_equal(c.suspected_by + c.ancient_by + c.windowed_by, v.known_by - holds_self)
        assert np.array_equal(c.suspects + c.ancient + c.windowed, view - holds_self)
        assert int(view.sum()) == v.summary["pairs"] == c.summary["cells"] + int(holds_self.sum())
        s = c.summary
        assert sum(s["hist"]) == s["windowed"] > 0 and sum(s["hist"][:SHARE_AGE]) == s["fresh"]


def test_age_census_is_read_only(gpu):
    has_kernel(gpu)
    case, rounds = SPARSE["partition_heal"]
    a, b = Sim(gpu, case["cfg"]), Sim(gpu, case["cfg"])
    for r in range(rounds):
        parity.apply_events((a, b), case, r)
        a.step(1)
        b.step(1)
        a.age_census()
        assert a.census().same_as(b.census()) == []      # the view census's scratch is shared with the pass
        d = parity.diff_states(parity.state_of(a), parity.state_of(b))
        assert not d, f"round {r}: " + "; ".join(d[:6])
    a.close()
    b.close()


def test_refusals(gpu):
    has_kernel(gpu)
    dense = STD["stop_start"][0]["cfg"]
    sparse = parity.with_cfg(STD["stop_start"][0], variant=KB_VARIANT_SPARSE_ROWS)["cfg"]
    with Sim(gpu, sparse, rank=0, world=1, uid=rccl_unique_id(gpu)) as g:
        g.step(1)
        with pytest.raises(KbError) as e:
            g.age_census()
        assert e.value.code == KB_INVALID_OPERATION and "rank" in str(e.value)
    with Sim(gpu, dense) as g:                           # dense rows: not answered, and said so
        g.step(1)
        with pytest.raises(KbError) as e:
            g.age_census()
        assert e.value.code == KB_INVALID_OPERATION and "dense" in str(e.value)
    cap = sparse.capacity
    with Sim(gpu, sparse) as g:
        g.step(3)
        full = g.age_census()
        assert 0.0 < g.age_census_device_ms() < 1000.0
        out = KbAgeCensus()
        b32, i32 = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.int32)
        p32, pi = b32.ctypes.data_as(C.POINTER(C.c_uint32)), i32.ctypes.data_as(C.POINTER(C.c_int32))
        g.lib.call("sim_age_census", g.h, C.byref(out), None, None, None, None, pi, cap, None, None, None, None, 0)
        assert np.array_equal(i32, full.last_heard)      # last_heard alone
        g.lib.call("sim_age_census", g.h, C.byref(out), None, None, None, None, None, 0, None, None, p32, None, cap)
        assert np.array_equal(b32, full.windowed)        # one row array alone
        short = ((p32, None, None, None, None, cap - 1, None, None, None, None, 0),
                 (None, None, None, None, pi, cap - 1, None, None, None, None, 0),
                 (None, None, None, None, None, 0, None, None, None, p32, cap - 1))
        for args in short:
            with pytest.raises(KbError) as e:
                g.lib.call("sim_age_census", g.h, C.byref(out), *args)
            assert e.value.code == KB_INVALID_ARGUMENT
        with pytest.raises(KbError) as e:
            g.lib.call("sim_age_census", g.h, None, None, None, None, None, None, 0, None, None, None, None, 0)
        assert e.value.code == KB_INVALID_ARGUMENT
