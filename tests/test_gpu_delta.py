"""The view-delta census on the GPU (kb_sim_delta_mark / _census / _release, include/kaboodle_delta.h; kernel in
kaboodle_amd/csrc/kb_delta.h): against the CPU oracle through the same calls every round, over a multi-round
interval, on crafted matrices through kb_delta_of against delta_ref, read-only, and the refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_DELTA_ADVANCE, KB_INVALID_ARGUMENT, KB_INVALID_OPERATION,
                               KB_VARIANT_EXACT_LRU, KB_VARIANT_SPARSE_ROWS, KbDelta, KbError, Sim, delta_of,
                               rccl_unique_id)
from kaboodle_amd.delta import ARRAYS, delta_ref, sum_parts

pytestmark = pytest.mark.gpu

NAMES = ("churn40", "stop_start", "identity_change", "partition", "socket_faithful", "trunc_odd")
# how the GPU runs a scenario -> the config fields replaced; the oracle ignores debug_flags, not the variant
MODES = {"plain": {}, "dbg_all": {"debug_flags": KB_DBG_ALL}, "exact_lru": {"variant": KB_VARIANT_EXACT_LRU}}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    lib = parity.gpu_lib()
    assert "sim_delta_census" in lib.fn and "delta_of" in lib.fn   # the numpy fallback cannot stand in for the kernel
    return lib


def scenario(name: str, **kw) -> dict:
    return parity.with_cfg(scenarios.BY_NAME[name], **kw)


def drive(sim: Sim, sc: dict, mark_after: int = -1, until: int | None = None):
    """The scenario on `sim` with a mark after round `mark_after` (-1: before the first): yields the round index after
    every later step."""
    scenarios.setup(sim, sc)
    if mark_after < 0:
        sim.delta_mark()
    for r in range(sc["rounds"] if until is None else until + 1):
        scenarios.apply_events(sim, sc, r)
        sim.step(1)
        if r == mark_after:
            sim.delta_mark()
        elif r > mark_after:
            yield r


_ORACLE: dict = {}


def oracle_deltas(name: str, variant: int):
    """The oracle's advancing delta census after every round of the scenario: computed once, shared, never changed."""
    key = (name, variant)
    if key not in _ORACLE:
        sc = scenario(name, variant=variant)
        with Sim(parity.oracle_lib(), sc["cfg"]) as o:
            assert "sim_delta_census" not in o.lib.fn
            _ORACLE[key] = [o.delta_census(advance=True) for _ in drive(o, sc)]
    return _ORACLE[key]


@pytest.mark.parametrize("shards", [0, 3], ids=["unsharded", "shards3"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_delta_equals_oracle_every_round(gpu, name, mode, shards):
    want = oracle_deltas(name, MODES[mode].get("variant", 0))
    sc = scenario(name, **MODES[mode])
    changed = 0
    with Sim(gpu, sc["cfg"], shards=shards) as g:
        for r in drive(g, sc):
            got = g.delta_census(advance=True)
            d = got.same_as(want[r])
            assert not d, f"{name} round {r}: " + "; ".join(d[:6])
            changed += got.summary["changed_ids"]
    assert changed > 0


def test_delta_over_a_multi_round_interval(gpu):
    """Mark after round 2, census after round 12 without ADVANCE: what was gained and lost again in between cancels."""
    sc = scenario("churn40")
    with Sim(parity.oracle_lib(), sc["cfg"]) as o:
        for _ in drive(o, sc, mark_after=2, until=12):
            pass
        want = o.delta_census(advance=False)
    per_round = oracle_deltas("churn40", 0)
    assert sum(int(d.gained.sum()) for d in per_round[3:13]) > int(want.gained.sum()) > 0     # something did cancel
    with Sim(gpu, sc["cfg"]) as g:
        for _ in drive(g, sc, mark_after=2, until=12):
            pass
        got = g.delta_census(advance=False)
        assert not got.same_as(want), "; ".join(got.same_as(want)[:6])
        assert (got.summary["round_base"], got.summary["round"]) == (3, 13)
        assert not g.delta_census(advance=False).same_as(got)                                # read-only: the same again
        assert g.delta_census(advance=False, arrays=False).summary == got.summary


# ---- crafted matrices through kb_delta_of ------------------------------------------------------------------------
def pack(m: np.ndarray, cap: int) -> np.ndarray:
    """bool [rows][cols <= W] -> uint32 [rows][W/32], bit j & 31 of word j >> 5 is id j."""
    W = (cap + 8191) // 8192 * 8192
    full = np.zeros((m.shape[0], W), dtype=np.uint8)
    full[:, : m.shape[1]] = m
    return np.packbits(full, axis=1, bitorder="little").view("<u4")


def crafted(cap: int, rows: int, row_lo: int, pattern: str, seed: int):
    """(base, now, run0, run1, ext): member matrices [rows][W] (bits past the capacity set at random: ignored) of
    the ids row_lo onwards, with rows of all four kinds and a few external ids."""
    rng = np.random.default_rng(seed)
    W = (cap + 8191) // 8192 * 8192
    kind = rng.choice(4, size=cap, p=[0.7, 0.1, 0.1, 0.1])           # continuing, new, ended, never
    ext = (kind == 3) & (rng.random(cap) < 0.5)
    run0, run1 = (kind == 0) | (kind == 2), (kind == 0) | (kind == 1)
    base = rng.random((rows, W)) < 0.5
    lose, gain = cap - 1, 33 if cap < 4200 else 4097                  # the last valid id; one of another column block
    run1[lose], run1[gain], ext[lose], ext[gain] = True, False, False, False   # a live id lost, a dead id gained
    cont = (run0 & run1)[row_lo:row_lo + rows]
    now = base.copy()
    if pattern == "same_id":
        base[:, lose], now[:, lose] = True, False
        base[:, gain], now[:, gain] = False, True
    elif pattern == "flipped":
        now = ~base
    elif pattern == "others_only":
        now[~cont] = ~base[~cont]
    else:
        assert pattern == "unchanged"
    return base, now, run0, run1, ext


_CRAFTED = [(300, 300, 0), (8200, 300, 4000)]                        # capacity, rows, the first row's id


@pytest.mark.parametrize("rpw", [24, 48])
@pytest.mark.parametrize("pattern", ["same_id", "flipped", "unchanged", "others_only"])
@pytest.mark.parametrize("cap,rows,row_lo", _CRAFTED, ids=["cap300", "cap8200"])
def test_crafted_matrices_against_delta_ref(gpu, cap, rows, row_lo, pattern, rpw):
    base, now, run0, run1, ext = crafted(cap, rows, row_lo, pattern, seed=cap + rpw)
    want = delta_ref(base, run0, now, run1, ext, row_lo)
    pb, pn = pack(base, cap), pack(now, cap)
    got = delta_of(gpu, pb, run0, pn, run1, ext, row_lo=row_lo, rpw=rpw)
    assert not got.same_as(want), "; ".join(got.same_as(want)[:6])
    cut = 137                                                         # two row ranges: their parts add up
    parts = [delta_of(gpu, pb[:cut], run0, pn[:cut], run1, ext, row_lo=row_lo, rpw=rpw),
             delta_of(gpu, pb[cut:], run0, pn[cut:], run1, ext, row_lo=row_lo + cut, rpw=rpw)]
    whole = sum_parts(parts, run0, run1, ext)
    assert not whole.same_as(want), "; ".join(whole.same_as(want)[:6])
    n_cont = int((run0 & run1)[row_lo:row_lo + rows].sum())
    if pattern == "same_id":
        assert got.lost_by[cap - 1] == got.gained_by[33 if cap < 4200 else 4097] == n_cont > 100
        assert got.summary["false_drops"] == got.summary["ghost_adds"] == n_cont
    elif pattern == "flipped":
        assert got.summary["changed_rows"] == n_cont and int(got.gained.sum() + got.lost.sum()) == n_cont * cap
    else:
        assert not any(getattr(got, n).any() for n in ARRAYS) and got.summary["changed_ids"] == 0


@pytest.mark.parametrize("rpw", [0, 4080], ids=["default_rpw", "rpw4080"])
def test_counts_past_the_high_planes(gpu, rpw):
    """4,160 continuing rows all lose id 0: more than the 2^12 - 1 one wave's planes can hold, so the count is the
    sum of several waves' tiles; at 4,080 rows per wave one wave's planes come as close to full as they can."""
    cap = 4160
    rng = np.random.default_rng(5)
    base = np.zeros((cap, cap), dtype=bool)
    base[:, :64] = rng.random((cap, 64)) < 0.5
    base[:, 0] = True
    now = base.copy()
    now[:, 0] = False
    run = np.ones(cap, dtype=bool)
    ext = np.zeros(cap, dtype=bool)
    got = delta_of(gpu, pack(base, cap), run, pack(now, cap), run, ext, rpw=rpw)
    want = delta_ref(base, run, now, run, ext)
    assert not got.same_as(want), "; ".join(got.same_as(want)[:6])
    assert got.lost_by[0] == cap and got.summary["false_drops"] == cap and (got.lost_live == 1).all()
    half = [delta_of(gpu, pack(base[:4090], cap), run, pack(now[:4090], cap), run, ext, row_lo=0, rpw=rpw),
            delta_of(gpu, pack(base[4090:], cap), run, pack(now[4090:], cap), run, ext, row_lo=4090, rpw=rpw)]
    assert not sum_parts(half, run, run, ext).same_as(want)


# ---- the handle's contract -----------------------------------------------------------------------------------------
def test_delta_census_is_read_only(gpu):
    """Two meshes side by side, one with an advancing delta census every round: the complete state stays identical."""
    sc = scenario("churn40")
    with Sim(gpu, sc["cfg"]) as a, Sim(gpu, sc["cfg"]) as b:
        scenarios.setup(b, sc)
        for r in drive(a, sc):
            scenarios.apply_events(b, sc, r)
            b.step(1)
            a.delta_census(advance=True)
            d = parity.diff_states(parity.state_of(a), parity.state_of(b))
            assert not d, f"round {r}: " + "; ".join(d[:6])


@pytest.mark.parametrize("shards", [0, 2], ids=["unsharded", "shards2"])
def test_advance_is_a_mark_and_release_forgets(gpu, shards):
    sc = scenario("churn40")
    with Sim(gpu, sc["cfg"], shards=shards) as g, Sim(gpu, sc["cfg"], shards=shards) as m:
        assert g.delta_census_device_ms() == 0.0
        with pytest.raises(KbError) as e:
            g.delta_census()
        assert e.value.code == KB_INVALID_OPERATION and "no baseline" in str(e.value)
        assert g.delta_census_device_ms() == 0.0
        g.delta_release()                                             # nothing to free: KB_OK
        for (r, _) in zip(drive(g, sc, until=8), drive(m, sc, until=8)):
            first = g.delta_census(advance=True)
            assert g.delta_census_device_ms() > 0.0
            zero = g.delta_census(advance=False)
            assert zero.summary["round_base"] == zero.summary["round"] == r + 1
            assert not any(getattr(zero, n).any() for n in ARRAYS)
            assert all(zero.summary[k] == 0 for k in ("new_rows", "ended_rows", "changed_rows", "changed_ids"))
            other = m.delta_census(advance=False)                     # the same interval by an explicit mark
            m.delta_mark()
            assert not other.same_as(first), "; ".join(other.same_as(first)[:6])
        g.delta_release()
        with pytest.raises(KbError) as e:
            g.delta_census(advance=False)
        assert e.value.code == KB_INVALID_OPERATION and "no baseline" in str(e.value)
        g.delta_mark()                                                # and a new mark answers again
        assert g.delta_census(advance=False).summary["changed_ids"] == 0


OWN_ROWS = " (use kb_sim_create or kb_sim_create_local)"
SPARSE_TEXT = ": sparse rows keep no member bits to take a baseline of"
RANK_TEXT = ": a rank handle holds its own rows only and a baseline of the whole mesh spans ranks" + OWN_ROWS


@pytest.mark.parametrize("kind", ["sparse", "sparse_x2", "rank", "sparse_rank"])
def test_refusals(gpu, kind):
    sc = scenario("stop_start", variant=KB_VARIANT_SPARSE_ROWS if kind.startswith("sparse") else 0)
    kw = dict(rank=0, world=1, uid=rccl_unique_id(gpu)) if kind.endswith("rank") else dict(shards=2 if kind == "sparse_x2" else 0)
    text = SPARSE_TEXT if kind.startswith("sparse") else RANK_TEXT   # sparse rows are refused before a rank handle
    with Sim(gpu, sc["cfg"], **kw) as g:
        g.step(2)
        for call, fn in (("kb_sim_delta_mark", g.delta_mark), ("kb_sim_delta_census", g.delta_census),
                         ("kb_sim_delta_release", g.delta_release)):
            with pytest.raises(KbError) as e:
                fn()
            assert e.value.code == KB_INVALID_OPERATION
            assert gpu.fn["last_error"]().decode() == call + text
        assert g.delta_census_device_ms() == 0.0


def test_arguments(gpu):
    sc = scenario("stop_start")
    cap = sc["cfg"].capacity
    with Sim(gpu, sc["cfg"]) as g:
        g.step(1)
        g.delta_mark()
        g.step(2)
        out = KbDelta()
        buf = np.zeros(cap, dtype=np.uint32)
        ptr = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        call = lambda *a: g.lib.call("sim_delta_census", g.h, *a)
        call(C.byref(out), None, None, 0, None, None, None, 0, 0)                     # every array NULL
        assert out.round_base == 1 and out.round == 3
        call(C.byref(out), None, None, 0, None, None, ptr, cap, 0)                    # lost_live alone
        short = [(ptr, None, cap - 1, None, None, None, 0), (None, ptr, cap - 1, None, None, None, 0),
                 (None, None, 0, ptr, None, None, cap - 1), (None, None, 0, None, ptr, None, cap - 1),
                 (None, None, 0, None, None, ptr, cap - 1)]
        for args in short:
            with pytest.raises(KbError) as e:
                call(C.byref(out), *args, 0)
            assert e.value.code == KB_INVALID_ARGUMENT
        for args in ((None, None, None, 0, None, None, None, 0, 0),                    # no summary
                     (C.byref(out), None, None, 0, None, None, None, 0, KB_DELTA_ADVANCE | 2)):   # an unknown flag
            with pytest.raises(KbError) as e:
                call(*args)
            assert e.value.code == KB_INVALID_ARGUMENT
        assert g.delta_census(advance=False).summary["round_base"] == 1                # nothing above advanced
