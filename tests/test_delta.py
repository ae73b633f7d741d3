"""The view-delta census on the CPU (kaboodle_amd/delta.py): delta_ref against hand-counted matrices, the oracle's
path through Sim.delta_mark / delta_census against delta_ref of the dumped rows, the sum invariants, the link to the
view census, and the PairTracker on a crafted sequence."""
from __future__ import annotations

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd._ffi import KB_INVALID_OPERATION, KbError, Sim
from kaboodle_amd.census import census_ref
from kaboodle_amd.delta import ARRAYS, KB_CENSUS_NONE, SUMMARY_FIELDS, DeltaCensus, PairTracker, delta_ref


def mat(rows):
    """Member matrix from one set of ids per row, 7 columns: ids 0..5 and one column past the capacity of 6."""
    m = np.zeros((len(rows), 7), dtype=np.uint8)
    for i, ids in enumerate(rows):
        m[i, list(ids)] = 1
    return m


# ids 0-2 run throughout, 3 begins to run, 4 ends, 5 is external (never a row); column 6 is past the capacity
RUN0 = [1, 1, 1, 0, 1, 0]
RUN1 = [1, 1, 1, 1, 0, 0]
EXT = [0, 0, 0, 0, 0, 1]
BASE = mat([{0, 1, 2, 4}, {0, 1, 2, 4, 5, 6}, {0, 1, 2}, set(), {0, 1, 2, 4}, set()])
NOW = mat([{0, 2, 3, 5},          # gains the new id and the external one; loses live 1 and dead 4
           {0, 1, 2, 3},          # gains 3; loses dead 4 and external 5 (and column 6, ignored)
           {0, 1, 2, 3, 4, 6},    # gains 3 and dead 4 (a ghost add; and column 6, ignored)
           {0, 1, 2, 3},          # a new row: not counted
           set(),                 # an ended row: not counted
           set()])


def test_delta_ref_by_hand():
    d = delta_ref(BASE, RUN0, NOW, RUN1, EXT, round_base=3, round_=9)
    assert d.gained_by.tolist() == [0, 0, 0, 3, 1, 1]
    assert d.lost_by.tolist() == [0, 1, 0, 0, 2, 1]
    assert d.gained.tolist() == [2, 1, 2, 0, 0, 0]
    assert d.lost.tolist() == [2, 2, 0, 0, 0, 0]
    assert d.lost_live.tolist() == [1, 0, 0, 0, 0, 0]
    assert all(a.dtype == np.uint32 for a in (d.gained_by, d.lost_by, d.gained, d.lost, d.lost_live))
    assert tuple(d.summary) == SUMMARY_FIELDS
    assert d.summary == {"round_base": 3, "round": 9, "continuing": 3, "new_rows": 1, "ended_rows": 1,
                         "changed_rows": 3, "changed_ids": 4, "top_false_drop": 1, "top_false_drop_by": 1,
                         "learned": 3, "ghost_adds": 1, "detections": 2, "false_drops": 1, "ext_gained": 1,
                         "ext_lost": 1}


def test_delta_ref_nothing_lost_and_row_range():
    d = delta_ref(BASE, RUN0, BASE, RUN0, EXT)
    assert not any(getattr(d, n).any() for n in ARRAYS)
    assert (d.summary["top_false_drop"], d.summary["top_false_drop_by"]) == (KB_CENSUS_NONE, 0)
    assert d.summary["continuing"] == 4 and d.summary["changed_rows"] == d.summary["changed_ids"] == 0
    # rows 1..2 alone: the parts of two row ranges add up to the whole
    whole = delta_ref(BASE, RUN0, NOW, RUN1, EXT)
    a = delta_ref(BASE[:1], RUN0, NOW[:1], RUN1, EXT, row_lo=0)
    b = delta_ref(BASE[1:], RUN0, NOW[1:], RUN1, EXT, row_lo=1)
    for n in ARRAYS:
        assert np.array_equal(getattr(a, n) + getattr(b, n), getattr(whole, n)), n
    assert a.summary["continuing"] + b.summary["continuing"] == 3
    # the tie goes to the lowest id: rows 0 and 1 both lose live ids 1 and 2
    now = BASE.copy()
    now[0, [1, 2]] = 0
    now[1, [1, 2]] = 0
    s = delta_ref(BASE, RUN0, now, RUN0, EXT).summary
    assert (s["top_false_drop"], s["top_false_drop_by"], s["false_drops"]) == (1, 2, 4)


def check_sums(d: DeltaCensus) -> None:
    s = d.summary
    assert int(d.gained_by.sum()) == int(d.gained.sum()) == s["learned"] + s["ghost_adds"] + s["ext_gained"]
    assert int(d.lost_by.sum()) == int(d.lost.sum()) == s["detections"] + s["false_drops"] + s["ext_lost"]
    assert int(d.lost_live.sum()) == s["false_drops"]


def run_oracle(name: str):
    """The scenario on the oracle: yields (round index, sim) after every step."""
    sc = scenarios.BY_NAME[name]
    with Sim(parity.oracle_lib(), sc["cfg"]) as o:
        assert "sim_delta_census" not in o.lib.fn           # delta_ref answers through the same calls
        scenarios.setup(o, sc)
        yield -1, o
        for r in range(sc["rounds"]):
            scenarios.apply_events(o, sc, r)
            o.step(1)
            yield r, o


@pytest.mark.parametrize("name,a,b", [("churn40", 2, 12), ("stop_start", 1, 9)])
def test_oracle_delta_over_an_interval(name, a, b):
    """Mark after round a, census after round b: delta_ref of the rows dumped at the two instants; a non-advancing
    call repeated is identical; every round in between an advancing census on a second handle obeys the sums."""
    gen2 = run_oracle(name)
    base = None
    for (r, o), (_, p) in zip(run_oracle(name), gen2):
        if r == -1:
            with pytest.raises(KbError) as e:
                o.delta_census()
            assert e.value.code == KB_INVALID_OPERATION and "no baseline" in str(e.value)
            p.delta_mark()
            continue
        d = p.delta_census(advance=True)                    # per-round deltas on the second handle
        check_sums(d)
        assert (d.summary["round_base"], d.summary["round"]) == (r, r + 1)
        if r == a:
            o.delta_mark()
            base = (o.rows(), o.scalars()[:, 0] != 0, o.stats()["round"])
        if r == b:
            ext = np.zeros(o.capacity, dtype=bool)
            want = delta_ref(base[0], base[1], o.rows(), o.scalars()[:, 0] != 0, ext, 0, base[2], o.stats()["round"])
            got = o.delta_census(advance=False)
            assert not got.same_as(want), got.same_as(want)
            assert not o.delta_census(advance=False).same_as(got)
            assert o.delta_census(advance=False, arrays=False).summary == got.summary
            check_sums(got)
            assert got.summary["changed_ids"] > 0 and got.summary["new_rows"] + got.summary["ended_rows"] > 0
            z = o.delta_census(advance=True)
            assert not z.same_as(got)
            z = o.delta_census(advance=False)               # the advance made now the baseline
            assert z.summary["round_base"] == z.summary["round"] and not any(getattr(z, n).any() for n in ARRAYS)
            o.delta_release()
            with pytest.raises(KbError):
                o.delta_census()
            break
    gen2.close()


def test_delta_explains_the_change_of_known_by():
    """No row begins or ends in conv_loss48, so every change of known_by is a gain or a loss of a continuing row."""
    prev = None
    seen = 0
    for r, o in run_oracle("conv_loss48"):
        if r == -1:
            o.delta_mark()
            prev = census_ref(o).known_by.astype(np.int64)
            continue
        d = o.delta_census(advance=True)
        kb = census_ref(o).known_by.astype(np.int64)
        assert d.summary["new_rows"] == d.summary["ended_rows"] == 0 and d.summary["continuing"] == 48
        assert np.array_equal(kb - prev, d.gained_by.astype(np.int64) - d.lost_by.astype(np.int64)), f"round {r}"
        check_sums(d)
        seen += d.summary["changed_ids"]
        prev = kb
    assert seen > 0


def test_pair_tracker_on_a_crafted_sequence():
    def dc(round_, gby, lby, **s):
        z = np.zeros(4, dtype=np.uint32)
        summary = {**{k: 0 for k in SUMMARY_FIELDS}, "round": round_, "round_base": round_ - 1, **s}
        return DeltaCensus(summary, np.array(gby, np.uint32), np.array(lby, np.uint32), z, z, z)

    t = PairTracker()
    t.update(dc(5, [0, 0, 0, 0], [0, 0, 0, 1], continuing=4, false_drops=1), [1, 1, 1, 1])   # 3 still runs: no pair
    assert t.latencies()["removals"] == 0 and t.latencies()["quantiles"]["p50"] is None
    t.update(dc(6, [0, 0, 0, 0], [0, 0, 0, 2], continuing=3, ghost_adds=0), [1, 1, 1, 0])    # 3 stopped: at = 6
    t.update(dc(7, [0, 0, 0, 1], [1, 0, 0, 1], continuing=3, false_drops=1, ghost_adds=1), [1, 1, 1, 0])
    t.update(dc(9, [0, 0, 0, 0], [0, 0, 0, 1], continuing=3), [1, 1, 1, 0])                  # dropped again, 3 later
    lat = t.latencies()
    assert t.at == {3: 6}
    assert lat["detect_hist"] == [2, 1, 0, 1] and lat["relearn_hist"] == [0, 1]
    assert (lat["removals"], lat["relearned"], lat["stopped_ids"]) == (4, 1, 1)
    assert lat["quantiles"] == {"p50": 0, "p90": 3, "p99": 3, "max": 3}
    assert (t.rounds, t.false_drops, t.ghost_adds, t.continuing) == ([5, 6, 7, 9], [1, 0, 1, 0], [0, 0, 1, 0], [4, 3, 3, 3])
    assert "counted twice" in PairTracker.__doc__ and "relearn_hist" in PairTracker.__doc__
