"""The view census on the CPU oracle (kaboodle_amd/census.py): census_ref against a direct count from peers() of
every node, the external-peer convention, and the Tracker on hand-written sequences and on the oracle."""
from __future__ import annotations

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import KB_INIT_CONVERGED, Sim, SimConfig
from kaboodle_amd.census import KB_CENSUS_NONE, Census, Tracker, census_ref
from parity import K_JOIN

CASES = {n: (c, r) for n, c, r in parity.standard_cases()}


def direct_count(sim: Sim, external=()):
    """known_by / missing / stale / |view| straight from the definitions, through peers() and is-running scalars."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    ext = set(external)
    kb, mi, st, view = (np.zeros(C, dtype=np.uint32) for _ in range(4))
    run_set = set(np.flatnonzero(running).tolist())
    for i in sorted(run_set):
        p = set(sim.peers(i))
        assert i in p                                   # a view holds its own address
        for j in p:
            kb[j] += 1
        view[i] = len(p)
        mi[i] = len(run_set - p)
        st[i] = len([j for j in p if j not in run_set and j not in ext])
    return running, kb, mi, st, view


def check_against_direct(sim: Sim, external=()):
    c = sim.census()                                    # the oracle has no kb_sim_census: census_ref answers
    running, kb, mi, st, view = direct_count(sim, external)
    assert np.array_equal(c.known_by, kb) and np.array_equal(c.missing, mi) and np.array_equal(c.stale, st)
    assert np.array_equal(c.running, running)
    s, n_obs = c.summary, int(running.sum())
    assert s["round"] == sim.stats()["round"]
    assert s["observers"] == s["running"] == n_obs
    assert s["pairs"] == int(view.sum()) == int(kb.sum())
    assert s["missing"] == int(mi.sum()) and s["stale"] == int(st.sum())
    assert s["exact_views"] == int((running & (mi == 0) & (st == 0)).sum())
    assert s["full_ids"] == int((running & (kb == n_obs)).sum())
    ghosts = [j for j in range(sim.capacity) if not running[j] and j not in set(external) and kb[j] > 0]
    assert s["ghost_ids"] == len(ghosts)
    if ghosts:
        top = max(kb[j] for j in ghosts)
        assert (s["top_ghost"], s["top_ghost_by"]) == (min(j for j in ghosts if kb[j] == top), top)
    else:
        assert (s["top_ghost"], s["top_ghost_by"]) == (KB_CENSUS_NONE, 0)
    ids = np.flatnonzero(running)
    low = kb[ids].min()
    assert (s["least_known"], s["least_known_by"]) == (int(ids[kb[ids] == low][0]), int(low))
    return c


@pytest.mark.parametrize("name,every", [("stop_start", 1), ("churn_loss_512", 8), ("fresh_ids", 1)])
def test_census_ref_equals_direct_count(name, every):
    case, rounds = CASES[name]
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        assert "sim_census" not in o.lib.fn
        parity.setup(o, case)
        seen_ghost = seen_missing = False
        for r in range(rounds):
            parity.apply_events((o,), case, r)
            o.step(1)
            if (r + 1) % every == 0 or r == rounds - 1:
                c = check_against_direct(o)
                seen_ghost |= c.summary["ghost_ids"] > 0
                seen_missing |= c.summary["missing"] > 0
        assert seen_ghost and seen_missing              # the cases do exercise stale and missing entries


def test_external_peers_count_in_known_by_never_in_missing_or_stale():
    cfg = SimConfig(capacity=48, initial_nodes=40, init_mode=KB_INIT_CONVERGED, seed=5)
    with Sim(parity.oracle_lib(), cfg) as s:
        s.set_external(46)
        s.step(1)
        s.inject(46, 0, K_JOIN)
        s.step(1)
        c = check_against_direct(s, external=[46])
        assert c.known_by[46] == 40                     # every running peer inserted the external Join
        assert c.summary["pairs"] == 40 * 41            # ... and it counts in pairs
        assert c.summary["stale"] == 0 and c.summary["missing"] == 0 and c.summary["ghost_ids"] == 0
        assert c.summary["exact_views"] == 40 and c.summary["full_ids"] == 40
        # the same views with the id NOT declared external: a non-running id in 40 views is a ghost
        d = census_ref(s, external=[])
        assert d.summary["stale"] == 40 and d.summary["ghost_ids"] == 1 and d.summary["top_ghost"] == 46
        assert d.summary["top_ghost_by"] == 40 and d.summary["exact_views"] == 0
        assert np.array_equal(d.known_by, c.known_by) and np.array_equal(d.missing, c.missing)


def _census(r, running, known_by):
    running = np.asarray(running, dtype=bool)
    kb = np.asarray(known_by, dtype=np.uint32)
    z = np.zeros(len(kb), dtype=np.uint32)
    return Census({"round": r, "observers": int(running.sum())}, kb, z, z, running)


def test_tracker_hand_written_sequences():
    t = Tracker()
    #            round  running            known_by
    t.update(_census(1, [1, 1, 1, 1, 0], [4, 4, 4, 4, 0]))
    t.update(_census(2, [1, 1, 1, 0, 0], [3, 3, 3, 3, 0]))     # 3 stopped; still in all 3 views
    assert t.stopped == {3: {"at": 2, "first_dropped": -1, "gone": -1}}
    t.update(_census(3, [1, 1, 1, 0, 1], [4, 4, 4, 2, 1]))     # 4 started (knows itself); 3 dropped by one view
    assert t.stopped[3] == {"at": 2, "first_dropped": 3, "gone": -1}
    assert t.started == {4: {"at": 3, "everywhere": -1}}
    t.update(_census(4, [1, 1, 1, 0, 1], [4, 4, 4, 1, 3]))
    t.update(_census(5, [1, 1, 1, 0, 1], [4, 4, 4, 0, 4]))     # 3 gone, 4 everywhere
    assert t.stopped[3] == {"at": 2, "first_dropped": 3, "gone": 5}
    assert t.started[4] == {"at": 3, "everywhere": 5}
    t.update(_census(6, [1, 1, 1, 0, 1], [4, 4, 4, 2, 4]))     # a stale KnownPeers list re-inserts 3: the record stands
    assert t.stopped[3]["gone"] == 5
    lat = t.latencies()
    assert lat["first_dropped"].tolist() == [1] and lat["gone"].tolist() == [3] and lat["everywhere"].tolist() == [2]
    assert lat["open_gone"] == 0 and lat["open_everywhere"] == 0
    assert t.histogram() == {"first_dropped": [0, 1], "gone": [0, 0, 0, 1], "everywhere": [0, 0, 1]}


def test_tracker_same_census_marks_and_open_records():
    t = Tracker()
    t.update(_census(7, [1, 1, 1], [3, 3, 3]))
    t.update(_census(8, [1, 1, 0], [2, 2, 0]))                 # stopped and unknown to everyone in the same census
    assert t.stopped[2] == {"at": 8, "first_dropped": 8, "gone": 8}
    t.update(_census(9, [1, 0, 0], [1, 1, 0]))                 # 1 stopped, never forgotten while we watch
    t.update(_census(10, [1, 0, 0], [1, 1, 0]))
    assert t.stopped[1] == {"at": 9, "first_dropped": -1, "gone": -1}
    lat = t.latencies()
    assert lat["gone"].tolist() == [0] and lat["open_gone"] == 1
    assert t.histogram()["gone"] == [1] and t.histogram()["everywhere"] == []


def test_tracker_keeps_the_record_of_an_id_that_stops_twice():
    t = Tracker()
    t.update(_census(1, [1, 1, 1], [3, 3, 3]))
    t.update(_census(2, [1, 1, 0], [2, 2, 1]))                 # 2 stops
    t.update(_census(3, [1, 1, 0], [2, 2, 0]))                 # gone after 1 round
    t.update(_census(4, [1, 1, 1], [2, 2, 1]))                 # the address runs again (a first start_node of a test)
    t.update(_census(6, [1, 1, 1], [3, 3, 3]))                 # everywhere after 2 rounds
    t.update(_census(7, [1, 1, 0], [2, 2, 2]))                 # stops again
    t.update(_census(10, [1, 1, 0], [2, 2, 0]))                # gone after 3 rounds
    assert t.earlier_stopped == [(2, {"at": 2, "first_dropped": 2, "gone": 3})]
    assert t.stopped[2] == {"at": 7, "first_dropped": 10, "gone": 10}
    lat = t.latencies()
    assert sorted(lat["gone"].tolist()) == [1, 3] and lat["everywhere"].tolist() == [2] and lat["open_gone"] == 0


def test_tracker_gone_on_stop_start_equals_rows():
    """`gone` of the stopped ids 5 and 17 = the first round in which no running row of the oracle holds them."""
    case, rounds = CASES["stop_start"]
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        parity.setup(o, case)
        t = Tracker()
        first_unheld = {}
        for r in range(rounds):
            parity.apply_events((o,), case, r)
            o.step(1)
            t.update(o.census())
            rows, running = o.rows(), o.scalars()[:, 0] != 0
            for j in (5, 17):
                if not running[j] and j not in first_unheld and not rows[running][:, j].any():
                    first_unheld[j] = o.stats()["round"]
        assert set(first_unheld) == {5, 17}
        for j in (5, 17):
            assert t.stopped[j]["gone"] == first_unheld[j]
            assert t.stopped[j]["at"] == 3                     # stopped by the call of round 2, seen after that round
            assert t.stopped[j]["at"] <= t.stopped[j]["first_dropped"] <= t.stopped[j]["gone"]
        assert 120 in t.started and t.started[120]["everywhere"] >= t.started[120]["at"]
