"""The fingerprint-class census on the CPU (kaboodle_amd/classes.py): the numpy reference on hand-made arrays with the
expected result written out, and on the oracle against a plain dictionary count with the invariants of
include/kaboodle_classes.h every round."""
from __future__ import annotations

import collections

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd._ffi import KbFpClass, KbFpClasses, Sim
from kaboodle_amd.classes import KB_CENSUS_NONE, SUMMARY_FIELDS, FpClasses, fp_classes_of_arrays, fp_classes_ref

NONE = KB_CENSUS_NONE


def hist(**bins) -> list[int]:
    h = [0] * 32
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_reference_on_hand_made_arrays():
    #        id:  0   1   2   3   4   5   6   7   8   9
    fps = [7, 5, 7, 0, 5, 9, 0, 5, 7, 4]
    run = [1, 1, 1, 1, 1, 0, 1, 0, 0, 1]
    # running: 7 {0, 2}, 5 {1, 4}, 0 {3, 6}, 4 {9}.  Ids 5, 7, 8 are not running: the 9, 5 and 7 in their slots
    # count for nothing (5 and 7 are running rows' keys as well).  Three classes tie at size 2: fp ascending.
    r = fp_classes_of_arrays(fps, run, true_fp=5, top=16, round_=12)
    assert tuple(r.summary) == SUMMARY_FIELDS
    assert r.summary == {"round": 12, "observers": 7, "classes": 4, "largest": 2, "singletons": 1, "true_fp": 5,
                         "true_size": 2, "true_rank": 1, "size_hist": hist(b0=1, b1=3), "listed": 4,
                         "listed_observers": 7}
    assert r.classes.dtype == np.uint32 and r.classes.tolist() == [[0, 2, 3], [5, 2, 1], [7, 2, 0], [4, 1, 9]]
    assert r.rep.tolist() == [0, 1, 0, 3, 1, NONE, 3, NONE, NONE, 9]
    assert r.size.tolist() == [2, 2, 2, 2, 2, 0, 2, 0, 0, 1]
    # a short list: the first two in canonical order; the summary still covers every class
    s = fp_classes_of_arrays(fps, run, true_fp=4, top=2, arrays=False)
    assert s.classes.tolist() == [[0, 2, 3], [5, 2, 1]] and s.rep is None and s.size is None
    assert (s.summary["listed"], s.summary["listed_observers"]) == (2, 4)
    assert (s.summary["true_size"], s.summary["true_rank"], s.summary["round"]) == (1, 3, -1)
    # the true fingerprint is a stopped row's only: no such class
    t = fp_classes_of_arrays(fps, run, true_fp=9, top=0)
    assert (t.summary["true_size"], t.summary["true_rank"], t.summary["listed"]) == (0, NONE, 0)
    assert t.classes.shape == (0, 3)
    # same_as names what differs
    assert not r.same_as(fp_classes_of_arrays(fps, run, 5, round_=12))
    d = r.same_as(fp_classes_of_arrays(fps, [1, 1, 1, 1, 1, 0, 1, 0, 1, 1], 5, round_=12))
    assert any(x.startswith("summary.observers") for x in d) and any(x.startswith("size:") for x in d)


def test_reference_on_an_empty_mesh():
    for fps, run in (([], []), ([3, 3, 0], [0, 0, 0])):
        r = fp_classes_of_arrays(fps, run, true_fp=0)
        assert r.summary == {"round": -1, "observers": 0, "classes": 0, "largest": 0, "singletons": 0, "true_fp": 0,
                             "true_size": 0, "true_rank": NONE, "size_hist": [0] * 32, "listed": 0,
                             "listed_observers": 0}
        assert r.classes.shape == (0, 3) and r.rep.tolist() == [NONE] * len(fps) and r.size.tolist() == [0] * len(fps)


def test_reference_extreme_keys_and_sizes():
    fps = np.array([0xFFFFFFFF] * 5 + [0] * 5 + [1 << 31] * 9, dtype=np.uint32)
    r = fp_classes_of_arrays(fps, np.ones(19), true_fp=0xFFFFFFFF)
    assert r.classes.tolist() == [[1 << 31, 9, 10], [0, 5, 5], [0xFFFFFFFF, 5, 0]]
    assert (r.summary["true_rank"], r.summary["size_hist"]) == (2, hist(b2=2, b3=1))


def test_ctypes_mirrors_match_the_header():
    import ctypes as C
    assert C.sizeof(KbFpClass) == 16 and C.sizeof(KbFpClasses) == 200
    assert KbFpClasses.size_hist.offset == 32 and KbFpClasses.listed.offset == 160 and KbFpClasses.reserved.offset == 168


def dictionary_count(sim: Sim):
    fps, running = sim.fingerprints(), sim.scalars()[:, 0] != 0
    members = collections.defaultdict(list)
    for i in np.flatnonzero(running).tolist():
        members[int(fps[i])].append(i)
    return running, members


def check_round(sim: Sim) -> FpClasses:
    r = sim.fp_classes(top=1024)                        # the oracle has no kb_sim_fp_classes: fp_classes_ref answers
    running, members = dictionary_count(sim)
    s = r.summary
    want = sorted(((fp, len(m), m[0]) for fp, m in members.items()), key=lambda c: (-c[1], c[0]))
    assert r.classes.tolist() == [list(c) for c in want]
    assert s["round"] == sim.stats()["round"] and s["observers"] == int(running.sum()) and s["classes"] == len(members)
    assert s["largest"] == (want[0][1] if want else 0) and s["singletons"] == sum(c[1] == 1 for c in want)
    tfp = sim.true_fingerprint()
    rank = [k for k, c in enumerate(want) if c[0] == tfp]
    assert s["true_fp"] == tfp and s["true_rank"] == (rank[0] if rank else NONE)
    assert s["true_size"] == (want[rank[0]][1] if rank else 0)
    # the invariants
    assert int(r.classes[:, 1].sum()) == s["observers"] == s["listed_observers"] and s["listed"] == s["classes"]
    assert sum(s["size_hist"]) == s["classes"]
    obs = np.flatnonzero(running)
    assert (r.rep[~running] == NONE).all() and not r.size[~running].any()
    assert np.array_equal(r.rep[r.rep[obs]], r.rep[obs])
    shared = collections.Counter(r.rep[obs].tolist())
    assert r.size[obs].tolist() == [shared[int(x)] for x in r.rep[obs]]
    assert not r.same_as(fp_classes_ref(sim, top=1024))
    return r


@pytest.mark.parametrize("name", ["join32", "partition"])
def test_reference_equals_dictionary_count_every_round(name):
    sc = scenarios.BY_NAME[name]
    seen = []
    with Sim(parity.oracle_lib(), sc["cfg"]) as o:
        assert "sim_fp_classes" not in o.lib.fn
        scenarios.setup(o, sc)
        for r in range(sc["rounds"]):
            scenarios.apply_events(o, sc, r)
            o.step(1)
            s = check_round(o).summary
            seen.append((s["classes"], s["largest"]))
    # the scenario is not trivial: several classes at some round, a class of more than one row at some round
    assert any(c > 1 for c, _ in seen), seen
    assert any(big > 1 for _, big in seen), seen
