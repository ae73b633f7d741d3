"""The latency census on the CPU (kaboodle_amd/latency.py): the numpy reference on hand-made peer_states arrays with
the expected result written out, and on the oracle against a plain dictionary count over peer_states()."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

import parity
from kaboodle_amd._ffi import KB_LATENCY_NONE, KbLatCensus, Sim
from kaboodle_amd.latency import (KB_CENSUS_NONE, KB_LAT_HIST, SUMMARY_FIELDS, bucket, latency_census_of_arrays,
                                  latency_census_of_states, latency_census_ref)

NONE = KB_CENSUS_NONE
NL = KB_LATENCY_NONE
STD = {n: (c, r) for n, c, r in parity.standard_cases()}


def hist(**bins) -> list[int]:
    h = [0] * KB_LAT_HIST
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_reference_on_hand_made_states():
    # observers 0, 2, 3 of a capacity-5 mesh; id 1 is not running (no row), id 4 is known on hearsay alone
    states = {0: ([0, 1, 2, 4], [NL, 2, 4, NL]),
              2: ([0, 2, 3], [1000, NL, 2]),
              3: ([0, 1, 2, 3, 4], [4, 805, 2, NL, NL])}
    r = latency_census_of_states(states, 5, round_=7)
    assert tuple(r.summary) == SUMMARY_FIELDS
    assert r.summary == {"round": 7, "observers": 3, "measured": 7, "sum_ms": 1819, "min_ms": 2, "max_ms": 1000,
                         "max_peer": 0, "measured_ids": 4, "hist": hist(b2=3, b3=2, b10=2), "orphans": 0}
    assert r.measured_by.tolist() == [2, 2, 2, 1, 0] and r.measured_by.dtype == np.uint32
    assert r.sum_ms.tolist() == [1004, 807, 6, 2, 0] and r.sum_ms.dtype == np.uint64
    assert r.min_ms.tolist() == [4, 2, 2, 2, NONE] and r.max_ms.tolist() == [1000, 805, 4, 2, 0]
    assert r.measured.tolist() == [2, 0, 2, 3, 0] and r.row_sum_ms.tolist() == [6, 0, 1002, 811, 0]
    assert r.row_sum_ms.dtype == np.uint64
    s = latency_census_of_states(states, 5, arrays=False)
    assert s.measured_by is None and s.row_sum_ms is None and s.summary["round"] == -1
    assert {k: v for k, v in s.summary.items() if k != "round"} == {k: v for k, v in r.summary.items() if k != "round"}
    # same_as names what differs
    assert not r.same_as(latency_census_of_states(states, 5, round_=7))
    d = r.same_as(latency_census_of_states({**states, 2: ([0, 2, 3], [1000, NL, 3])}, 5, round_=7))
    assert any(x.startswith("summary.sum_ms") for x in d) and any(x.startswith("max_ms:") for x in d)


def test_reference_histogram_bucket_edges():
    # 0, 1, then 2^k - 1 and 2^k for every k up to 15, and 65534 (the clamp of the EWMA): one observer, one peer each
    vals = [0, 1] + [v for k in range(1, 16) for v in ((1 << k) - 1, 1 << k)] + [65535 - 1]
    vals = sorted(set(vals))
    want = [0] * KB_LAT_HIST
    want[0] = 1                                         # 0
    for b in range(1, 17):                              # bucket b: 2^(b-1) .. 2^b - 1
        want[b] = sum(1 for v in vals if (1 << (b - 1)) <= v < (1 << b))
    assert want == [1, 1] + [2] * 15                    # bucket 16: 32768 and 65534 (32767 is the top of bucket 15)
    assert [bucket(v) for v in (0, 1, 2, 3, 4, 7, 8, 1023, 1024, 32767, 32768, 65534)] == \
        [0, 1, 2, 2, 3, 3, 4, 10, 11, 15, 16, 16]
    r = latency_census_of_states({0: (list(range(len(vals))), vals)}, len(vals))
    assert r.summary["hist"] == want and sum(want) == len(vals) == r.summary["measured"]
    assert (r.summary["min_ms"], r.summary["max_ms"], r.summary["max_peer"]) == (0, 65534, len(vals) - 1)
    assert r.min_ms[0] == 0 and r.measured_by[0] == 1             # a measured 0 is a value, not None


def test_reference_on_an_all_none_mesh():
    for states, cap in (({}, 3), ({0: ([0, 1], [NL, NL]), 1: ([0, 1], [NL, NL])}, 4)):
        r = latency_census_of_states(states, cap)
        assert r.summary == {"round": -1, "observers": len(states), "measured": 0, "sum_ms": 0, "min_ms": NONE,
                             "max_ms": 0, "max_peer": NONE, "measured_ids": 0, "hist": [0] * KB_LAT_HIST, "orphans": 0}
        assert r.min_ms.tolist() == [NONE] * cap and not r.max_ms.any() and not r.measured_by.any()
        assert not r.measured.any() and not r.row_sum_ms.any() and not r.sum_ms.any()


def test_reference_max_peer_tie_rule():
    # ids 1 and 3 share the largest max_ms: the lowest id wins; id 0's larger sum and count do not matter
    states = {0: ([0, 1, 3], [50, 900, 2]), 1: ([0, 1, 3], [60, NL, 900]), 2: ([0], [70])}
    r = latency_census_of_states(states, 4)
    assert r.max_ms.tolist() == [70, 900, 0, 900] and r.summary["max_peer"] == 1 and r.summary["max_ms"] == 900
    # a single measured 0: max_ms is 0 and still names its peer
    z = latency_census_of_states({2: ([1], [0])}, 3)
    assert (z.summary["max_peer"], z.summary["max_ms"], z.summary["min_ms"]) == (1, 0, 0)


def test_reference_on_a_whole_table():
    # 3 ids x 4 rows, peer-major; row 3 is not running; (row 1, id 2) holds a value under a clear bit: an orphan
    L = 0xFFFF
    lat = np.array([[L, 2, 4, 9], [7, L, L, 9], [L, 1000, 65534, 9]], dtype=np.uint16)
    member = np.array([[1, 1, 0], [1, 1, 0], [1, 0, 1], [1, 1, 1]], dtype=np.uint8)
    r = latency_census_of_arrays(lat, member, [1, 1, 1, 0])
    assert r.summary == {"round": -1, "observers": 3, "measured": 4, "sum_ms": 2 + 4 + 7 + 65534, "min_ms": 2,
                         "max_ms": 65534, "max_peer": 2, "measured_ids": 3, "hist": hist(b2=1, b3=2, b16=1), "orphans": 1}
    assert r.measured_by.tolist() == [2, 1, 1] and r.measured.tolist() == [1, 1, 2, 0]
    assert r.row_sum_ms.tolist() == [7, 2, 4 + 65534, 0]


def test_ctypes_mirror_matches_the_header():
    assert C.sizeof(KbLatCensus) == 216
    assert KbLatCensus.hist.offset == 40 and KbLatCensus.orphans.offset == 176 and KbLatCensus.reserved.offset == 184


def dictionary_count(sim: Sim):
    running = np.flatnonzero(sim.scalars()[:, 0] != 0).tolist()
    by_peer, by_row = collections.defaultdict(list), collections.defaultdict(list)
    for i in running:
        for peer, _state, _since, lat, _ident in sim.peer_states(i):
            if lat != KB_LATENCY_NONE:
                by_peer[peer].append(lat)
                by_row[i].append(lat)
    return running, by_peer, by_row


def test_reference_equals_dictionary_count_on_the_oracle():
    case, rounds = STD["churn_loss_512"]
    case = parity.with_cfg(case, track_latency=1)
    last_faulty = case["cfg"].fault_end_round - 1
    cap = case["cfg"].capacity
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        assert "sim_latency_census" not in o.lib.fn
        for r in range(rounds):
            o.step(1)
            if r % 6 and r != last_faulty and r != rounds - 1:
                continue                                 # every 6th round, the last faulty one and the last
            c = o.latency_census()                       # the oracle has no kb_sim_latency_census: the reference answers
            running, by_peer, by_row = dictionary_count(o)
            s = c.summary
            allv = [v for vs in by_peer.values() for v in vs]
            assert s["round"] == o.stats()["round"] and s["observers"] == len(running) and s["orphans"] == 0
            assert s["measured"] == len(allv) and s["sum_ms"] == sum(allv) and s["measured_ids"] == len(by_peer)
            assert s["min_ms"] == (min(allv) if allv else NONE) and s["max_ms"] == (max(allv) if allv else 0)
            top = max(allv) if allv else None
            assert s["max_peer"] == (min(p for p, vs in by_peer.items() if max(vs) == top) if allv else NONE)
            h = [0] * KB_LAT_HIST
            for v in allv:
                h[0 if v == 0 else int(np.floor(np.log2(v))) + 1] += 1
            assert s["hist"] == h
            for j in range(cap):
                vs = by_peer.get(j, [])
                assert (c.measured_by[j], c.sum_ms[j]) == (len(vs), sum(vs))
                assert (c.min_ms[j], c.max_ms[j]) == ((min(vs), max(vs)) if vs else (NONE, 0))
                ws = by_row.get(j, [])
                assert (c.measured[j], c.row_sum_ms[j]) == (len(ws), sum(ws))
            assert not c.same_as(latency_census_ref(o))
            if r == last_faulty:
                # the case is not vacuous: something is measured, direct Acks (2 ms) and a slower population (late
                # or indirect Acks, EWMA-mixed) fall into different buckets, and some id is held on hearsay
                known_by = o.census().known_by
                assert s["measured"] > 0
                assert sum(1 for x in s["hist"] if x) >= 2 and s["hist"][2] > 0, s["hist"]
                assert (c.measured_by <= known_by).all() and (c.measured_by < known_by).any()
