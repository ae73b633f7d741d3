"""The contact-age census on the CPU (kaboodle_amd/age.py): the numpy references on a hand-made table with the expected
result written out, against plain loops on a random table and over peer_states() of the oracle after every round,
and the identities that tie the census to the view census."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import KB_VARIANT_SPARSE_ROWS, KbAgeCensus, Sim
from kaboodle_amd.age import (ARRAYS, EOFF, EPOCH, INT32_MIN, KB_AGE_HIST, KB_CENSUS_NONE, SHARE_AGE, SUMMARY_FIELDS,
                              AgeCensus, age_census_of_arrays, age_census_ref, since_of_byte)

NONE = KB_CENSUS_NONE
STD = {n: (c, r) for n, c, r in parity.standard_cases()}
ORACLE_CASES = {"config1_2x2": STD["config1_2x2"], "join_loss_300_ids": STD["join_loss_300_ids"],
                "stop_start": STD["stop_start"], "partition_heal": STD["partition_heal"],
                "partition_heal_sparse": (parity.with_cfg(STD["partition_heal"][0], variant=KB_VARIANT_SPARSE_ROWS),
                                          STD["partition_heal"][1])}


def hist(**bins) -> list[int]:
    h = [0] * KB_AGE_HIST
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_ctypes_mirror_matches_the_header():
    assert C.sizeof(KbAgeCensus) == 2176
    assert KbAgeCensus.cells.offset == 8 and KbAgeCensus.dead_suspects.offset == 48 and KbAgeCensus.unheard_ids.offset == 80
    assert KbAgeCensus.oldest_heard.offset == 88 and KbAgeCensus.hist.offset == 96 and KbAgeCensus.reserved.offset == 2144


def test_window_bound():
    # the freshest byte of round r is r % 64 + 192 <= 255, the oldest windowed byte is 3
    for r in (0, 1, 63, 64, 127, 128, 1000):
        top = r % EPOCH + EOFF
        assert top <= 255 and since_of_byte(top, r + 1) == r
        ages = [r - since_of_byte(b, r + 1) for b in range(3, top + 1)]
        assert min(ages) == 0 and max(ages) == top - 3 <= 252 < KB_AGE_HIST
    assert since_of_byte(192, 0) == 0                    # before the first round: decoded as round 0


def test_reference_on_a_hand_made_table():
    # round 12: r = 11, Known(11) is byte 203, fresh from byte 194 (age 9).  Row 2 is not running; (1, 3) holds a byte
    # under a clear member bit; the diagonal is the self entry.
    stamp = np.array([[203, 1, 2, 203], [194, 203, 193, 3], [203, 203, 203, 203]], dtype=np.uint8)
    member = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]], dtype=np.uint8)
    r = age_census_of_arrays(stamp, member, [1, 1, 0], 12)
    assert tuple(r.summary) == SUMMARY_FIELDS
    assert r.summary == {"round": 12, "observers": 2, "cells": 5, "suspects": 1, "ancient": 1, "windowed": 3, "fresh": 2,
                         "dead_suspects": 0, "dead_ancient": 1, "dead_windowed": 2, "dead_fresh": 1, "unheard_ids": 1,
                         "oldest_heard_id": 1, "oldest_heard": INT32_MIN, "hist": hist(a0=1, a9=1, a10=1)}
    assert r.suspected_by.tolist() == [0, 1, 0, 0] and r.ancient_by.tolist() == [0, 0, 1, 0]
    assert r.windowed_by.tolist() == [1, 0, 1, 1] and r.fresh_by.tolist() == [1, 0, 0, 1]
    assert r.last_heard.tolist() == [2, INT32_MIN, 1, 11] and r.last_heard.dtype == np.int32
    assert r.suspects.tolist() == [1, 0, 0] and r.ancient.tolist() == [1, 0, 0]
    assert r.windowed.tolist() == [1, 2, 0] and r.fresh.tolist() == [1, 1, 0] and r.fresh.dtype == np.uint32
    s = age_census_of_arrays(stamp, member, [1, 1, 0], 12, arrays=False)
    assert s.summary == r.summary and all(getattr(s, n) is None for n in ARRAYS)
    # same_as names what differs
    assert not r.same_as(age_census_of_arrays(stamp, member, [1, 1, 0], 12))
    stamp[0, 3] = 2
    d = r.same_as(age_census_of_arrays(stamp, member, [1, 1, 0], 12))
    assert any(x.startswith("summary.ancient") for x in d) and any(x.startswith("last_heard:") for x in d)
    # nothing runs
    e = age_census_of_arrays(stamp, member, [0, 0, 0], 12)
    assert (e.summary["oldest_heard_id"], e.summary["oldest_heard"], e.summary["cells"]) == (NONE, INT32_MIN, 0)
    # a byte past Known(r) has no age
    stamp[0, 3] = 204
    with pytest.raises(ValueError):
        age_census_of_arrays(stamp, member, [1, 1, 0], 12)


def loops_of_arrays(stamp, member, running, round_):
    """The census of a table by one branch per cell."""
    n_rows, n_ids = stamp.shape
    r = round_ - 1 if round_ > 0 else 0
    e0 = (r // EPOCH) * EPOCH
    by = np.zeros((4, n_ids), dtype=np.uint32)
    rw = np.zeros((4, n_rows), dtype=np.uint32)
    lh = [INT32_MIN] * n_ids
    h = [0] * KB_AGE_HIST
    for i in range(n_rows):
        if not running[i]:
            continue
        for j in range(n_ids):
            b = int(stamp[i, j])
            if j == i or not member[i, j] or b == 0:
                continue
            if b == 1:
                c = [0]
            elif b == 2:
                c = [1]
            else:
                since = b + e0 - EOFF
                age = r - since
                h[age] += 1
                lh[j] = max(lh[j], since)
                c = [2, 3] if age < SHARE_AGE else [2]
            for k in c:
                by[k, j] += 1
                rw[k, i] += 1
    return by, rw, lh, h


def test_reference_equals_loops_on_a_random_table():
    rng = np.random.default_rng(17)
    n_rows, n_ids, round_ = 40, 70, 64                   # r = 63: every byte up to 255 is a valid stamp
    stamp = rng.integers(0, 256, size=(n_rows, n_ids)).astype(np.uint8)
    stamp[rng.random((n_rows, n_ids)) < 0.3] = rng.integers(0, 3)
    member = (rng.random((n_rows, n_ids)) < 0.7).astype(np.uint8)
    running = (rng.random(n_rows) < 0.8).astype(np.uint8)
    c = age_census_of_arrays(stamp, member, running, round_)
    by, rw, lh, h = loops_of_arrays(stamp, member, running, round_)
    for k, (a, b) in enumerate(zip(("suspected_by", "ancient_by", "windowed_by", "fresh_by"),
                                   ("suspects", "ancient", "windowed", "fresh"))):
        assert getattr(c, a).tolist() == by[k].tolist(), a
        assert getattr(c, b).tolist() == rw[k].tolist(), b
    assert c.last_heard.tolist() == lh and c.summary["hist"] == h
    s = c.summary
    assert (s["suspects"], s["ancient"], s["windowed"], s["fresh"]) == tuple(int(by[k].sum()) for k in range(4))
    assert s["cells"] == s["suspects"] + s["ancient"] + s["windowed"] and s["observers"] == int(running.sum())
    assert sum(h) == s["windowed"] > 0 and sum(h[:SHARE_AGE]) == s["fresh"] > 0 and s["suspects"] > 0 and s["ancient"] > 0
    run_ids = [j for j in range(n_ids) if j < n_rows and running[j]]
    assert s["unheard_ids"] == sum(1 for j in run_ids if by[2, j] == 0)
    assert s["oldest_heard"] == min(lh[j] for j in run_ids)
    assert s["oldest_heard_id"] == min(j for j in run_ids if lh[j] == s["oldest_heard"])
    dead = [j for j in range(n_ids) if j not in run_ids]
    assert s["dead_windowed"] == sum(int(by[2, j]) for j in dead) and s["dead_suspects"] == sum(int(by[0, j]) for j in dead)


def loops_of_peer_states(sim: Sim):
    """The census from plain loops over peer_states(): dictionaries, no numpy."""
    cap = sim.capacity
    sc = sim.scalars()
    running = [i for i in range(cap) if sc[i, 0]]
    round_ = sim.stats()["round"]
    r = round_ - 1 if round_ > 0 else 0
    ext = set(sim.external)
    by = [[0] * cap for _ in range(4)]
    rw = [[0] * cap for _ in range(4)]
    lh = [INT32_MIN] * cap
    h = [0] * KB_AGE_HIST
    for i in running:
        for peer, state, since, _lat, _ident in sim.peer_states(i):
            if peer == i:
                continue
            if state != 0:
                c = [0]
            elif since == INT32_MIN:
                c = [1]
            else:
                assert 0 <= r - since < KB_AGE_HIST
                h[r - since] += 1
                lh[peer] = max(lh[peer], since)
                c = [2, 3] if r - since < SHARE_AGE else [2]
            for k in c:
                by[k][peer] += 1
                rw[k][i] += 1
    dead = [j for j in range(cap) if j not in running and j not in ext]
    s = {"round": round_, "observers": len(running), "cells": sum(by[0]) + sum(by[1]) + sum(by[2]),
         "suspects": sum(by[0]), "ancient": sum(by[1]), "windowed": sum(by[2]), "fresh": sum(by[3]),
         "dead_suspects": sum(by[0][j] for j in dead), "dead_ancient": sum(by[1][j] for j in dead),
         "dead_windowed": sum(by[2][j] for j in dead), "dead_fresh": sum(by[3][j] for j in dead),
         "unheard_ids": sum(1 for j in running if by[2][j] == 0)}
    old = min((lh[j] for j in running), default=INT32_MIN)
    s["oldest_heard_id"] = min((j for j in running if lh[j] == old), default=NONE)
    s["oldest_heard"] = old
    s["hist"] = h
    return AgeCensus(s, *(np.array(x, dtype=np.uint32) for x in by), np.array(lh, dtype=np.int32),
                     *(np.array(x, dtype=np.uint32) for x in rw))


def check_identities(sim: Sim, c: AgeCensus) -> None:
    """The four identities of include/kaboodle_age.h, against the view census and the rows."""
    s = c.summary
    assert sum(s["hist"]) == s["windowed"] and sum(s["hist"][:SHARE_AGE]) == s["fresh"]
    known_by = sim.census().known_by
    running = sim.scalars()[:, 0] != 0
    holds_self = np.zeros(sim.capacity, dtype=np.uint32)
    for i in np.flatnonzero(running).tolist():
        row = sim.row(i)
        holds_self[i] = row[i] != 0
        assert int(c.suspects[i]) + int(c.ancient[i]) + int(c.windowed[i]) == int((row != 0).sum()) - int(holds_self[i]), i
    assert np.array_equal(c.suspected_by + c.ancient_by + c.windowed_by, known_by - holds_self)
    assert (c.fresh_by <= c.windowed_by).all() and (c.fresh <= c.windowed).all()
    assert not c.suspects[~running].any() and not c.windowed[~running].any() and not c.ancient[~running].any()


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_reference_equals_plain_loops_on_the_oracle_every_round(name):
    case, rounds = ORACLE_CASES[name]
    seen = {"suspects": 0, "ancient": 0, "windowed": 0}
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        assert "sim_age_census" not in o.lib.fn
        parity.setup(o, case)
        for r in range(rounds):
            parity.apply_events((o,), case, r)
            o.step(1)
            c = o.age_census()                           # the oracle has no kb_sim_age_census: the reference answers
            d = c.same_as(loops_of_peer_states(o))
            assert not d, f"{name} round {r}: " + "; ".join(d[:6])
            assert not c.same_as(age_census_ref(o)) and o.age_census(arrays=False).summary == c.summary
            if r % 5 == 4 or r == rounds - 1:
                check_identities(o, c)
            for k in seen:
                seen[k] += c.summary[k]
    assert seen["windowed"] > 0, name                    # the case exercises the table at all
    if name.startswith("partition_heal"):
        assert seen["suspects"] > 0 and seen["ancient"] > 0, seen
