"""The reciprocity census on the CPU oracle (kaboodle_amd/reciprocity.py): reciprocity_ref against a direct count from
peers() of every node, the identities that tie it to the view census, the order of the pair list and its overflow
rule."""
from __future__ import annotations

import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import Sim
from kaboodle_amd.reciprocity import KB_CENSUS_NONE, SUMMARY_FIELDS, Reciprocity

CASES = {n: (c, r) for n, c, r in parity.standard_cases()}


def direct_count(sim: Sim):
    """mutual / lacks / lacked_by and the mutual pairs straight from the definitions, through peers() and the
    is-running scalars: sets and loops, no matrix."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    obs = np.flatnonzero(running).tolist()
    view = {i: set(sim.peers(i)) for i in obs}
    mu, lk, lb = (np.zeros(C, dtype=np.uint32) for _ in range(3))
    pairs = []
    for i in obs:
        for j in obs:
            if i == j:
                continue
            i_lacks, j_lacks = j not in view[i], i not in view[j]
            mu[i] += i_lacks and j_lacks
            lk[i] += i_lacks and not j_lacks
            lb[i] += j_lacks and not i_lacks
            if i < j and i_lacks and j_lacks:
                pairs.append((i, j))
    return running, mu, lk, lb, pairs


def check_against_direct(sim: Sim) -> Reciprocity:
    r = sim.reciprocity()                               # the oracle has no kb_sim_reciprocity: reciprocity_ref answers
    running, mu, lk, lb, pairs = direct_count(sim)
    assert np.array_equal(r.mutual, mu) and np.array_equal(r.lacks, lk) and np.array_equal(r.lacked_by, lb)
    s = r.summary
    assert tuple(s) == SUMMARY_FIELDS
    assert s["round"] == sim.stats()["round"] and s["observers"] == int(running.sum())
    assert s["mutual_pairs"] == len(pairs) and s["oneway_pairs"] == int(lk.sum())
    assert s["rows_mutual"] == int((mu > 0).sum()) and s["rows_oneway"] == int((lk > 0).sum())
    if pairs:
        top = int(mu.max())
        assert (s["max_mutual_row"], s["max_mutual"]) == (int(np.flatnonzero(mu == top)[0]), top)
    else:
        assert (s["max_mutual_row"], s["max_mutual"]) == (KB_CENSUS_NONE, 0)
    # the pair list: ascending by (i, j), i < j, as long as the total
    assert s["pairs_listed"] == len(pairs) == len(r.pairs)
    assert r.pairs.tolist() == [list(p) for p in sorted(pairs)]
    # the identities of include/kaboodle_reciprocity.h
    c = sim.census()
    assert np.array_equal(r.mutual + r.lacks, c.missing)
    assert int(r.lacks.sum()) == int(r.lacked_by.sum())
    assert int(r.mutual.sum()) == 2 * s["mutual_pairs"]
    assert not r.mutual[~running].any() and not r.lacks[~running].any() and not r.lacked_by[~running].any()
    return r


@pytest.mark.parametrize("name", ["stop_start", "fresh_ids", "converged_loss_256", "join_64"])
def test_reciprocity_ref_equals_direct_count_every_round(name):
    case, rounds = CASES[name]
    seen = []
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        assert "sim_reciprocity" not in o.lib.fn
        parity.setup(o, case)
        for r in range(rounds):
            parity.apply_events((o,), case, r)
            o.step(1)
            s = check_against_direct(o).summary
            seen.append((s["mutual_pairs"], s["oneway_pairs"]))
    # the cases are not vacuous
    if name == "join_64":
        assert seen[0] == (64 * 63 // 2, 0)             # after the first round nobody knows anybody
        assert all(p == (0, 0) for p in seen[1:])
    else:
        assert any(m > 0 for m, _ in seen), seen
    if name in ("stop_start", "converged_loss_256"):
        assert any(w > 0 for _, w in seen), seen


def test_pair_list_overflow_lists_nothing():
    case, rounds = CASES["converged_loss_256"]
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        parity.setup(o, case)
        o.step(rounds)
        full = o.reciprocity()
        n = full.summary["mutual_pairs"]
        assert n > 1 and full.summary["pairs_listed"] == n == len(full.pairs)
        exact = o.reciprocity(max_pairs=n)              # the total fits exactly: listed
        assert exact.summary["pairs_listed"] == n and np.array_equal(exact.pairs, full.pairs)
        short = o.reciprocity(max_pairs=n - 1)          # one short: nothing is listed, the total still reported
        assert short.summary["pairs_listed"] == 0 and len(short.pairs) == 0
        assert short.summary["mutual_pairs"] == n
        assert np.array_equal(short.mutual, full.mutual) and np.array_equal(short.lacks, full.lacks)
        assert [d for d in short.same_as(full)] == [f"summary.pairs_listed: 0 != {n}",
                                                    f"pairs: 0 listed != {n} listed, or other entries"]
        assert not full.same_as(exact)
        # arrays=False: the summary alone and nothing listed, as the device call with every array NULL answers
        bare = o.reciprocity(arrays=False)
        assert bare.summary == {**full.summary, "pairs_listed": 0}
        assert bare.mutual is None and bare.lacks is None and bare.lacked_by is None and bare.pairs is None
