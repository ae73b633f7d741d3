"""The gap list and the holders query on the CPU (kaboodle_amd/gaps.py): the header against the ctypes mirror,
gaps_ref / holders_ref on a hand-made table with the expected lists written out, against one-branch-per-cell loops on a
random table, and against the view census's counts on the oracle after every round."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd import _ffi
from kaboodle_amd._ffi import KbGaps, Sim
from kaboodle_amd.census import census_ref
from kaboodle_amd.gaps import KB_HOLDERS_MAX, SUMMARY_FIELDS, gaps_ref, holders_ref, same_gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_ctypes_mirror_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "kaboodle_gaps.h")).read()
    for fn in ("kb_sim_gaps", "kb_sim_gaps_device_ms", "kb_sim_holders", "kb_sim_holders_device_ms"):
        assert re.search(rf"\bint {fn}\(", hdr), fn
        assert fn[3:] in _ffi._OPTIONAL
        assert fn not in open(os.path.join(ROOT, "include", "kaboodle_sim.h")).read()   # no oracle twin is owed
    assert int(re.search(r"#define KB_HOLDERS_MAX (\d+)", hdr).group(1)) == KB_HOLDERS_MAX == _ffi.KB_HOLDERS_MAX == 1024
    body = re.search(r"typedef struct kb_gaps \{(.*?)\} kb_gaps;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.match(r"\w+", d.strip()).group(0) for line in body.split(";") if line.strip()
             for d in line.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in KbGaps._fields_]
    assert C.sizeof(KbGaps) == 2 * 4 + 4 * 8 + 2 * 4 + 4 * 8 == 80
    assert KbGaps.missing.offset == 8 and KbGaps.stale_listed.offset == 32 and KbGaps.rows_missing.offset == 40
    assert KbGaps.reserved.offset == 48
    assert tuple(KbGaps().as_dict()) == SUMMARY_FIELDS


# 6 rows x 40 ids.  Ids 0, 1, 2, 4 and 33 run; 3 is dead, 5 is dead too, 39 is external; the others never ran.
HAND_RUN = [0, 1, 2, 4, 33]
HAND_EXT = [39]
HAND_ROWS = [{0, 1, 2, 4, 33},        # exact
             {1, 0, 3, 39},           # lacks 2, 4, 33; holds the dead 3; the external id is in neither list
             {0, 1, 4, 33, 5, 38},    # does not hold itself: (2, 2) is missing; holds the dead 5 and 38
             {0, 1, 2, 3, 4, 33},     # the row of a dead id: not an observer, whatever it holds
             {4},                     # holds only itself
             {0, 1, 2, 4, 33, 5}]     # a dead id's row (5 < 6): not read
HAND_MISSING = [(1, 2), (1, 4), (1, 33), (2, 2), (4, 0), (4, 1), (4, 2), (4, 33)]
HAND_STALE = [(1, 3), (2, 5), (2, 38)]


def hand():
    rows = np.zeros((6, 40), dtype=np.uint8)
    for i, ids in enumerate(HAND_ROWS):
        rows[i, list(ids)] = 7                                         # any stamp != 0 is a member
    run, ext = np.zeros(40, dtype=bool), np.zeros(40, dtype=bool)
    run[HAND_RUN], ext[HAND_EXT] = True, True
    full = np.zeros((40, 40), dtype=np.uint8)                          # rows 6.. hold nothing: 33 lacks everything
    full[:6] = rows
    return full, run, ext


def test_refs_by_hand():
    rows, run, ext = hand()
    g = gaps_ref(rows, run, ext, round_=9)
    row33 = [(33, j) for j in HAND_RUN]                                # the observer whose row is empty
    assert g["missing_pairs"].tolist() == [list(p) for p in HAND_MISSING + row33]
    assert g["stale_pairs"].tolist() == [list(p) for p in HAND_STALE]
    assert g["missing_pairs"].dtype == g["stale_pairs"].dtype == np.uint32
    assert {k: g[k] for k in SUMMARY_FIELDS} == {"round": 9, "observers": 5, "missing": 13, "stale": 3, "missing_listed": 13,
                                                  "stale_listed": 3, "rows_missing": 4, "rows_stale": 2}
    capped = gaps_ref(rows, run, ext, max_pairs=12)                    # each list decides for itself
    assert capped["missing_pairs"] is None and capped["missing_listed"] == 0 and capped["missing"] == 13
    assert capped["stale_pairs"].tolist() == g["stale_pairs"].tolist() and capped["stale_listed"] == 3
    assert gaps_ref(rows, run, ext, max_pairs=13)["missing_listed"] == 13
    assert same_gaps(g, g) == [] and same_gaps(g, capped)
    off, who = holders_ref(rows, run, [0, 3, 39, 5, 2, 20, 0])
    assert off.tolist() == [0, 3, 4, 5, 6, 7, 7, 10] and off.dtype == np.uint64 and who.dtype == np.uint32
    assert who.tolist() == [0, 1, 2, 1, 1, 2, 0, 0, 1, 2]             # 3's own dead row and row 5 hold ids: not observers
    assert holders_ref(rows, run, [0, 3], max_rows=3)[1] is None and holders_ref(rows, run, [0, 3], max_rows=4)[1] is not None


def test_refs_against_per_cell_loops():
    rng = np.random.default_rng(5)
    C_, W = 40, 70                                                     # 70 columns: those past the capacity are ignored
    rows = (rng.random((C_, W)) < 0.6).astype(np.uint8) * rng.integers(1, 255, (C_, W), dtype=np.uint8)
    run = rng.random(C_) < 0.7
    ext = ~run & (rng.random(C_) < 0.3)
    miss, stale = [], []
    for i in range(C_):
        for j in range(C_):
            if run[i] and run[j] and rows[i, j] == 0:
                miss.append([i, j])
            if run[i] and rows[i, j] != 0 and not run[j] and not ext[j]:
                stale.append([i, j])
    g = gaps_ref(rows, run, ext)
    assert g["missing_pairs"].tolist() == miss and g["stale_pairs"].tolist() == stale and miss and stale
    assert (g["missing"], g["stale"], g["observers"]) == (len(miss), len(stale), int(run.sum()))
    assert g["rows_missing"] == len({p[0] for p in miss}) and g["rows_stale"] == len({p[0] for p in stale})
    ids = list(range(C_)) + [7, 7]
    off, who = holders_ref(rows, run, ids)
    for q, j in enumerate(ids):
        assert who[int(off[q]):int(off[q + 1])].tolist() == [i for i in range(C_) if run[i] and rows[i, j] != 0]


@pytest.mark.parametrize("name", ["stop_start", "partition", "churn40"])
def test_lists_agree_with_the_view_census_on_the_oracle(name):
    sc = scenarios.BY_NAME[name]
    seen = 0
    with Sim(parity.oracle_lib(), sc["cfg"]) as o:
        assert "sim_gaps" not in o.lib.fn and "sim_holders" not in o.lib.fn     # the references answer through the same calls
        scenarios.setup(o, sc)
        for r in range(sc["rounds"]):
            scenarios.apply_events(o, sc, r)
            o.step(1)
            g, c = o.gaps(max_pairs=o.capacity ** 2), census_ref(o)
            assert g["round"] == c.summary["round"] and g["observers"] == c.summary["observers"]
            assert (g["missing"], g["stale"]) == (c.summary["missing"], c.summary["stale"])
            for kind, want in (("missing", c.missing), ("stale", c.stale)):
                assert np.array_equal(np.bincount(g[kind + "_pairs"][:, 0], minlength=o.capacity), want), (r, kind)
            off, _ = o.holders(list(range(o.capacity)))
            assert np.array_equal(np.diff(off).astype(np.uint32), c.known_by), r
            seen += g["missing"] + g["stale"]
    assert seen > 0
