"""The island census on the CPU (kaboodle_amd/islands.py): the header against the ctypes mirror, islands_ref on a
hand-made matrix with the expected result written out, against a plain flood fill on random matrices, and the
identities that tie the census to the views and to the view census on the oracle after every round."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import parity
import scenarios
from kaboodle_amd import _ffi
from kaboodle_amd._ffi import KB_CENSUS_NONE, KbIslands, Sim
from kaboodle_amd.islands import ARRAYS, KB_ISLANDS_TOP, SUMMARY_FIELDS, Islands, islands_ref

NONE = KB_CENSUS_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = {n: (c, r) for n, c, r in parity.standard_cases()}


def test_exports_and_ctypes_mirror_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "kaboodle_islands.h")).read()
    for fn in ("kb_sim_islands", "kb_sim_islands_device_ms", "kb_islands_of"):
        assert re.search(rf"\bint {fn}\(", hdr), fn
        assert fn[3:] in _ffi._OPTIONAL
    assert int(re.search(r"#define KB_ISLANDS_TOP (\d+)", hdr).group(1)) == KB_ISLANDS_TOP == _ffi.KB_ISLANDS_TOP == 8
    body = re.search(r"typedef struct kb_islands \{(.*?)\} kb_islands;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.match(r"\w+", d.strip()).group(0) for line in body.split(";") if line.strip()
             for d in [line.strip().split(None, 1)[1]]]
    assert names == [n for n, _ in KbIslands._fields_]
    assert C.sizeof(KbIslands) == 8 * 4 + 8 + KB_ISLANDS_TOP * 8 + 2 * 4 + 4 * 8 == 144
    assert KbIslands.unreachable_pairs.offset == 32 and KbIslands.top.offset == 40
    assert KbIslands.sweeps.offset == 104 and KbIslands.reserved.offset == 112
    assert tuple(KbIslands().as_dict()) == SUMMARY_FIELDS
    assert "not of the state" in hdr                       # sweeps: documented as a property of the execution


# 12 ids, 4 and 9 do not run; column 12 is past the capacity.  Every running row holds itself.
HAND_RUN = [1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1]
HAND_ROWS = [{0, 1},            # a one-way edge: 1 does not hold 0
             {1, 2}, {2, 1},    # mutual
             {3, 4, 6, 12},     # 3 and 5 both hold the dead id 4, whose stale row holds both: no bridge
             {3, 4, 5, 7},      # the dead id's row: not read
             {5, 4, 7},         # 5 holds 7 one-way
             {6, 3}, {7},
             {8},               # a singleton that holds only itself: it broadcasts Join again
             {0, 10},           # a dead row holding live ids: nothing
             {10, 9, 12},       # a singleton that holds a dead id: two entries, no re-broadcast
             {11, 2}]           # one-way from above into the first island
HAND_LABEL = [0, 0, 0, 3, NONE, 5, 3, 5, 8, NONE, 10, 0]
HAND_SIZE = [4, 4, 4, 2, 0, 2, 2, 2, 1, 0, 1, 4]


def hand_matrix() -> np.ndarray:
    m = np.zeros((12, 13), dtype=np.uint8)
    for i, ids in enumerate(HAND_ROWS):
        m[i, list(ids)] = 1
    return m


def test_islands_ref_by_hand():
    r = islands_ref(hand_matrix(), HAND_RUN, round_=7)
    assert r.label.tolist() == HAND_LABEL and r.size.tolist() == HAND_SIZE
    assert r.label.dtype == r.size.dtype == np.uint32
    assert tuple(r.summary) == SUMMARY_FIELDS
    assert r.summary == {"round": 7, "observers": 10, "islands": 5, "singletons": 2, "rebroadcasting": 1, "largest": 4,
                         "largest_label": 0, "second": 2, "unreachable_pairs": 4 * 6 + 2 * 8 + 2 * 8 + 9 + 9,
                         "top": [[0, 4], [3, 2], [5, 2], [8, 1], [10, 1], [NONE, 0], [NONE, 0], [NONE, 0]], "sweeps": 0}
    s = islands_ref(hand_matrix(), HAND_RUN, round_=7, arrays=False)
    assert s.summary == r.summary and s.label is None and s.size is None
    assert not r.same_as(Islands({**r.summary, "sweeps": 3}, r.label, r.size))       # sweeps is not compared
    assert r.same_as(Islands({**r.summary, "second": 3}, r.label, r.size))
    nobody = islands_ref(hand_matrix(), [0] * 12)
    assert nobody.summary["islands"] == nobody.summary["observers"] == nobody.summary["largest"] == 0
    assert nobody.summary["largest_label"] == NONE and (nobody.label == NONE).all() and not nobody.size.any()
    assert nobody.summary["top"] == [[NONE, 0]] * 8


def flood_fill(member: np.ndarray, running) -> tuple[list[int], list[int]]:
    """Labels and sizes by plain loops: from every unvisited running id in ascending order, a stack walk over the
    running ids it holds or that hold it."""
    n = len(running)
    label, size = [NONE] * n, [0] * n
    for s in range(n):
        if not running[s] or label[s] != NONE:
            continue
        stack, seen = [s], [s]
        label[s] = s
        while stack:
            i = stack.pop()
            for j in range(n):
                if running[j] and label[j] == NONE and (member[i][j] or member[j][i]):
                    label[j] = s
                    stack.append(j)
                    seen.append(j)
        for i in seen:
            size[i] = len(seen)
    return label, size


@pytest.mark.parametrize("seed", range(6))
def test_islands_ref_against_a_flood_fill(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 90))
    p = [0.3, 1.0, 1.5, 2.5, 0.7, 1.2][seed] / n               # around the threshold: many components of mixed sizes
    m = (rng.random((n, n + 3)) < p).astype(np.uint8)
    run = rng.random(n) < 0.85
    r = islands_ref(m, run)
    label, size = flood_fill(m.tolist(), run.tolist())
    assert r.label.tolist() == label and r.size.tolist() == size
    sizes = sorted((size[h] for h in set(label) - {NONE}), reverse=True)
    s = r.summary
    assert s["islands"] == len(sizes) and s["observers"] == int(run.sum()) == sum(sizes)
    assert s["largest"] == sizes[0] and s["second"] == (sizes[1] if len(sizes) > 1 else 0)
    assert [e[1] for e in s["top"]] == (sizes + [0] * 8)[:8]
    assert s["unreachable_pairs"] == sum(a * (sum(sizes) - a) for a in sizes)
    assert s["singletons"] == sizes.count(1) >= s["rebroadcasting"]


def test_host_summary_under_sanitizers(tmp_path):
    """The host half of the census (sizes and summary, kaboodle_amd/csrc/kb_islands_sum.h: no HIP in it) as a
    stand-alone program on hand-made labels, built with AddressSanitizer and UBSan."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "islands_summary")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "islands_summary_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "islands summary ok" in out.stdout, out.stdout + out.stderr


# a partition long enough for each side to drop the other wholesale (sim_sender honours Failed): two sealed camps
SPLIT = ({"cfg": _ffi.SimConfig(capacity=32, initial_nodes=32, init_mode=_ffi.KB_INIT_CONVERGED, loss=0.02,
                                partition_groups=2, partition_start=2, partition_end=40, seed=4)}, 48)
ORACLE_CASES = {"config1_2x2": STD["config1_2x2"], "stop_start": STD["stop_start"], "partition_heal": STD["partition_heal"],
                "partition": (scenarios.BY_NAME["partition"], scenarios.BY_NAME["partition"]["rounds"]), "split32": SPLIT}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_identities_on_the_oracle_every_round(name):
    case, rounds = ORACLE_CASES[name]
    multi = 0
    with Sim(parity.oracle_lib(), case["cfg"]) as o:
        assert "sim_islands" not in o.lib.fn                 # islands_ref answers through the same call
        parity.setup(o, case)
        for r in range(rounds):
            parity.apply_events((o,), case, r)
            o.step(1)
            got = o.islands()
            s, label, size = got.summary, got.label, got.size
            run = o.scalars()[:, 0] != 0
            heads = np.flatnonzero(label == np.arange(o.capacity))
            assert s["round"] == r + 1 and s["observers"] == int(run.sum()) == int(size[heads].sum())
            assert ((label != NONE) == run).all() and ((size > 0) == run).all()
            assert (label[run] <= np.flatnonzero(run)).all()
            assert (label[label[run]] == label[run]).all()
            missing = o.census().missing
            for i in np.flatnonzero(run):
                mine = [j for j in o.peers(int(i)) if run[j]]
                assert (label[mine] == label[i]).all(), f"round {r}: row {i} holds a peer of another island"
                assert missing[i] >= s["observers"] - size[i]
            assert o.islands(arrays=False).summary == s
            multi += s["second"] >= 2
    if name == "split32":
        assert multi > 0 and s["islands"] == 2 and s["top"][:2] == [[0, 16], [16, 16]]  # the two halves, sealed: the heal never comes
    if name == "config1_2x2":
        assert s["islands"] == 1 and s["largest"] == 4
