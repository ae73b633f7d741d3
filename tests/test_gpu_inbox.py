"""The receive window (csrc/kb_waves.h: k_kp, k_sortfast, k_proc; k_sp_handle on sparse rows) on crafted wave-0
inboxes injected by external peers: the cases of tests/inbox.py (groups A-F), whose conditions
tests/test_inbox.py proves on the oracle alone.  Every comparison is bit-exact: the complete state, the exported
records with their payload ids and stats() after every round against the oracle's recorded run, and the addressed
destinations' fingerprints against kb_fingerprint_of_set of their peers().  Which path ran is read from what the
library already reports: debug_paths(), the bytes k_proc counts for the nodes it handles (kernel_bytes), the dirty flag
and stale mask of checkpoints(), or it follows from the oracle's state before the round (tests/test_inbox.py).

Engines: every case runs on a dense unsharded handle.  One representative per group, the 8193-record inbox and the
column-split KnownPeers group (ENGINE_CASES) also run with KB_DBG_ALL, as 3 in-process row shards, and on sparse rows
(variant 4) unsharded and as 3 shards; sparse rows keep no latency table, so group F runs there without
track_latency (its slot release is still compared through suspects()), its script recorded from the sparse oracle.

What is by construction only: which of the two sorts orders an inbox (64 | 65), and that an answer of group F goes
through the fast lane (three running peers there: k_proc's byte counter cannot single out one node)."""
from dataclasses import replace

import pytest

import inbox
import parity
from inbox import PATH_KP_BIG_HBM, PATH_KP_BIG_LDS, PATH_PROC_DEFERRED, PATH_PROC_UNSORTED
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_DBG_KP_BIG_SMALL, KB_DBG_KP_HBM, KB_DBG_PROC_UNSORTED, KB_DBG_WAVE0_SERIAL,
                               KB_VARIANT_SPARSE_ROWS)
from test_gpu_fold import RowRef, check_round
from test_inbox import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def run(gpu, name, case=None, **kw):
    """run_crafted, and the path bits every run must respect: the selection path (bit 16) is taken by the 8193-record
    inbox and under KB_DBG_PROC_UNSORTED only; the deferred pass (512) never under KB_DBG_WAVE0_SERIAL."""
    case = case or CASES[name]
    hooks = {k: kw.pop(k) for k in ("pre_round", "post_round") if k in kw}
    out = inbox.run_crafted(case, {"lib": gpu, **kw}, **hooks)
    flags = kw.get("debug_flags", 0)
    unsorted_ = bool(out["paths"] & PATH_PROC_UNSORTED)
    if not flags & KB_DBG_PROC_UNSORTED:
        assert unsorted_ == (name == "A8193"), f"{name}: paths {out['paths']:#x}"
    if flags & KB_DBG_WAVE0_SERIAL:
        assert not out["paths"] & PATH_PROC_DEFERRED
    print(f"{case.name} {kw}: paths {out['paths']:#x}, exported {sum(len(e) for e in out['exports'])}, launches "
          f"k_kp {out['launches'].get('k_kp')} k_sortfast {out['launches'].get('k_sortfast')} k_proc {out['launches'].get('k_proc')}")
    return out


# ---- A: in-order inbox length ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "A"])
def test_a_inbox_length(gpu, name):
    """n in-order records to peer 0 in one wave: the exported Acks come back in (sender, seq) order and equal the
    oracle's.  Fast lane or k_proc: k_proc counts algorithmic bytes for every node it handles, and peer 0 is the
    only running peer, so the counter stands still over the round exactly when the fast lane took the inbox: it
    must for n <= FAST_MAX = 8 (every sender a member, the dirty flag read clear before the round), and must move
    for n >= 9 and for the non-member and stale-fingerprint variants of n = 8.  8193 > SORT_MAX takes k_proc's
    selection path (bit 16) with no debug flag, 8192 in a fresh handle does not.  Which sort orders an inbox of
    9..8192 (one wave's registers up to 64, k_sortfast's workgroups above) follows from its length alone and is not
    observable: the sort workgroups are part of every k_sortfast launch.  What is pinned is their result, on the
    *_unsorted cases: there the inbox reaches the sorts out of order (inbox.case_a_unsorted), at 8 (the fast
    lane's network), 9 and 64 (k_proc's register sort), 65, 129 and 257 (k_sortfast, padded to 128, 256, 512).
    With a sort disabled (scratch builds) every *_unsorted case of that sort fails, and so do the plain cases from 64
    records up, whose senders span several scatter waves; the plain cases of 1..63 records arrive sorted already and
    pin the lengths, not the order.  Nothing shows how 8192 and 8193 arrive."""
    case = CASES[name]
    seen = {}

    def pre(r, g):
        if r == 2:
            seen["dirty"] = g.checkpoints(0)[2]

    out = run(gpu, name, pre_round=pre)
    inbox.acks_in_order([m for m in inbox.oracle_trace(case)[1][3] if m[1] == 0], out["exports"][2])
    assert seen["dirty"] == 0, "peer 0's fingerprint was stale before the round: the case is not the one it names"
    n = int(name[1:].split("_")[0])
    fast = n <= inbox.FAST_MAX and not name.endswith(("nonmember", "stale"))
    print(f"{name}: k_proc bytes per round {out['proc_bytes']}")
    assert (out["proc_bytes"][2] == 0) == fast, f"{name}: k_proc counted {out['proc_bytes'][2]} bytes in round 2"
    assert not out["paths"] & (PATH_KP_BIG_LDS | PATH_KP_BIG_HBM)


# ---- B: prologue insertions and the incremental fingerprint ----------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "B"])
def test_b_prologue_insertions(gpu, name):
    """k first-contact senders in one wave; after every round the stored checkpoints satisfy the invariant of
    DESIGN.md §3.4 (test_gpu_fold.check_round) and the fingerprint equals generate_fingerprint of peers().  *_stale:
    before the wave the stale mask of checkpoints() names some segments and not all (the helper's insertion of the
    round before left its segment marked), and the same wave's KnownPeers list marks two more."""
    case = CASES[name]
    counts = {"rows": 0, "marked": 0, "dirty": 0}
    ref = {}

    def pre(r, g):
        if r == 0:
            ref["ref"] = RowRef(g)
        seg, stale, dirty, fp = g.checkpoints(0)
        print(f"{name} before round {r}: stale mask {stale:#x} dirty {dirty}")
        if name.endswith("stale") and r == 2:
            assert stale not in (0, 2**64 - 1), f"{name}: stale mask {stale:#x} before the wave: nothing partly stale"

    def post(r, g):
        check_round(g, ref["ref"], f"{name} round {r}", counts)

    out = run(gpu, name, pre_round=pre, post_round=post)
    r = 2 if name.endswith("stale") else 1
    inbox.acks_in_order(inbox.oracle_trace(case)[r - 1][3], out["exports"][r])
    assert counts["rows"] >= 3 * case.rounds


# ---- C: the curious table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C_fast", "C_slow"])
def test_c_curious_table(gpu, name):
    """The table's 8 x 4 limits, the forwarded Acks and the freed entries (what they must be: tests/test_inbox.py),
    through the fast lane's copy of the handlers (at most 8 records, all members) and through k_proc's (more)."""
    out = run(gpu, name)
    assert out["states"][3]["stats"]["curious_overflow"] == 2 == out["states"][-1]["stats"]["curious_overflow"]
    # peer 0 runs alone: k_proc's byte counter stands still in a round exactly when the fast lane handled its inbox
    print(f"{name}: k_proc bytes per round {out['proc_bytes']}")
    assert all((out["proc_bytes"][r] == 0) == (name == "C_fast") for r in range(2, 7)), out["proc_bytes"]


# ---- D: KnownPeers groups --------------------------------------------------------------------------------------
D_NAMES = [n for n in CASES if n[0] == "D"]
D_BIG = [n for n in D_NAMES if n in ("D_total4096", "D_dups", "D_colsplit", "D_lengths_big") or n.startswith("D_count")]


@pytest.mark.parametrize("name", D_NAMES)
def test_d_groups(gpu, name):
    """A group of >= KP_BIG = 4096 ids takes the BIG body with the row's bitset in LDS (bit 128), on two column
    parts; 4095 ids in a fresh handle do not.  D_lengths_*: lists of 1, 63, 64, 65 ids and, since the oracle
    delivers an injected list of any length (the 10240-byte datagram limit binds only what simulated peers send),
    639, 640, 641, 1281 around the BIG body's 640-id chunk and the whole row, 8192."""
    out = run(gpu, name)
    assert bool(out["paths"] & PATH_KP_BIG_LDS) == (name in D_BIG), f"{name}: paths {out['paths']:#x}"
    assert not out["paths"] & PATH_KP_BIG_HBM


@pytest.mark.parametrize("flag", [KB_DBG_KP_HBM, KB_DBG_KP_BIG_SMALL], ids=["kp_hbm", "kp_big_small"])
@pytest.mark.parametrize("name", [n for n in D_NAMES if n != "D_many_dests"])
def test_d_groups_flagged(gpu, name, flag):
    """KB_DBG_KP_HBM: the BIG body on the bitset in place, one workgroup per group (bit 8, never 128);
    KB_DBG_KP_BIG_SMALL: every group takes the BIG body, the small ones included (bit 128)."""
    out = run(gpu, name, debug_flags=flag)
    if flag == KB_DBG_KP_HBM:
        assert bool(out["paths"] & PATH_KP_BIG_HBM) == (name in D_BIG) and not out["paths"] & PATH_KP_BIG_LDS
    else:
        assert out["paths"] & PATH_KP_BIG_LDS


def test_d_duplicates_are_order_independent(gpu):
    """The duplicate-heavy group twice on the library: state, exports and fingerprints identical (the atomics decide
    which arm inserts an id, and nothing the ABI shows may depend on it)."""
    a, b = run(gpu, "D_dups"), run(gpu, "D_dups")
    assert a["exports"] == b["exports"] and a["paths"] == b["paths"]
    for r, (x, y) in enumerate(zip(a["states"], b["states"])):
        assert not inbox.diff_compact(x, y), r


# ---- E: KnownPeers and in-order records to the same destination ------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "E"])
def test_e_group_and_inorder(gpu, name):
    """A BIG group plus m Pings to peer 0.  With a Join list in the round wave 0 splits and the deferred k_proc pass
    handles peer 0's Pings after the join (bit 512); without one the fused launch stays (bit 512 clear).  Either
    way the run equals the oracle's and the same run under KB_DBG_WAVE0_SERIAL, state for state."""
    a = run(gpu, name)
    s = run(gpu, name, debug_flags=KB_DBG_WAVE0_SERIAL)
    assert bool(a["paths"] & PATH_PROC_DEFERRED) == name.endswith("join"), f"{name}: paths {a['paths']:#x}"
    assert a["paths"] & PATH_KP_BIG_LDS and s["paths"] & PATH_KP_BIG_LDS
    assert a["exports"] == s["exports"]
    for r, (x, y) in enumerate(zip(a["states"], s["states"])):
        assert not inbox.diff_compact(x, y), r
    inbox.acks_in_order(inbox.oracle_trace(CASES[name])[1][3], a["exports"][2])


# ---- F: a prologue that ends a suspicion -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "F"])
def test_f_late_answer_frees_the_slot(gpu, name):
    """The recorded late answers replayed: suspects() (in the state) and peer_states() with their latencies equal
    the oracle's every round; that the oracle freed the slot and measured about 1000 ms is tests/test_inbox.py's."""
    out = run(gpu, name)
    assert bool(out["paths"] & PATH_KP_BIG_LDS) == (name == "F_kp_big")
    lat = {e[3] for st in out["states"] for i in range(3) for e in st["peer_states"][i] if e[3] != 0xFFFFFFFF}
    assert any(1001 <= v <= 1009 for v in lat), lat


# ---- the other engines -----------------------------------------------------------------------------------------
ENGINE_CASES = ["A65_mixed", "A8193", "B65_edges_8192", "C_slow", "D_dups", "D_colsplit", "E9_join", "F_ack_proc", "F_kp_big"]
ENGINES = {"dbg_all": dict(debug_flags=KB_DBG_ALL), "x3": dict(shards=3), "sparse": dict(), "sparse_x3": dict(shards=3)}


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engines(gpu, name, engine):
    """parity.run_external_case's rule on the crafted cases: exports and state identical to the oracle's on every
    engine (row shards: the external's shard injects, the sender's shard exports)."""
    case = CASES[name]
    if engine.startswith("sparse"):      # (path bits and byte counters are the dense kernels': not read on sparse rows)
        cfg = replace(case.cfg, variant=KB_VARIANT_SPARSE_ROWS, sparse_row_cap=case.cfg.capacity, track_latency=0)
        case = replace(inbox.case_f(name[2:]) if name[0] == "F" else case, cfg=cfg, name=name + "_sparse")
        out = inbox.run_crafted(case, {"lib": gpu, "proc_bytes": False, **ENGINES[engine]})
    else:
        out = run(gpu, name, **ENGINES[engine])
    assert sum(len(e) for e in out["exports"]) > 0
