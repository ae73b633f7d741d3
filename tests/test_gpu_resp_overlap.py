"""The Join responses split around A2: k_tick_scan runs first and flags the nodes A2 may touch; the
flagged responders are served on the main stream ahead of k_tick_pre (phase 1), every other responder on a third
stream beside A2, the fold and the exact A3 order (phase 2), joined ahead of k_tick_post.  Every case compares the
complete state with the oracle after every round; KB_DBG_RESP_SERIAL keeps all responses ahead of the tick in one
phase, for the byte-for-byte comparison of the two GPU schedules."""
import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import (KB_DBG_RESP_HBM, KB_DBG_RESP_SERIAL, KB_DBG_WAVE_GRAPH, KB_INIT_CONVERGED, Sim,
                               SimConfig)
from test_gpu_fold import BIG_8197, RowRef, check_round

pytestmark = pytest.mark.gpu

PATH_RESP_PHASE1 = 16384                      # kb_common.h: phase 1 served a responder that A2 may touch
PATH_A2_RESPONDER = 32768                     # kb_common.h: A2 removed a member from a responder's row
BY_NAME = {n: (c, r) for n, c, r in parity.standard_cases()}
RESP = ("k_resp_wave", "k_resp_node")


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def launches(sim):
    bd = sim.kernel_breakdown()                  # (a kernel that never ran has no entry)
    return {k: bd[k]["launches"] if k in bd else 0 for k in RESP}


def against_oracle_and_serial(gpu, case, rounds, flags=0, on_round=None, profile=False):
    """`case` with the split schedule against the oracle every round, and byte for byte against a twin of the same
    library with KB_DBG_RESP_SERIAL.  Returns (final stats, paths of the split run, paths of the serial run, per-round
    launch counts of both when profiled)."""
    per_round = []
    with Sim(gpu, parity.with_cfg(case, debug_flags=flags)["cfg"]) as g, \
            Sim(gpu, parity.with_cfg(case, debug_flags=flags | KB_DBG_RESP_SERIAL)["cfg"]) as s:
        parity.setup(s, case)                    # (run_case sets g up)
        if profile:
            for x in (g, s):
                x.set_profiling(2)
                x.reset_kernel_time()

        def both(r, o, gg):
            parity.apply_events((s,), case, r)
            s.step(1)
            d = parity.diff_states(parity.state_of(gg), parity.state_of(s))
            assert not d, f"round {r}: split != serial: {d[:6]}"
            if profile:
                per_round.append((launches(gg), launches(s)))
            if on_round is not None:
                on_round(r, o, gg)

        ok, msg, st = parity.run_case(parity.with_cfg(case, debug_flags=flags), rounds, gpu=g, on_round=both)
        assert ok, msg
        return st, g.debug_paths(), s.debug_paths(), per_round


def test_churn_and_loss(gpu):
    """churn_loss_512 for 30 rounds: Joins arrive in most rounds and suspects time out beside them, so both phases
    serve responders.  The serial twin never runs phase 1."""
    st, pg, ps, _ = against_oracle_and_serial(gpu, BY_NAME["churn_loss_512"][0], 30)
    assert st["bcast_join"] > 0
    assert pg & PATH_RESP_PHASE1 and not ps & PATH_RESP_PHASE1, (pg, ps)


N2, STOPS, STOP_ROUND = 2048, 256, 1
JOIN_ROUNDS = range(2, 13)                    # PING_TIMEOUT + the indirect-ping timeout + 2 rounds, and a margin


def conflict_case():
    """A converged loss-free mesh of 2048.  STOPS members stop in round 1: their pingers suspect them, ask for indirect
    pings PING_TIMEOUT rounds later and remove them after as many again (A2): some 250 rows in round 5, fewer in each
    round after it.  One fresh peer starts in each of rounds 2..12, so each of rounds 3..13 delivers a Join broadcast,
    which a dozen or two of the members answer."""
    ev = {STOP_ROUND: [("stop", 7 * k + 5, None) for k in range(STOPS)]}
    for k, r in enumerate(JOIN_ROUNDS):
        ev[r] = [("start", N2 + k, None)]
    return {"cfg": SimConfig(capacity=N2 + 64, initial_nodes=N2, init_mode=KB_INIT_CONVERGED, seed=41), "events": ev}


def test_a2_changes_a_responders_row(gpu):
    """The conflict itself: a responder whose own row A2 changes in the same round must be served ahead of A2.  The
    oracle alone shows the condition: some round both answers a Join broadcast (join_responses rises) and removes
    timed-out suspects (removed_timeout rises).  On the GPU the row of one of the round's responders lost a member to
    A2 (PATH_A2_RESPONDER) and phase 1 served flagged responders."""
    case, rounds = conflict_case(), JOIN_ROUNDS[-1] + 2
    prev, both_rounds = {"join_responses": 0, "removed_timeout": 0}, []

    def on_round(r, o, g):
        st = o.stats()
        if st["join_responses"] > prev["join_responses"] and st["removed_timeout"] > prev["removed_timeout"]:
            both_rounds.append(r)
        prev.update(st)

    st, pg, ps, _ = against_oracle_and_serial(gpu, case, rounds, on_round=on_round)
    assert both_rounds, "no round with Join responses and A2 removals on the oracle"
    assert st["bcast_join"] > 0 and st["removed_timeout"] > 0
    assert pg & PATH_A2_RESPONDER, "A2 removed no member from a responder's row"
    assert pg & PATH_RESP_PHASE1 and not ps & PATH_RESP_PHASE1, (pg, ps)


def test_no_responders(gpu):
    """The 8000-peer converged mesh without churn: no Join broadcast, so no round launches a response kernel in either
    phase, and parity holds (sampled rows: the oracle comparison of tests/parity.py)."""
    case = parity.with_cfg(BIG_8197[0], churn=0.0)
    with Sim(gpu, case["cfg"]) as g:
        g.set_profiling(2)
        g.reset_kernel_time()
        ok, msg, st = parity.run_case(case, 4, full_rows=False, omp=True, gpu=g)
        assert ok, msg
        assert st["bcast_join"] == 0
        assert launches(g) == {"k_resp_wave": 0, "k_resp_node": 0}
        assert not g.debug_paths() & PATH_RESP_PHASE1
        with Sim(parity.oracle_lib(True), case["cfg"]) as o:
            o.step(4)
            d = parity.compare_sampled(o, g, np.random.default_rng(5), 16)
            assert not d, d


def test_forced_hbm_rows_stay_serial(gpu):
    """config2_join_1k with KB_DBG_RESP_HBM: the workgroup path's HBM scratch is sized for one launch, so the responses
    keep the serial order: the same response launches every round as the twin with KB_DBG_RESP_SERIAL, no phase 1."""
    _, pg, _, per_round = against_oracle_and_serial(gpu, BY_NAME["config2_join_1k"][0], 6, flags=KB_DBG_RESP_HBM,
                                                    profile=True)
    assert all(a == b for a, b in per_round), per_round
    assert per_round[-1][0]["k_resp_node"] > 0 and not pg & PATH_RESP_PHASE1


def test_window_graph(gpu):
    """config2_join_1k with the receive window as a replayed graph: the third stream joins ahead of the window, so the
    capture is unaffected and the split may stay on; parity decides."""
    against_oracle_and_serial(gpu, BY_NAME["config2_join_1k"][0], 6, flags=KB_DBG_WAVE_GRAPH)


def test_checkpoint_invariant_with_the_split(gpu):
    """tests/test_gpu_fold.py's invariant on churn_loss_512 with the split on: the fold runs beside phase 2, which
    reads rows the fold's checkpoints describe and writes none."""
    case = BY_NAME["churn_loss_512"][0]
    counts = {"rows": 0, "marked": 0, "dirty": 0}
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        g.set_profiling(2)
        g.reset_kernel_time()
        ref = RowRef(g)
        split_rounds = 0
        for r in range(10):
            parity.apply_events((g,), case, r)
            before = launches(g)
            g.step(1)
            after = launches(g)
            split_rounds += all(after[k] - before[k] == 2 for k in RESP)   # a split round: both phases launch both kernels
            check_round(g, ref, f"split churn_loss_512 round {r}", counts)
        assert counts["rows"] > 0 and split_rounds > 0
