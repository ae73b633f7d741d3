"""Wave 0 with its BIG KnownPeers groups on the side stream: in a round with joiners the groups of at
least KP_BIG ids run beside the in-order handlers of every other node, and the joiners' own in-order inboxes are
handled by a deferred k_proc pass after the join.  Every case compares the complete state with the oracle after every
round; KB_DBG_WAVE0_SERIAL keeps the one-launch path, for the byte-for-byte comparison of the two GPU paths."""
import numpy as np
import pytest

import parity
from kaboodle_amd._ffi import KB_DBG_WAVE0_SERIAL, KB_INIT_CONVERGED, Sim, SimConfig
from test_gpu_fold import BIG_8197, RowRef, check_round

pytestmark = pytest.mark.gpu

PATH_PROC_DEFERRED = 512                      # kb_common.h: the deferred pass handled a BIG destination's inbox
BY_NAME = {n: (c, r) for n, c, r in parity.standard_cases()}


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def launches(sim):
    bd = sim.kernel_breakdown()
    return {k: bd[k]["launches"] for k in ("k_scatter", "k_kp", "k_sortfast", "k_proc")}


def test_big_groups_against_oracle_and_serial(gpu):
    """config2_join_1k: all 1024 peers join in round 0, so every joiner's group is BIG.  The split path against the
    oracle, and against the serial path of the same library byte for byte; the split path adds one k_kp and one k_proc
    launch in every round with joiners, the serial path none."""
    case, rounds = BY_NAME["config2_join_1k"][0], 6
    with Sim(gpu, case["cfg"]) as g, Sim(gpu, parity.with_cfg(case, debug_flags=KB_DBG_WAVE0_SERIAL)["cfg"]) as s:
        parity.setup(s, case)                    # (run_case sets g up)
        for x in (g, s):
            x.set_profiling(2)
            x.reset_kernel_time()

        def both(r, o, gg):
            s.step(1)
            d = parity.diff_states(parity.state_of(gg), parity.state_of(s))
            assert not d, f"round {r}: split != serial: {d[:6]}"

        ok, msg, _ = parity.run_case(case, rounds, gpu=g, on_round=both)
        assert ok, msg
        lg, ls = launches(g), launches(s)
        assert ls["k_kp"] == ls["k_scatter"] == ls["k_proc"], ls
        extra = lg["k_kp"] - lg["k_scatter"]
        assert 1 <= extra <= rounds and lg["k_proc"] - lg["k_scatter"] == extra and lg["k_scatter"] == ls["k_scatter"], (lg, ls)
        assert g.debug_paths() & PATH_PROC_DEFERRED and not s.debug_paths() & PATH_PROC_DEFERRED


N2, JOINERS, JOIN_ROUND = 2048, 8, 1
PINGERS = 3


def joiner_case(pings: bool):
    """A converged loss-free mesh of 2048; 8 fresh peers start in JOIN_ROUND (their Join broadcasts are answered in
    the next round's wave 0), and in that next round three members each ping every joiner (wave 0 as well)."""
    ev = {JOIN_ROUND: [("start", N2 + k, None) for k in range(JOINERS)]}
    if pings:
        ev[JOIN_ROUND + 1] = [("ping", 100 * k + 7 * q + 1, [N2 + k]) for k in range(JOINERS) for q in range(PINGERS)]
    return {"cfg": SimConfig(capacity=N2 + 64, initial_nodes=N2, init_mode=KB_INIT_CONVERGED, seed=41), "events": ev}


def test_joiner_that_is_also_an_in_order_destination(gpu):
    """The deferred k_proc pass: joiners whose BIG group and Pings arrive in the same wave 0.  The oracle alone shows
    it (condition): in round JOIN_ROUND + 1 every joiner's view grows from itself to most of the mesh (its Join
    responses, >= KP_BIG ids) and, against the same run without the scripted pings, exactly JOINERS x PINGERS more
    Pings are sent and as many more Acks (loss-free: each was received and answered by its joiner in that round)."""
    case, rounds = joiner_case(True), JOIN_ROUND + 4
    base = joiner_case(False)
    with Sim(parity.oracle_lib(True), base["cfg"]) as b:
        parity.setup(b, base)
        for r in range(JOIN_ROUND + 2):
            parity.apply_events((b,), base, r)
            b.step(1)
        base_stats = b.stats()
    seen = {}

    def on_round(r, o, g):
        if r == JOIN_ROUND:
            seen["before"] = [len(o.peers(N2 + k)) for k in range(JOINERS)]
        if r == JOIN_ROUND + 1:
            seen["after"] = [len(o.peers(N2 + k)) for k in range(JOINERS)]
            seen["stats"] = o.stats()
            seen["paths"] = g.debug_paths()

    ok, msg, _ = parity.run_case(case, rounds, omp=True, on_round=on_round)
    assert max(seen["before"]) <= 1 and min(seen["after"]) >= 1024, seen
    assert seen["stats"]["sent_ping"] - base_stats["sent_ping"] == JOINERS * PINGERS, (seen["stats"], base_stats)
    assert seen["stats"]["sent_ack"] - base_stats["sent_ack"] == JOINERS * PINGERS, (seen["stats"], base_stats)
    assert seen["paths"] & PATH_PROC_DEFERRED, "no deferred node had an in-order inbox"
    assert ok, msg


def test_no_joiners_keeps_the_fused_launch(gpu):
    """The 8000-peer converged mesh without churn: no round has a Join broadcast, so every wave keeps the one k_kp
    launch and the one k_proc launch, and parity holds (sampled rows: the oracle comparison of tests/parity.py)."""
    case = parity.with_cfg(BIG_8197[0], churn=0.0)
    with Sim(gpu, case["cfg"]) as g:
        g.set_profiling(2)
        g.reset_kernel_time()
        ok, msg, st = parity.run_case(case, 4, full_rows=False, omp=True, gpu=g)
        assert ok, msg
        assert st["bcast_join"] == 0
        n = launches(g)
        assert n["k_kp"] == n["k_scatter"] == n["k_sortfast"] == n["k_proc"] > 0, n
        assert not g.debug_paths() & PATH_PROC_DEFERRED
        with Sim(parity.oracle_lib(True), case["cfg"]) as o:
            o.step(4)
            d = parity.compare_sampled(o, g, np.random.default_rng(5), 16)
            assert not d, d


def test_checkpoint_invariant_on_the_split_path(gpu):
    """tests/test_gpu_fold.py's invariant on config2_join_1k with the split path: the BIG groups refold checkpoints
    from their LDS slice on the side stream, and the deferred handlers run wave_fp on the same rows after the join."""
    case, rounds = BY_NAME["config2_join_1k"]
    counts = {"rows": 0, "marked": 0, "dirty": 0}
    with Sim(gpu, case["cfg"]) as g:
        parity.setup(g, case)
        ref = RowRef(g)
        for r in range(rounds):
            parity.apply_events((g,), case, r)
            g.step(1)
            check_round(g, ref, f"split config2_join_1k round {r}", counts)
        assert counts["rows"] > 0 and g.debug_paths() & PATH_PROC_DEFERRED


def test_churn_and_loss(gpu):
    """churn_loss_512 for 30 rounds: joins arrive in most rounds, with mixed inbox sizes."""
    case = BY_NAME["churn_loss_512"][0]
    ok, msg, st = parity.run_case(case, 30)
    assert ok, msg
    assert st["bcast_join"] > 0
