"""The round's shared host steps (csrc/kb_roundframe.h) while their buffers grow more than once in a handle's life:
the event list, the Probe responses, the injected records with their payload ids and the export buffers, through
all four kinds of handle, against the C oracle given the same calls.

Case: converged_loss_256 with 4 spare addresses, two of them external (as test_gpu_external_peers builds it), 10
rounds.  Round 2 queues 1 Probe and 2 stops, round 4 3 Probes and 12 lifecycle events, round 7 9 Probes and 40
(stops, and restarts of earlier stops: the two spare addresses that are not external are the fresh ids there are);
the scripted replies of parity.external_replies are injected every round.  Rounds count from one (round k is the k-th
kb_sim_step): counted from zero, the single Probe of round 2 draws no response under this case's seed, and the
check of the Probe drain would be vacuous there."""
from dataclasses import replace

import pytest

import parity
from kaboodle_amd._ffi import Sim

ROUNDS = 10
PROBED = {2: 1, 4: 3, 7: 9}                      # round (from one) -> Probes queued before it
KINDS = {"dense": (0, 0), "dense_x3": (0, 3), "sparse": (4, 0), "sparse_x3": (4, 3)}   # kind -> (variant, shards)


def schedule() -> dict:
    """The API calls ahead of each round, keyed as parity.apply_events takes them (the step's index, from zero)."""
    ev = {2: [("stop", 5, None), ("stop", 17, None)],
          4: [("restart", 5, None)] + [("stop", n, None) for n in range(20, 31)],
          7: [("restart", 17, None)] + [("stop", n, None) for n in range(40, 79)]}
    assert [len(ev[r]) for r in (2, 4, 7)] == [2, 12, 40]
    for r, n in PROBED.items():
        ev[r] = ev[r] + [("probe", None, (f"192.168.{r}.{k + 1}", 4000 + k)) for k in range(n)]
    return {r - 1: calls for r, calls in ev.items()}


def the_case(variant: int) -> tuple[dict, list[int]]:
    case, _ = {n: (c, r) for n, c, r in parity.standard_cases()}["converged_loss_256"]
    c = case["cfg"]
    cfg = replace(c, capacity=c.capacity + 4, variant=variant)
    return {**case, "cfg": cfg, "events": schedule()}, [c.capacity + 1, c.capacity + 3]


def drive(sim: Sim, case: dict, externals, injections=None, count_waits=False):
    """The schedule on one implementation: yields (round, host waits of the round, complete state, exported records,
    the replies injected for the next round).  injections = the recorded replies of another run to replay (they
    depend only on the exports, which must be identical); None: scripted from this run's own exports."""
    cfg = case["cfg"]
    parity.setup(sim, case)
    for x in externals:
        sim.set_external(x)
    known: dict = {}
    targets = {x: [(x * 7 + k * 13) % cfg.initial_nodes for k in range(5)] for x in externals}
    for r in range(ROUNDS):
        parity.apply_events((sim,), case, r)
        n0 = sim.host_syncs() if count_waits else 0
        sim.step(1)
        waits = sim.host_syncs() - n0 if count_waits else 0
        ex = sim.exported()
        st = parity.state_of(sim)
        inj = parity.external_replies(ex, known, r, targets) if injections is None else injections[r]
        for m in inj:
            sim.inject(*m[:6], ids=m[6])
        yield r, waits, st, ex, inj


_TRACE: dict = {}


def oracle_trace(variant: int) -> list:
    """The oracle's run of the schedule, computed once per variant and shared by the tests (never modified)."""
    if variant not in _TRACE:
        case, externals = the_case(variant)
        with Sim(parity.oracle_lib(), case["cfg"]) as o:
            _TRACE[variant] = [(st, ex, inj) for _, _, st, ex, inj in drive(o, case, externals)]
    return _TRACE[variant]


@pytest.mark.parametrize("variant", [0, 4], ids=["dense", "sparse"])
def test_schedule_is_not_vacuous(variant):
    """On the oracle alone: every probed round returns at least one ProbeResponse, records are exported, and the
    injected records grow over the run (so the dense engine's device buffer behind them grows twice)."""
    tr = oracle_trace(variant)
    for r in PROBED:
        assert len(tr[r - 1][0]["probe"]) >= 1, f"round {r}: no ProbeResponse"
        assert all(p[0] == r - 1 for p in tr[r - 1][0]["probe"])
    assert all(not tr[k][0]["probe"] for k in range(ROUNDS) if k + 1 not in PROBED)
    assert sum(len(ex) for _, ex, _ in tr) >= 1
    ninj = [sum(1 for m in inj if m[2] != parity.K_JOIN) for _, _, inj in tr]
    # the dense engine's buffer starts at twice the first count: a later round outgrows that too (a second growth)
    assert ninj[0] > 0 and max(ninj) > 2 * ninj[0], ninj


def wait_bound(kind: str, cfg, events) -> int:
    """Host waits of one kb_sim_step(1), as test_host_waits_per_round states them for the dense engine: unsharded two
    pinned hand-offs, row-sharded one hand-off for the broadcast lists plus one per delivery wave (and one more wave
    boundary); plus the step's own stream synchronisation.  A round that applies lifecycle events waits once more
    for them, and once per restart for the moved row's header (move_row); the sparse engine reads its scan totals
    back instead (two per round and two per wave, sharded one more each, and up to three per restart)."""
    restarts = sum(1 for e in events if e[0] == "restart")
    lifecycle = sum(1 for e in events if e[0] in ("stop", "start", "restart"))
    variant, shards = KINDS[kind]
    if variant == 0:
        base = 2 + 1 if not shards else 1 + cfg.max_waves + 1 + 1
        return base + ((1 + restarts) if lifecycle else 0)
    sh = 1 if shards else 0
    return 3 + sh + (2 + sh) * cfg.max_waves + ((1 + 3 * restarts) if lifecycle else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_roundframe_growth_against_oracle(kind):
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    variant, shards = KINDS[kind]
    case, externals = the_case(variant)
    tr = oracle_trace(variant)
    with Sim(parity.gpu_lib(), case["cfg"], shards=shards) as g:
        for r, waits, st, ex, _ in drive(g, case, externals, injections=[inj for _, _, inj in tr], count_waits=True):
            ost, oex, _ = tr[r]
            d = parity.diff_states(ost, st)
            assert not d, f"{kind} round {r}: " + "; ".join(d[:6])
            assert ex == oex, f"{kind} round {r}: exports differ: {oex[:3]} vs {ex[:3]}"
            assert st["probe"] == ost["probe"], f"{kind} round {r}: probe responses differ"
            bound = wait_bound(kind, case["cfg"], case["events"].get(r, []))
            print(f"{kind} round {r}: host waits {waits} (bound {bound}), exported {len(ex)}, probe responses {len(st['probe'])}")
            assert waits <= bound, f"{kind} round {r}: {waits} host waits > {bound}"
