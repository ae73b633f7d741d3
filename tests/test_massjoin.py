"""The mass-join scenarios (tests/massjoin.py) stay on their paths, checked on the CPU oracle alone.

Each scenario exists to push one list length past a limit of the dense HIP engine (PB_JMAX, RESP_JCAP,
RW_JCAP, LOGCAP, UCAP).  The lengths are read here from the oracle's per-round broadcast lists and counter
deltas, so an edit to a seed or a size that moves a scenario off its path fails without a GPU.  The bounds are
inequalities (the measured counts are in the comments); the OpenMP oracle runs each scenario in about a second."""
import time

import pytest

import massjoin
import parity
from kaboodle_amd._ffi import Sim

KEYS = ("join_responses", "sent_kpr", "sent_known_peers", "drop_oversize")


def _trace(name):
    """Per round: the counters' deltas and the broadcast list the next round delivers, plus the wall time."""
    sc = massjoin.BY_NAME[name]
    out = []
    t0 = time.perf_counter()
    with Sim(parity.oracle_lib(omp=True), sc["cfg"]) as o:
        parity.setup(o, sc)
        prev = o.stats()
        for r in range(sc["rounds"]):
            parity.apply_events((o,), sc, r)
            o.step(1)
            st = o.stats()
            b = o.broadcasts()
            out.append({**{k: st[k] - prev[k] for k in KEYS}, "joins": sum(k == "Join" for k, _, _ in b),
                        "faileds": sum(k == "Failed" for k, _, _ in b)})
            prev = st
    return out, time.perf_counter() - t0


@pytest.fixture(scope="module")
def traces():
    return {s["name"]: _trace(s["name"]) for s in massjoin.SCENARIOS}


@pytest.mark.parametrize("name", [s["name"] for s in massjoin.SCENARIOS])
def test_oracle_run_is_quick(traces, name):
    """Seconds on the OpenMP oracle (measured: 1.0 s for mass_join_2200, 0.2 s for wave_join_1100)."""
    assert traces[name][1] < 20.0, traces[name][1]


def test_mass_join_2200_path(traces):
    t, _ = traces["mass_join_2200"]
    assert t[0]["joins"] == 2200                      # > PB_JMAX and > UCAP in round 1's broadcast phase
    # round 1: every receiver answers (2199 new joiners each, > RESP_JCAP), KPRs are sent and their replies
    # are oversize (measured 62,428 / 1,623 / 1,490)
    assert t[1]["join_responses"] > 0 and t[1]["sent_kpr"] > 0 and t[1]["drop_oversize"] > 0, t[1]
    # while round 1's 2199 log entries per node are inside the 10-round window (> LOGCAP once anything
    # follows them) KPR replies stay oversize; once they left it the replies fit again
    for r in range(1, 11):
        assert t[r]["drop_oversize"] > 0, (r, t[r])
    for r in range(11, 14):
        assert t[r]["drop_oversize"] == 0 and t[r]["sent_known_peers"] > 0, (r, t[r])


def test_wave_join_1100_path(traces):
    t, _ = traces["wave_join_1100"]
    # round 6's row pass: 1100 Joins (> PB_JMAX) beside a Failed list (measured 27 Faileds)
    assert t[5]["joins"] == 1100 and t[5]["faileds"] >= 1, t[5]
    assert t[6]["join_responses"] > 0, t[6]           # measured 26,998; 1100 new joiners per receiver > RESP_JCAP


@pytest.mark.parametrize("name,n", [("wave_128", 128), ("wave_129", 129)])
def test_wave_sides_of_rw_jcap(traces, name, n):
    t, _ = traces[name]
    assert t[3]["joins"] == n and t[4]["join_responses"] > 0, (t[3], t[4])
    assert massjoin.BY_NAME[name]["cfg"].initial_nodes > 567      # n - nnew above the KnownPeers cap: sampled


@pytest.mark.parametrize("name,n", [("join_1025", 1025), ("join_2049", 2049), ("join_2050", 2050)])
def test_join_sizes(traces, name, n):
    t, _ = traces[name]
    assert t[0]["joins"] == n and t[1]["join_responses"] > 0, (t[0], t[1])
