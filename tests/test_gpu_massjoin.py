"""The mass-join paths of the dense engine against the CPU oracle, on an MI355X (tests/massjoin.py).

Every other parity case starts converged or joins at most 1024 peers in a round, so the kernel paths chosen by
longer lists were never run: the row pass with its lists in HBM beside staged rows (> PB_JMAX Joins with a Failed
list), k_resp_node with the joiners in HBM (> RESP_JCAP), the KnownPeersRequest oversize proof on a wrapped log
ring (> LOGCAP), Join responses as lists past the union slots (> UCAP, row shards), and both sides of RW_JCAP.

Bar: bit-exact, the complete state every round (stamp rows, scalars, suspect and curious tables, fingerprints,
counters, broadcast lists) against the OpenMP oracle; peer_states() on a fixed sample of 32 nodes after the last
round (every node every round would cost millions of Python tuples at 2200 peers).  The coverage bits of
kb_sim_debug_paths prove that the path under test did the work."""
from dataclasses import replace

import numpy as np
import pytest

import massjoin
import parity
from kaboodle_amd._ffi import (KB_DBG_ALL, KB_DBG_NO_UNION, KB_DBG_WAVE_GRAPH, KB_VARIANT_EXACT_LRU,
                               KB_VARIANT_SPARSE_ROWS, Sim)
from massjoin import (PATH_JOIN_LIST_PAST_UCAP, PATH_KPR_WRAPPED, PATH_RESP_JOINERS_HBM, PATH_RESP_WAVE,
                      PATH_ROWPASS_LDS_HBM_LISTS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import kaboodle_amd
    kaboodle_amd.require_gpu()
    return parity.gpu_lib()


def run(gpu, name, shards=0, **cfg_kw):
    """The scenario on both implementations; returns (final GPU stats, kb_sim_debug_paths)."""
    sc = massjoin.BY_NAME[name]
    case = {**sc, "cfg": replace(sc["cfg"], **cfg_kw)}
    cfg, rounds = case["cfg"], sc["rounds"]
    sample = np.random.default_rng(5).choice(cfg.capacity, 32, replace=False)
    ps = []

    def last_round(r, o, g):
        if r == rounds - 1:
            ps.extend(parity.diff_peer_states(o, g, sample))

    g = Sim(gpu, cfg, shards=shards)
    try:
        ok, msg, st = parity.run_case(case, rounds, gpu=g, omp=True, on_round=last_round)
        assert ok, f"{name} ({cfg_kw}, shards={shards}): {msg}"
        assert not ps, f"{name} ({cfg_kw}, shards={shards}): {ps}"
        return st, g.debug_paths()
    finally:
        g.close()


# the bits each scenario must report with default flags (wave_129: parity and responses only; whether a
# receiver holds all 129 Joins depends on the loss draws, so no bit is asked of it)
WANT = {"mass_join_2200": PATH_KPR_WRAPPED | PATH_RESP_JOINERS_HBM,
        "wave_join_1100": PATH_ROWPASS_LDS_HBM_LISTS | PATH_RESP_JOINERS_HBM,
        "join_1025": 0, "join_2049": 0, "join_2050": PATH_KPR_WRAPPED,
        "wave_128": PATH_RESP_WAVE, "wave_129": 0}


@pytest.mark.parametrize("name", [s["name"] for s in massjoin.SCENARIOS])
def test_massjoin_parity(gpu, name):
    st, paths = run(gpu, name)
    assert st["join_responses"] > 0
    assert paths & WANT[name] == WANT[name], f"{name}: paths {paths:#x}, want {WANT[name]:#x}"


@pytest.mark.parametrize("name", ["mass_join_2200", "wave_join_1100"])
def test_massjoin_wide_row_paths(gpu, name):
    """KB_DBG_ALL: responses from HBM scratch with more than 1024 new joiners, BIG KnownPeers groups on HBM."""
    st, paths = run(gpu, name, debug_flags=KB_DBG_ALL)
    assert st["join_responses"] > 0 and paths & PATH_RESP_JOINERS_HBM and paths & (2 | 4) and paths & 8, hex(paths)


def test_massjoin_exact_lru(gpu):
    run(gpu, "wave_join_1100", variant=KB_VARIANT_EXACT_LRU)


def test_massjoin_wave_graph(gpu):
    run(gpu, "join_1025", debug_flags=KB_DBG_WAVE_GRAPH)


@pytest.mark.parametrize("name", ["mass_join_2200", "join_1025", "wave_join_1100"])
def test_massjoin_sharded(gpu, name):
    """Three row shards.  More than UCAP joiners in the round: those past slot 1023 get their responses as
    whole lists beside the unions (wave_join_1100's 1100 joiners too, but only the first two are asked for)."""
    _, paths = run(gpu, name, shards=3)
    if name != "wave_join_1100":
        assert paths & PATH_JOIN_LIST_PAST_UCAP, hex(paths)


def test_massjoin_sharded_lists_only(gpu):
    """The same mesh with every Join response shipped whole (KB_DBG_NO_UNION)."""
    _, paths = run(gpu, "mass_join_2200", shards=3, debug_flags=KB_DBG_NO_UNION)
    assert not paths & PATH_JOIN_LIST_PAST_UCAP      # the bit reports lists beside unions only


@pytest.mark.parametrize("name", ["wave_join_1100", "join_1025"])
def test_massjoin_sparse_rows(gpu, name):
    cap = massjoin.BY_NAME[name]["cfg"].capacity
    run(gpu, name, variant=KB_VARIANT_SPARSE_ROWS, track_latency=0, sparse_row_cap=cap)
