"""Mass-join scenarios: joiner lists past the dense engine's LDS caps, and a freshness log ring that wraps.

Plain data like tests/scenarios.py: each scenario is a SimConfig plus per-round API events in the form
parity.run_case takes, and the rounds to run.  The limits they cross (kaboodle_amd/csrc/):

  PB_JMAX = 1024 Joins / PB_FMAX = 2048 Faileds in a round   row pass with the lists read from HBM
  RESP_JCAP = 1024 new joiners at one receiver               k_resp_node reads joiner ids from HBM
  RW_JCAP = 128 new joiners at one receiver                  k_resp_wave hands the responder to k_resp_node
  LOGCAP = 2048 log entries in a 10-round freshness window   the KPR oversize proof on a wrapped ring
  UCAP = 1024 joiners in a round, row-sharded                Join responses as lists beside the unions

tests/test_massjoin.py keeps every scenario on its path (on the CPU oracle); tests/test_gpu_massjoin.py
compares the HIP library with the oracle on them.
"""
from __future__ import annotations

from kaboodle_amd._ffi import KB_INIT_CONVERGED, SimConfig

# coverage bits of kb_sim_debug_paths (PATH_* in kaboodle_amd/csrc/kb_common.h)
PATH_RESP_WAVE = 64
PATH_ROWPASS_LDS_HBM_LISTS = 1024
PATH_KPR_WRAPPED = 2048
PATH_RESP_JOINERS_HBM = 4096
PATH_JOIN_LIST_PAST_UCAP = 8192


def _sc(name, cfg, rounds, events=None):
    return {"name": name, "cfg": cfg, "rounds": rounds, "events": events or {}}


def _mesh700(seed=7):
    return SimConfig(capacity=1856, initial_nodes=700, init_mode=KB_INIT_CONVERGED, loss=0.02, seed=seed)


def _wave(n, at):
    return {at: [("start", i, None) for i in range(700, 700 + n)]}


SCENARIOS = [
    # every peer joins at once: 2200 Joins in round 0's list (> PB_JMAX, > UCAP), every receiver sees 2199 new
    # joiners in round 1 (> RESP_JCAP) and logs them all (> LOGCAP) until round 1 leaves the window after round 10
    _sc("mass_join_2200", SimConfig(capacity=2304, initial_nodes=2200, loss=0.03, seed=19), 14),
    # 20 peers of a converged mesh stop, then 1100 fresh ids start together: round 6's row pass sees 1100 Joins
    # beside a Failed list (rows staged in LDS, lists read from HBM), 680 receivers with 1100 new joiners each
    _sc("wave_join_1100", _mesh700(), 12,
        {1: [("stop", i, None) for i in range(0, 40, 2)], **_wave(1100, 5)}),
    # one past PB_JMAX and UCAP; rows of 1025 ids (no multiple of 32)
    _sc("join_1025", SimConfig(capacity=1025, initial_nodes=1025, loss=0.02), 6),
    # every node logs 2048 / 2049 entries in round 1: the window exactly full / one over
    _sc("join_2049", SimConfig(capacity=2049, initial_nodes=2049, loss=0.03), 13),
    _sc("join_2050", SimConfig(capacity=2050, initial_nodes=2050, loss=0.03), 13),
    # the two sides of RW_JCAP, from views (700) above the KnownPeers cap: sampled responses, by wave / by node
    _sc("wave_128", _mesh700(), 8, _wave(128, 3)),
    _sc("wave_129", _mesh700(), 8, _wave(129, 3)),
]

BY_NAME = {s["name"]: s for s in SCENARIOS}
