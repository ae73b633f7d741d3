"""The contact-age census in numpy: the per-(node, peer) stamp read mesh-wide (include/kaboodle_age.h).

`Sim.age_census()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_age_census, which passes over sparse rows'
entry lists on the device (dense handles refuse).  `age_census_ref` computes the same result from `peer_states_array(i)` of the running ids and
`scalars()` alone, so it works on the CPU oracle and on any handle; it is what `Sim.age_census()` falls back to for
a library without kb_sim_age_census (the oracle), so the oracle and the GPU answer the same call.
`age_census_of_arrays` is the same census of a crafted stamp table, member matrix and running flags.  Pure numpy:
nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

KB_AGE_HIST = 256
INT32_MIN = -(2 ** 31)
SHARE_AGE = 10                    # src/kaboodle.rs:49: a KnownPeersRequest reply lists entries stamped within it
EPOCH, EOFF = 64, 192             # the stamp byte's window: since = byte + epoch_base(r) - EOFF
ST_SUSPECT, ST_ANCIENT = 1, 2
KB_STATE_KNOWN = 0
SUMMARY_FIELDS = ("round", "observers", "cells", "suspects", "ancient", "windowed", "fresh", "dead_suspects",
                  "dead_ancient", "dead_windowed", "dead_fresh", "unheard_ids", "oldest_heard_id", "oldest_heard", "hist")
ID_ARRAYS = ("suspected_by", "ancient_by", "windowed_by", "fresh_by", "last_heard")
ROW_ARRAYS = ("suspects", "ancient", "windowed", "fresh")
ARRAYS = ID_ARRAYS + ROW_ARRAYS


@dataclass
class AgeCensus:
    """One contact-age census: `summary` (the fields of kb_age_census; hist a list of 256) and, over all ids, the
    uint32 arrays `suspected_by`, `ancient_by`, `windowed_by`, `fresh_by` and the int32 `last_heard` per peer, and
    `suspects`, `ancient`, `windowed`, `fresh` (uint32) per row; the nine arrays are None with arrays=False."""
    summary: dict
    suspected_by: np.ndarray | None = None
    ancient_by: np.ndarray | None = None
    windowed_by: np.ndarray | None = None
    fresh_by: np.ndarray | None = None
    last_heard: np.ndarray | None = None
    suspects: np.ndarray | None = None
    ancient: np.ndarray | None = None
    windowed: np.ndarray | None = None
    fresh: np.ndarray | None = None

    def same_as(self, other: "AgeCensus") -> list[str]:
        """The differences to another contact-age census (empty: identical summary and arrays)."""
        return diff_results(self, other, ARRAYS)


def last_round(round_: int) -> int:
    """r: the last simulated round of a state whose kb_stats.round is `round_` (0 before the first round)."""
    return round_ - 1 if round_ > 0 else 0


def since_of_byte(byte: int, round_: int) -> int:
    """The instant a windowed stamp byte (>= 3) stands for, decoded with the last simulated round's epoch."""
    r = last_round(round_)
    return int(byte) + (r // EPOCH) * EPOCH - EOFF


def _finish(n_ids, n_rows, observers, round_, running_ids, dead_ids, rows, peers, cls, since, arrays) -> AgeCensus:
    """The census of the counting cells (rows[k], peers[k]) of class cls[k] (0 suspect, 1 ancient, 2 windowed) and
    instant since[k] (windowed cells).  running_ids / dead_ids: bool per id."""
    r = last_round(round_)
    rows, peers, cls = (np.asarray(x, dtype=np.int64) for x in (rows, peers, cls))
    since = np.asarray(since, dtype=np.int64)
    win = cls == 2
    age = r - since[win]
    if len(age) and (age.min() < 0 or age.max() >= KB_AGE_HIST):
        raise ValueError("a windowed cell's age is outside [0, 255]")
    fresh = np.zeros(len(cls), dtype=bool)
    fresh[win] = age < SHARE_AGE
    cnt = lambda sel, idx, n: np.bincount(idx[sel], minlength=n).astype(np.uint32)
    by = [cnt(cls == 0, peers, n_ids), cnt(cls == 1, peers, n_ids), cnt(win, peers, n_ids), cnt(fresh, peers, n_ids)]
    lh = np.full(n_ids, INT32_MIN, dtype=np.int64)
    np.maximum.at(lh, peers[win], since[win])
    lh = lh.astype(np.int32)
    tot = lambda a, sel=None: int((a if sel is None else a[sel]).sum(dtype=np.uint64))
    s = {"round": int(round_), "observers": int(observers),
         "cells": int(len(cls)), "suspects": tot(by[0]), "ancient": tot(by[1]), "windowed": tot(by[2]), "fresh": tot(by[3]),
         "dead_suspects": tot(by[0], dead_ids), "dead_ancient": tot(by[1], dead_ids),
         "dead_windowed": tot(by[2], dead_ids), "dead_fresh": tot(by[3], dead_ids),
         "unheard_ids": int((running_ids & (by[2] == 0)).sum())}
    if running_ids.any():
        ids = np.flatnonzero(running_ids)
        k = ids[np.argmin(lh[ids])]                        # argmin: the first (lowest id) of the smallest
        s["oldest_heard_id"], s["oldest_heard"] = int(k), int(lh[k])
    else:
        s["oldest_heard_id"], s["oldest_heard"] = KB_CENSUS_NONE, INT32_MIN
    s["hist"] = [int(x) for x in np.bincount(age, minlength=KB_AGE_HIST)]
    if not arrays:
        return AgeCensus(s)
    rw = [cnt(cls == 0, rows, n_rows), cnt(cls == 1, rows, n_rows), cnt(win, rows, n_rows), cnt(fresh, rows, n_rows)]
    return AgeCensus(s, by[0], by[1], by[2], by[3], lh, *rw)


def age_census_of_arrays(stamp, member, running, round_: int, arrays: bool = True) -> AgeCensus:
    """The census of a whole table: `stamp` [n_rows][n_ids] bytes, `member` [n_rows][n_ids] (non-zero: j is in
    view(i)), `running` [n_rows]; row k is id k.  `round_` is what kb_stats.round would be.  A byte under a clear
    member bit and byte 0 count nowhere, id j runs iff j < n_rows and running[j], no id is external."""
    stamp = np.asarray(stamp, dtype=np.uint8)
    n_rows, n_ids = stamp.shape
    mem = np.asarray(member).reshape(n_rows, n_ids) != 0
    run = np.asarray(running).reshape(n_rows) != 0
    counts = mem & run[:, None] & (stamp != 0)
    k = min(n_rows, n_ids)
    counts[np.arange(k), np.arange(k)] = False             # the self entry
    rows, peers = np.nonzero(counts)
    b = stamp[rows, peers].astype(np.int64)
    cls = np.where(b == ST_SUSPECT, 0, np.where(b == ST_ANCIENT, 1, 2))
    since = b + (last_round(round_) // EPOCH) * EPOCH - EOFF
    run_ids = np.zeros(n_ids, dtype=bool)
    run_ids[:k] = run[:k]
    return _finish(n_ids, n_rows, int(run.sum()), round_, run_ids, ~run_ids, rows, peers, cls, since, arrays)


def age_census_ref(sim, arrays: bool = True, external=None) -> AgeCensus:
    """The contact-age census of `sim` from `sim.peer_states_array(i)` of the running rows it holds and
    `sim.scalars()`: one peer_states call per observer, the test and small-mesh path, and what the CPU oracle answers
    with.  `external`: the ids marked by set_external (default: the ones the handle recorded).  On the GPU use
    Sim.age_census()."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    ext = np.zeros(C, dtype=bool)
    ext[list(sim.external if external is None else external)] = True
    _, _, lo, hi = sim.shard_info()
    held = np.zeros(C, dtype=bool)
    held[lo:hi] = True
    rows, peers, cls, since = [], [], [], []
    obs = np.flatnonzero(running & held)
    for i in obs.tolist():
        ps = sim.peer_states_array(i)
        ps = ps[ps["peer"] != i]
        known = ps["state"] == KB_STATE_KNOWN
        anc = known & (ps["since"] == INT32_MIN)
        peers.append(ps["peer"].astype(np.int64))
        rows.append(np.full(len(ps), i, dtype=np.int64))
        cls.append(np.where(~known, 0, np.where(anc, 1, 2)))
        since.append(ps["since"].astype(np.int64))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)
    return _finish(C, C, len(obs), sim.stats()["round"], running, ~running & ~ext, cat(rows), cat(peers), cat(cls),
                   cat(since), arrays)
