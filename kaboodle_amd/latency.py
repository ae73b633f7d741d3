"""The latency census in numpy: the mesh's ping-latency table read mesh-wide (include/kaboodle_latency.h).

`Sim.latency_census()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_latency_census, which streams the
latency table on the device.  `latency_census_ref` computes the same result from `peer_states_array(i)` of the
running ids alone, so it works on the CPU oracle and on any handle; it is what `Sim.latency_census()` falls back to
for a library without kb_sim_latency_census (the oracle), so the oracle and the GPU answer the same call.
`latency_census_of_states` is the same computation on plain (peer, latency) arrays and `latency_census_of_arrays`
on a whole table, member matrix and running flags (orphans included).  Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

KB_LATENCY_NONE = 0xFFFFFFFF
KB_LAT_HIST = 17
LAT_NONE = 0xFFFF                 # None in a u16 latency table
SUMMARY_FIELDS = ("round", "observers", "measured", "sum_ms", "min_ms", "max_ms", "max_peer", "measured_ids", "hist",
                  "orphans")
ARRAYS = ("measured_by", "sum_ms", "min_ms", "max_ms", "measured", "row_sum_ms")


def bucket(v: int) -> int:
    """The histogram bucket of a value: 0 for 0, floor(log2 v) + 1 otherwise (65534 -> 16)."""
    return int(v).bit_length()


@dataclass
class LatencyCensus:
    """One latency census: `summary` (the fields of kb_lat_census; hist a list of 17) and, over all ids, the arrays
    `measured_by`, `min_ms`, `max_ms` (uint32), `sum_ms` (uint64) per peer and `measured` (uint32), `row_sum_ms`
    (uint64) per row; the six arrays are None with arrays=False."""
    summary: dict
    measured_by: np.ndarray | None = None
    sum_ms: np.ndarray | None = None
    min_ms: np.ndarray | None = None
    max_ms: np.ndarray | None = None
    measured: np.ndarray | None = None
    row_sum_ms: np.ndarray | None = None

    def same_as(self, other: "LatencyCensus") -> list[str]:
        """The differences to another latency census (empty: identical summary and arrays)."""
        return diff_results(self, other, ARRAYS)


def _finish(n_ids, n_rows, observers, round_, peers, rows, vals, orphans, arrays) -> LatencyCensus:
    """The census of the counting cells (peers[k], rows[k]) with values vals[k]."""
    peers = np.asarray(peers, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.uint64)
    mb = np.bincount(peers, minlength=n_ids).astype(np.uint32)
    sm = np.zeros(n_ids, dtype=np.uint64)
    np.add.at(sm, peers, vals)
    mn = np.full(n_ids, KB_CENSUS_NONE, dtype=np.uint32)
    np.minimum.at(mn, peers, vals.astype(np.uint32))
    mx = np.zeros(n_ids, dtype=np.uint32)
    np.maximum.at(mx, peers, vals.astype(np.uint32))
    hist = [0] * KB_LAT_HIST
    for v, c in zip(*np.unique(vals, return_counts=True)):
        hist[bucket(int(v))] += int(c)
    has = np.flatnonzero(mb)
    top = int(has[np.argmax(mx[has])]) if len(has) else KB_CENSUS_NONE       # argmax: the first (lowest id) on ties
    s = {"round": int(round_), "observers": int(observers), "measured": int(len(vals)), "sum_ms": int(vals.sum()),
         "min_ms": int(mn[has].min()) if len(has) else KB_CENSUS_NONE, "max_ms": int(mx[has].max()) if len(has) else 0,
         "max_peer": top, "measured_ids": int(len(has)), "hist": hist, "orphans": int(orphans)}
    if not arrays:
        return LatencyCensus(s)
    rc = np.bincount(rows, minlength=n_rows).astype(np.uint32)
    rsum = np.zeros(n_rows, dtype=np.uint64)
    np.add.at(rsum, rows, vals)
    return LatencyCensus(s, mb, sm, mn, mx, rc, rsum)


def latency_census_of_states(states: dict, capacity: int, arrays: bool = True, round_: int = -1) -> LatencyCensus:
    """The census of observers given as {row id: (peer ids, latency_ms values)}: the entries of each observer's
    peer_states, KB_LATENCY_NONE where nothing was measured.  Orphans cannot be seen through peer_states: 0."""
    peers, rows, vals = [], [], []
    for i, (p, lat) in states.items():
        p, lat = np.asarray(p, dtype=np.int64), np.asarray(lat, dtype=np.uint64)
        keep = lat != KB_LATENCY_NONE
        peers.append(p[keep])
        vals.append(lat[keep])
        rows.append(np.full(int(keep.sum()), i, dtype=np.int64))
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    return _finish(capacity, capacity, len(states), round_, cat(peers, np.int64), cat(rows, np.int64),
                   cat(vals, np.uint64), 0, arrays)


def latency_census_of_arrays(lat, member, running, arrays: bool = True, round_: int = -1) -> LatencyCensus:
    """The census of a whole table: `lat` peer-major [n_ids][n_rows] (0xFFFF = None), `member` [n_rows][n_ids]
    (non-zero: j is in view(i)), `running` [n_rows].  What kb_latency_census_of computes, orphans included."""
    lat = np.asarray(lat, dtype=np.uint16)
    n_ids, n_rows = lat.shape
    mem = (np.asarray(member).reshape(n_rows, n_ids) != 0).T          # [n_ids][n_rows], as lat
    run = np.asarray(running).reshape(n_rows) != 0
    has = (lat != LAT_NONE) & run[None, :]
    peers, rows = np.nonzero(has & mem)
    return _finish(n_ids, n_rows, int(run.sum()), round_, peers, rows, lat[peers, rows], int((has & ~mem).sum()), arrays)


def latency_census_ref(sim, arrays: bool = True) -> LatencyCensus:
    """The latency census of `sim` from `sim.peer_states_array(i)` of the running ids (column 0 of `sim.scalars()`)
    alone: one peer_states call per observer, the test and small-mesh path, and what the CPU oracle answers with.
    On the GPU use Sim.latency_census()."""
    running = np.flatnonzero(sim.scalars()[:, 0] != 0)
    states = {}
    for i in running.tolist():
        ps = sim.peer_states_array(i)
        states[i] = (ps["peer"], ps["latency_ms"])
    return latency_census_of_states(states, sim.capacity, arrays, sim.stats()["round"])
