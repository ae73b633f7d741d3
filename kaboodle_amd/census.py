"""The view census in numpy, and the detection / dissemination tracker built on it.

`Sim.census()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_census (include/kaboodle_census.h), which
counts on the device.  `census_ref` computes the same result from a handle's stamp rows and scalars; it is what
`Sim.census()` falls back to for a library without kb_sim_census (the CPU oracle), so the oracle and the GPU
answer the same call.  `Tracker` turns one census per round into per-id detection and dissemination latencies.
Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

SUMMARY_FIELDS = ("round", "observers", "running", "exact_views", "pairs", "missing", "stale", "full_ids",
                  "ghost_ids", "least_known", "least_known_by", "top_ghost", "top_ghost_by")


@dataclass
class Census:
    """One census: `summary` (the fields of kb_census) and, over all ids, `known_by` (observers whose view holds the
    id), `missing` (running ids the row's view lacks) and `stale` (ids in the row's view that are neither running
    nor external); uint32 arrays, or None when only the summary was asked for.  `running` is the running set the
    census was taken with (bool per id), for the Tracker."""
    summary: dict
    known_by: np.ndarray | None
    missing: np.ndarray | None
    stale: np.ndarray | None
    running: np.ndarray | None = None

    def same_as(self, other: "Census") -> list[str]:
        """The differences to another census (empty: identical summary and arrays)."""
        return diff_results(self, other, ("known_by", "missing", "stale"))


def summarize(round_: int, running: np.ndarray, external: np.ndarray, held: np.ndarray, known_by: np.ndarray,
              view: np.ndarray, missing: np.ndarray, stale: np.ndarray) -> dict:
    """The summary fields from the arrays (running / external / held: bool per id; view: |view(i)| per row)."""
    obs = running & held
    n_obs = int(obs.sum())
    s = {"round": int(round_), "observers": n_obs, "running": int(running.sum()),
         "exact_views": int((obs & (missing == 0) & (stale == 0)).sum()),
         "pairs": int(view[obs].sum(dtype=np.uint64)), "missing": int(missing.sum(dtype=np.uint64)),
         "stale": int(stale.sum(dtype=np.uint64)),
         "full_ids": int((running & (known_by == n_obs)).sum())}
    ghost = ~running & ~external & (known_by > 0)
    s["ghost_ids"] = int(ghost.sum())
    if running.any():
        ids = np.flatnonzero(running)
        k = ids[np.argmin(known_by[ids])]                 # argmin: the first (lowest id) of the smallest
        s["least_known"], s["least_known_by"] = int(k), int(known_by[k])
    else:
        s["least_known"], s["least_known_by"] = KB_CENSUS_NONE, 0
    if ghost.any():
        ids = np.flatnonzero(ghost)
        k = ids[np.argmax(known_by[ids])]
        s["top_ghost"], s["top_ghost_by"] = int(k), int(known_by[k])
    else:
        s["top_ghost"], s["top_ghost_by"] = KB_CENSUS_NONE, 0
    return s


def census_ref(sim, external=None) -> Census:
    """The census of `sim` from `sim.row()` of every running row it holds and `sim.scalars()`: a row entry != 0 is a
    member, column 0 of the scalars is the running set.  `external`: the ids marked by set_external (default: the
    ones the handle recorded); external ids can never be running.

    A test and small-mesh path only: it downloads every row (capacity bytes each) and counts on the host, O(N^2)
    bytes over the bus.  On the GPU use Sim.census()."""
    C = sim.capacity
    running = sim.scalars()[:, 0] != 0
    ext = np.zeros(C, dtype=bool)
    ext[list(sim.external if external is None else external)] = True
    _, _, lo, hi = sim.shard_info()
    held = np.zeros(C, dtype=bool)
    held[lo:hi] = True
    known_by = np.zeros(C, dtype=np.uint32)
    view, missing, stale = (np.zeros(C, dtype=np.uint32) for _ in range(3))
    n_run = int(running.sum())
    stale_class = ~running & ~ext
    for i in np.flatnonzero(running & held):
        m = sim.row(int(i)) != 0
        known_by += m
        view[i] = m.sum()
        missing[i] = n_run - int((m & running).sum())
        stale[i] = int((m & stale_class).sum())
    s = summarize(sim.stats()["round"], running, ext, held, known_by, view, missing, stale)
    return Census(s, known_by, missing, stale, running)


class Tracker:
    """Detection and dissemination latencies from one census per round.

    update(census) compares the census's running set with the previous one's.  For every id that stopped running it
    records `first_dropped`, the first round (census.summary["round"]) with known_by < observers, and `gone`, the
    first round with known_by == 0; for every id that started, `everywhere`, the first round with
    known_by == observers.  The census that first shows the change counts.  An id that changes state again before
    its record completes keeps what was recorded (the missing marks stay -1).  `stopped` / `started` hold the
    latest record of an id; when an id stops (or starts) a second time its earlier record moves to
    `earlier_stopped` / `earlier_started` (lists of (id, record)) and still counts in latencies()."""

    def __init__(self):
        self.prev = None
        self.stopped: dict[int, dict] = {}     # id -> {"at", "first_dropped", "gone"}
        self.started: dict[int, dict] = {}     # id -> {"at", "everywhere"}
        self.earlier_stopped: list[tuple[int, dict]] = []
        self.earlier_started: list[tuple[int, dict]] = []
        self._open_stop: set[int] = set()
        self._open_start: set[int] = set()

    def update(self, census: Census, running=None) -> None:
        run = np.asarray(census.running if running is None else running, dtype=bool)
        r, n_obs, kb = census.summary["round"], census.summary["observers"], census.known_by
        if self.prev is not None:
            for j in np.flatnonzero(self.prev & ~run):
                if int(j) in self.stopped:
                    self.earlier_stopped.append((int(j), self.stopped[int(j)]))
                self.stopped[int(j)] = {"at": r, "first_dropped": -1, "gone": -1}
                self._open_stop.add(int(j))
                self._open_start.discard(int(j))
            for j in np.flatnonzero(~self.prev & run):
                if int(j) in self.started:
                    self.earlier_started.append((int(j), self.started[int(j)]))
                self.started[int(j)] = {"at": r, "everywhere": -1}
                self._open_start.add(int(j))
                self._open_stop.discard(int(j))
        for j in list(self._open_stop):
            rec = self.stopped[j]
            if rec["first_dropped"] < 0 and kb[j] < n_obs:
                rec["first_dropped"] = r
            if kb[j] == 0:
                rec["gone"] = r
                self._open_stop.discard(j)
        for j in list(self._open_start):
            if kb[j] == n_obs:
                self.started[j]["everywhere"] = r
                self._open_start.discard(j)
        self.prev = run.copy()

    def _latency(self, recs: dict, earlier: list, mark: str) -> np.ndarray:
        every = [v for _, v in earlier] + list(recs.values())
        return np.array([v[mark] - v["at"] for v in every if v[mark] >= 0], dtype=np.int64)

    def latencies(self) -> dict:
        """Rounds from the census that first showed the change to each mark, one array per mark (completed records
        only), and how many records are still open."""
        es, ea = self.earlier_stopped, self.earlier_started
        return {"first_dropped": self._latency(self.stopped, es, "first_dropped"),
                "gone": self._latency(self.stopped, es, "gone"), "everywhere": self._latency(self.started, ea, "everywhere"),
                "open_gone": sum(v["gone"] < 0 for v in self.stopped.values()) + sum(v["gone"] < 0 for _, v in es),
                "open_everywhere": sum(v["everywhere"] < 0 for v in self.started.values())
                + sum(v["everywhere"] < 0 for _, v in ea)}

    def histogram(self) -> dict:
        """{mark: counts per latency in rounds (index = latency)} of latencies()."""
        lat = self.latencies()
        return {k: np.bincount(lat[k]).tolist() if len(lat[k]) else [] for k in ("first_dropped", "gone", "everywhere")}
