"""The view-delta census in numpy, and the per-pair detection tracker built on it.

`Sim.delta_census()` (kaboodle_amd/_ffi.py) asks the HIP library's kb_sim_delta_census (include/kaboodle_delta.h),
which compares the member bits with a baseline on the device.  `delta_ref` computes the same result from two member
matrices and their running sets; it is what `Sim.delta_census()` answers with for a library without
kb_sim_delta_census (the CPU oracle, whose baseline `Sim.delta_mark()` keeps on the host), so the oracle and the GPU
answer the same calls.  `PairTracker` turns one advancing delta census per round into the per-(observer, leaver)
detection histogram.  Pure numpy: nothing here needs a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._ffi import KB_CENSUS_NONE, diff_results

SUMMARY_FIELDS = ("round_base", "round", "continuing", "new_rows", "ended_rows", "changed_rows", "changed_ids",
                  "top_false_drop", "top_false_drop_by", "learned", "ghost_adds", "detections", "false_drops",
                  "ext_gained", "ext_lost")
ARRAYS = ("gained_by", "lost_by", "gained", "lost", "lost_live")


@dataclass
class DeltaCensus:
    """One delta census: `summary` (the fields of kb_delta) and, over all ids, `gained_by` / `lost_by` (continuing
    rows whose view gained / lost the id since the mark) and `gained` / `lost` / `lost_live` (ids the row's view
    gained, lost, and lost although they run now); uint32 arrays, or None when only the summary was asked for."""
    summary: dict
    gained_by: np.ndarray | None
    lost_by: np.ndarray | None
    gained: np.ndarray | None
    lost: np.ndarray | None
    lost_live: np.ndarray | None

    def same_as(self, other: "DeltaCensus") -> list[str]:
        """The differences to another delta census (empty: identical summary and arrays)."""
        return diff_results(self, other, ARRAYS)


def summarize(round_base: int, round_: int, run0: np.ndarray, run1: np.ndarray, external: np.ndarray,
              held: np.ndarray, gained_by: np.ndarray, lost_by: np.ndarray, gained: np.ndarray,
              lost: np.ndarray) -> dict:
    """The summary fields from the arrays (run0 / run1 / external / held: bool per id; held: the rows counted).
    Every id is classified by the running and external sets now."""
    dead = ~run1 & ~external
    u64 = lambda a, m: int(a[m].sum(dtype=np.uint64))
    s = {"round_base": int(round_base), "round": int(round_),
         "continuing": int((held & run0 & run1).sum()), "new_rows": int((held & ~run0 & run1).sum()),
         "ended_rows": int((held & run0 & ~run1).sum()), "changed_rows": int(((gained + lost) > 0).sum()),
         "changed_ids": int(((gained_by + lost_by) > 0).sum())}
    live_lost = run1 & (lost_by > 0)
    if live_lost.any():
        ids = np.flatnonzero(live_lost)
        k = ids[np.argmax(lost_by[ids])]                  # argmax: the first (lowest id) of the largest
        s["top_false_drop"], s["top_false_drop_by"] = int(k), int(lost_by[k])
    else:
        s["top_false_drop"], s["top_false_drop_by"] = KB_CENSUS_NONE, 0
    s.update(learned=u64(gained_by, run1), ghost_adds=u64(gained_by, dead), detections=u64(lost_by, dead),
             false_drops=u64(lost_by, run1), ext_gained=u64(gained_by, external), ext_lost=u64(lost_by, external))
    return s


def delta_ref(bits0, run0, bits1, run1, ext, row_lo: int = 0, round_base: int = -1, round_: int = -1) -> DeltaCensus:
    """The delta census from its definitions.  bits0 / bits1: the member matrices at the mark and now, [rows][>= C],
    an entry != 0 is a member (columns at ids >= C are ignored); their rows are the ids row_lo onwards.  run0 / run1 /
    ext: the running sets at the mark and now and the external ids, per id ([C]; C is their length)."""
    run0, run1, ext = (np.asarray(a) != 0 for a in (run0, run1, ext))
    C = len(run1)
    b0, b1 = np.asarray(bits0)[:, :C] != 0, np.asarray(bits1)[:, :C] != 0
    R = b0.shape[0]
    held = np.zeros(C, dtype=bool)
    held[row_lo:row_lo + R] = True
    cont = (run0 & run1)[row_lo:row_lo + R]
    g = b1 & ~b0 & cont[:, None]
    l = b0 & ~b1 & cont[:, None]
    gained, lost, live = (np.zeros(C, dtype=np.uint32) for _ in range(3))
    gained[row_lo:row_lo + R] = g.sum(axis=1)
    lost[row_lo:row_lo + R] = l.sum(axis=1)
    live[row_lo:row_lo + R] = (l & run1[None, :]).sum(axis=1)
    gby, lby = g.sum(axis=0).astype(np.uint32), l.sum(axis=0).astype(np.uint32)
    return DeltaCensus(summarize(round_base, round_, run0, run1, ext, held, gby, lby, gained, lost), gby, lby, gained,
                       lost, live)


def host_state(sim):
    """(member matrix, running set, round) of `sim` from row() of every running row it holds and scalars(): what a
    library without kb_sim_delta_mark keeps as its baseline.  A test and small-mesh path (O(N^2) bytes)."""
    C = sim.capacity
    run = sim.scalars()[:, 0] != 0
    _, _, lo, hi = sim.shard_info()
    bits = np.zeros((hi - lo, C), dtype=bool)
    for i in np.flatnonzero(run[lo:hi]):
        bits[i] = sim.row(int(lo + i)) != 0
    return bits, run, sim.stats()["round"]


def sum_parts(parts, run0, run1, ext) -> DeltaCensus:
    """The delta census of the rows of several disjoint row ranges from the census of each (kb_delta_of's parts, as a
    group adds its shards'): the arrays and the row counts of the summaries add, the rest follows from the sums."""
    run0, run1, ext = (np.asarray(a) != 0 for a in (run0, run1, ext))
    arr = {n: sum((getattr(p, n).astype(np.uint64) for p in parts)).astype(np.uint32) for n in ARRAYS}
    s = summarize(parts[0].summary["round_base"], parts[0].summary["round"], run0, run1, ext, np.ones(len(run1), bool),
                  arr["gained_by"], arr["lost_by"], arr["gained"], arr["lost"])
    for k in ("continuing", "new_rows", "ended_rows"):
        s[k] = sum(p.summary[k] for p in parts)
    return DeltaCensus(s, *(arr[n] for n in ARRAYS))


class PairTracker:
    """Per-(observer, leaver) detection latency from one advancing delta census per round.

    update(delta, running) takes the delta census of the interval that ends now and the running set now.  From
    successive running sets it learns at which census an id stopped (`at[j]`: the round of the first census that
    showed it not running, as census.Tracker does).  For every stopped id j it adds lost_by[j] to
    detect_hist[round - at[j]] (that many observers removed j in this interval) and gained_by[j] to
    relearn_hist[round - at[j]] (that many observers re-inserted it, from stale gossip).  Per census it keeps
    `false_drops`, `ghost_adds`, `continuing` and `rounds` (lists, one entry per update).

    A pair is counted once per removal, not once per pair: an observer that drops a leaver, re-learns it and drops
    it again is counted twice in detect_hist.  relearn_hist shows how often that happens: the removals minus the
    re-insertions up to a latency are the pairs that have detected and still hold their verdict.  Ids that were
    already not running at the first update have no `at` and are left out of both histograms."""

    def __init__(self):
        self.prev = None
        self.at: dict[int, int] = {}
        self.detect_hist: list[int] = []
        self.relearn_hist: list[int] = []
        self.rounds: list[int] = []
        self.false_drops: list[int] = []
        self.ghost_adds: list[int] = []
        self.continuing: list[int] = []

    @staticmethod
    def _add(hist: list, k: int, n: int) -> None:
        if n:
            hist.extend([0] * (k + 1 - len(hist)))
            hist[k] += n

    def update(self, delta: DeltaCensus, running) -> None:
        run = np.asarray(running, dtype=bool)
        r, s = delta.summary["round"], delta.summary
        if self.prev is not None:
            for j in np.flatnonzero(self.prev & ~run):
                self.at[int(j)] = r
            for j in np.flatnonzero(~self.prev & run):
                self.at.pop(int(j), None)
        for j, at in self.at.items():
            self._add(self.detect_hist, r - at, int(delta.lost_by[j]))
            self._add(self.relearn_hist, r - at, int(delta.gained_by[j]))
        self.rounds.append(r)
        self.false_drops.append(s["false_drops"])
        self.ghost_adds.append(s["ghost_adds"])
        self.continuing.append(s["continuing"])
        self.prev = run.copy()

    def latencies(self) -> dict:
        """The per-pair detection histogram (index = rounds from the census that first showed the leaver stopped to
        the census whose interval holds the removal), the re-insertions by the same index, their totals and the
        quantiles of the detection histogram (the smallest latency at which that share of the removals is reached;
        None when nothing was removed)."""
        h = np.asarray(self.detect_hist, dtype=np.int64)
        total = int(h.sum())
        q = {}
        for name, share in (("p50", 0.5), ("p90", 0.9), ("p99", 0.99), ("max", 1.0)):
            q[name] = int(np.searchsorted(np.cumsum(h), share * total, side="left")) if total else None
        return {"detect_hist": list(self.detect_hist), "relearn_hist": list(self.relearn_hist), "removals": total,
                "relearned": int(sum(self.relearn_hist)), "quantiles": q, "stopped_ids": len(self.at)}
